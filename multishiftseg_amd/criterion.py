"""SetCriterion of Mask2Former (lib/network/mask2former/modeling/criterion.py:91-488) on the HIP kernels of csrc/m2f_loss.hip and
csrc/m2f_mix.hip.

The reference walks the prediction steps one by one and, per step, composes torch.rand, three grid_samples, a topk, a gather and two
jit-scripted loss functions over the matched masks; its backward scatters through grid_sample with float atomics. Here the class
loss and the sampled mask losses of ALL S steps (the last output and its aux_outputs), all images and all matched masks are five
launches (three forward, two backward) after the matcher's two, with no device-to-host copy, and two runs give the same bits.
There is no CPU path.

`loss_ood` (criterion.py:128-187) is here in all three branches. `RCL` (what exps/M2F.yaml selects through
replace_official_odd_loss_with_RCL): per step two autograd nodes of `class_mix_upsample` -- the class mix of (pred_logits, pred_masks)
upsampled and cropped to the 19 logit maps, and that of (pred_logits_ood, pred_masks_ood) reduced to -max over the classes at full
size -- followed by `extra_loss(logits, score, target)`. `margin` (the reference's default: mask2former/config.py:118-119,
train_m2f.py:157-158 with lib/configs/config.py:44) and `bce`: per step one node `ood_loss.class_mix_ood_loss` over (pred_logits,
pred_masks) and the stacked ood_mask -- -max over the classes at the LOW resolution, the one-channel score interpolated with
align_corners=True to the size of ood_mask, two masked means. In every branch the mix and the sigmoids stay at the low resolution,
the backward gathers (no float atomics) and stores no argmax map: it recomputes it. `margin` and `bce` have no CPU path: with
tensors that are not on the device they raise NotImplementedError before any other check.

Deviations from the reference, all deliberate:
  * the random numbers have the reference's distribution, not its draw order (one torch.rand per kind for all rows of all steps);
  * ties at the k-th largest key go to the lowest candidate index (torch.topk leaves them unspecified);
  * loss_masks_aug: a half of the batch without masks gives 0 for its two terms (the reference divides by zero: NaN);
  * mask_loss_with_pixel_selection is a constructor argument (the reference reads a global config, criterion.py:424-426);
  * weight_dict is stored and shown, not applied (the reference applies it in maskformer_model.py);
  * a problem the matcher could not solve, or a label outside [0, num_classes), makes every loss of its step NaN and the step's
    gradients 0, with no host synchronisation (the reference raises inside scipy / indexes out of range);
  * loss_ood: where two classes tie for the maximum of the interpolated mix, the gradient of the score goes to the lowest class
    index (torch.max leaves that unspecified);
  * loss_ood: when pred_masks_ood is pred_masks, the two nodes each compute their own sigmoids and autograd adds the two mask
    gradients; the sum is the same as for two separate tensors;
  * loss_ood: a pixel-major step reads "pred_masks_ood_pixel_major", or "pred_masks_pixel_major" where that key is absent (this
    package's decoder shares the tensor); sem_seg may be a device tensor, which is then never copied to the host.
"""
import numpy as np
import torch
from torch import nn

from . import kernels as K
from .matcher import _steps_of
from .ood_loss import class_mix_ood_loss

CLEAN_OVERSAMPLE_RATIO = 1 / 0.8            # criterion.py:374-376: hard-coded in get_clean_point_coords_with_randomness
CLEAN_IMPORTANCE_SAMPLE_RATIO = 0.95

PLAIN_KEYS = ("loss_ce", "loss_mask", "loss_dice")
AUG_KEYS = ("loss_ce", "loss_original_mask", "loss_original_dice", "loss_aug_mask", "loss_aug_dice")


def selection_counts(num_points, oversample_ratio, importance_sample_ratio):
    """(K candidates, k kept) of one row, the integers exactly as the reference writes them (criterion.py:382,387)."""
    return int(num_points * oversample_ratio), int(importance_sample_ratio * num_points)


class _Plan:
    """Everything of one call that is not differentiated: the packed targets, the match table, the points and the row groups."""
    __slots__ = ("tmask", "tstart", "labels", "match", "points", "weight", "scales", "split", "num_points", "pixel_major", "Q", "S",
                 "want_masks")


class _CriterionFunction(torch.autograd.Function):
    """One function spans all steps: inputs = every step's mask logits, then every step's class logits; output = the loss table
    [S, 3] (or [S, 5]); the dict entries of SetCriterion.forward are views of it."""

    @staticmethod
    def forward(ctx, plan, *tensors):
        S = plan.S
        masks, logits = list(tensors[:S]), list(tensors[S:])
        rows = None
        if plan.want_masks:
            rows = K.m2f_mask_loss(masks, plan.tmask, plan.tstart, plan.match, plan.points, pixel_major=plan.pixel_major, Q=plan.Q)
        loss, tclass, bad, wsum = K.m2f_label_loss(logits, plan.labels, plan.tstart, plan.match, plan.weight, rows, plan.num_points,
                                                   plan.scales, plan.split)
        ctx.plan = plan                 # the packed targets, the match table and the points: held until the graph is freed
        ctx.save_for_backward(*tensors, tclass, bad, wsum, *([rows] if rows is not None else []))
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss):
        plan = ctx.plan
        S = plan.S
        saved = ctx.saved_tensors
        masks, logits = list(saved[:S]), list(saved[S:2 * S])
        tclass, bad, wsum = saved[2 * S:2 * S + 3]
        gloss = gloss.contiguous().float()
        gm = [None] * S
        if plan.want_masks and any(ctx.needs_input_grad[1:1 + S]):
            g = K.m2f_mask_loss_backward(masks, plan.tmask, plan.tstart, plan.match, bad, plan.points, saved[2 * S + 3], gloss, plan.scales,
                                         plan.split, pixel_major=plan.pixel_major, Q=plan.Q)
            gm = [g[s] for s in range(S)]
        gl = [None] * S
        if any(ctx.needs_input_grad[1 + S:]):
            g = K.m2f_label_loss_backward(logits, tclass, bad, plan.weight, wsum, gloss)
            gl = [g[s] for s in range(S)]
        return (None, *gm, *gl)


class _ClassMixUpsample(torch.autograd.Function):
    """One node for softmax, sigmoid, einsum, interpolate, crop and (mode "neg_max") -max over the classes."""

    @staticmethod
    def forward(ctx, class_logits, mask_logits, size, crop, mode, pixel_major, Q):
        mix, prob = K.m2f_class_mix(class_logits, mask_logits, pixel_major=pixel_major, Q=Q)
        out = K.m2f_mix_upsample(mix, size, crop, mode)
        ctx.save_for_backward(class_logits, mask_logits, mix, prob)
        ctx.cfg = (size, crop, mode, pixel_major, Q)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        class_logits, mask_logits, mix, prob = ctx.saved_tensors
        size, crop, mode, pixel_major, Q = ctx.cfg
        g = g.contiguous().float()
        dmix = K.m2f_mix_upsample_backward(mix, size, crop, **{"dlogits" if mode == "logits" else "dscore": g})
        dmasks, dcls = K.m2f_class_mix_backward(dmix, prob, class_logits, mask_logits, pixel_major=pixel_major, Q=Q)
        return dcls, dmasks, None, None, None, None, None


def class_mix_upsample(class_logits, mask_logits, size, crop=None, mode="logits", pixel_major=False, Q=None):
    """interpolate(einsum("bqc,bqhw->bchw", softmax(class_logits, -1)[..., :-1], sigmoid(mask_logits)), size, bilinear,
    align_corners=False)[:, :, :crop[0], :crop[1]] as ONE differentiable op (criterion.py:133-138, :166-168, :170-181).
    mode "logits": its first min(C, 19) channels [B,Cl,Ht,Wt]; "neg_max": -max over all C channels [B,Ht,Wt]. class_logits
    [B,Q,C+1], mask_logits [B,Q,h,w] or, with pixel_major, [B,h,w,ldq]; float32 on the device. Gradients reach both inputs; where
    classes tie for the maximum, the lowest class index takes the gradient."""
    if mode not in ("logits", "neg_max"):
        raise ValueError(f"class_mix_upsample: mode {mode!r} is not 'logits' or 'neg_max'")
    size = (int(size[0]), int(size[1]))
    crop = size if crop is None else (int(crop[0]), int(crop[1]))
    return _ClassMixUpsample.apply(class_logits.float().contiguous(), mask_logits.float().contiguous(), size, crop, mode, bool(pixel_major),
                                   None if Q is None else int(Q))


class SetCriterion(nn.Module):
    """The loss of Mask2Former's stage 2 (criterion.py:91-96): the Hungarian assignment between targets and predictions, then the
    class loss and the sampled mask losses of every matched pair. Constructor, set_extra_loss, forward()'s dict and __repr__ of
    the reference; `mask_loss_with_pixel_selection` selects loss_masks_aug (:244-310) instead of loss_masks (:312-363)."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio, importance_sample_ratio,
                 ood_loss=None, margin=None, deep_supervision=False, mask_loss_with_pixel_selection: bool = False):
        super().__init__()
        self.num_classes, self.matcher, self.weight_dict, self.eos_coef, self.losses = num_classes, matcher, weight_dict, eos_coef, losses
        self.num_points, self.oversample_ratio, self.importance_sample_ratio = num_points, oversample_ratio, importance_sample_ratio
        self.ood_loss, self.margin, self.deep_supervision = ood_loss, margin, deep_supervision
        self.extra_loss = None
        weight = torch.ones(num_classes + 1)                # the class weights of F.cross_entropy: eos_coef for "no object"
        weight[-1] = eos_coef
        self.register_buffer("empty_weight", weight)
        self.mask_loss_with_pixel_selection = mask_loss_with_pixel_selection
        # Set keep_tables to have a call leave its point table [S * sum T, num_points, 2] and the matcher's table [S, B, Tmax] int32
        # (both on the device) in last_points / last_match, for tests and diagnosis. Off by default: the point table is
        # S * sum T * num_points * 8 bytes, about 190 MB at C4, and would stay allocated between calls.
        self.keep_tables = False
        self.last_points = None
        self.last_match = None

    def selection(self):
        """(mode, K, k) of the rows that select their points (criterion.py:335-341; :374-387 for loss_masks_aug)."""
        if self.mask_loss_with_pixel_selection:
            return ("clean",) + selection_counts(self.num_points, CLEAN_OVERSAMPLE_RATIO, CLEAN_IMPORTANCE_SAMPLE_RATIO)
        assert self.oversample_ratio >= 1 and 0 <= self.importance_sample_ratio <= 1
        return ("uncertain",) + selection_counts(self.num_points, self.oversample_ratio, self.importance_sample_ratio)

    def _check_ood(self):
        """Which loss_ood this is (criterion.py:140-185), before anything is computed."""
        if self.ood_loss == "RCL":
            if self.extra_loss is None:                         # the reference asserts (criterion.py:163)
                raise NotImplementedError("loss_ood with ood_loss 'RCL' needs an extra_loss: call set_extra_loss(RelContrastiveLoss(...)) first")
        elif self.ood_loss not in ("margin", "bce"):        # those two: _refuse_host, with the call's tensors
            raise ValueError("define_ood_loss")

    def _refuse_host(self, outputs):
        """ood_loss 'margin' / 'bce' (criterion.py:140-161) with tensors that are not on the device: before any other check."""
        if self.ood_loss in ("margin", "bce") and not all(v.is_cuda for v in outputs.values() if isinstance(v, torch.Tensor)):
            raise NotImplementedError(f"SetCriterion.loss_ood with ood_loss {self.ood_loss!r} runs on an MI355X only (CUDA tensors); "
                                      "there is no CPU path")

    def _check_losses(self):
        for loss in self.losses:
            if loss == "ood":
                self._check_ood()
                continue
            assert loss in ("labels", "masks"), f"do you really want to compute {loss} loss?"

    def loss_ood(self, outputs, targets):
        """criterion.py:128-187 for one prediction step. ood_loss "margin" / "bce": see _loss_ood_pixel. "RCL": outputs holds pred_logits, pred_masks (or pred_masks_pixel_major),
        pred_logits_ood and pred_masks_ood; targets per image "ood_mask" (only its shape (H, W) is used) and "sem_seg" [Ht,Wt]
        (numpy array or tensor). extra_loss gets a fresh int64 copy of the stacked sem_seg, as the reference's torch.tensor(target):
        RelContrastiveLoss changes it in place. -> {"loss_ood": 0-d tensor}."""
        self._refuse_host(outputs)
        self._check_ood()
        pixel_major = "pred_masks" not in outputs
        if self.ood_loss in ("margin", "bce"):
            return {"loss_ood": self._loss_ood_pixel(outputs, targets, pixel_major)}
        cls, cls_ood = outputs["pred_logits"], outputs["pred_logits_ood"]
        if pixel_major:
            masks = outputs["pred_masks_pixel_major"]
            masks_ood = outputs.get("pred_masks_ood_pixel_major", masks)
        else:
            masks, masks_ood = outputs["pred_masks"], outputs["pred_masks_ood"]
        if not all(t.is_cuda for t in (cls, cls_ood, masks, masks_ood)):
            raise RuntimeError("SetCriterion.loss_ood runs on an MI355X only (CUDA tensors); there is no CPU path")
        dev = cls.device
        size = tuple(int(v) for v in targets[0]["ood_mask"].shape[-2:])
        sem = [t["sem_seg"] for t in targets]
        if all(isinstance(t, torch.Tensor) for t in sem):
            target = torch.stack([t.to(dev) for t in sem]).to(torch.int64)          # stack: a new tensor even where nothing converts
        else:
            sem = [t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in sem]
            target = torch.from_numpy(np.stack(sem)).to(dev).to(torch.int64)       # np.stack and the upload: a new tensor
        crop = tuple(int(v) for v in target.shape[-2:])
        Q = cls.shape[1]
        logits = class_mix_upsample(cls, masks, size, crop, "logits", pixel_major=pixel_major, Q=Q)
        score = class_mix_upsample(cls_ood, masks_ood, size, crop, "neg_max", pixel_major=pixel_major, Q=Q)
        return {"loss_ood": self.extra_loss(logits, score, target)}

    def _loss_ood_pixel(self, outputs, targets, pixel_major):
        """criterion.py:130-161 for one prediction step: pred_logits with pred_masks (or pred_masks_pixel_major), not the _ood heads;
        targets per image "ood_mask" [H,W], stacked: a uint8 or bool stack as it is, another dtype through == 1 / == 0. sem_seg and
        extra_loss are not read."""
        cls = outputs["pred_logits"]
        masks = outputs["pred_masks_pixel_major" if pixel_major else "pred_masks"]
        ood = torch.stack([t["ood_mask"] if isinstance(t["ood_mask"], torch.Tensor) else torch.as_tensor(t["ood_mask"]) for t in targets])
        if ood.dim() == 4 and ood.shape[1] == 1:                # [B,1,H,W]: the reference squeezes that axis (:144-145)
            ood = ood[:, 0]
        return class_mix_ood_loss(cls, masks, ood.to(cls.device), self.ood_loss, self.margin, pixel_major=pixel_major, Q=cls.shape[1])

    def forward(self, outputs, targets, *, num_masks=None, point_candidates=None, random_points=None, matcher_points=None):
        """The loss computation (criterion.py:432-469). outputs: {"pred_logits" [B,Q,C+1], "pred_masks" [B,Q,h,w] (or
        "pred_masks_pixel_major" [B,h,w,ldq]), "aux_outputs": [the same per earlier step]}; targets: per image {"labels" [T_b],
        "masks" [T_b,H,W]}. Returns {loss_ce, loss_mask, loss_dice} (or the four keys of loss_masks_aug), then `<key>_<i>` for
        aux_outputs[i] when deep_supervision is set: 0-d float32 device tensors attached to autograd, weight_dict NOT applied.
        With "ood" in losses every step also needs "pred_logits_ood" / "pred_masks_ood" and every target "ood_mask" / "sem_seg"
        (ood_loss "RCL"; "margin" and "bce" need "ood_mask" alone: see loss_ood), and "loss_ood" / "loss_ood_<i>" take their place in
        the order of `losses`.
        num_masks: overrides max(sum T_b, 1). point_candidates [S, rows that select, K, 2], random_points [S * sum T, Pr, 2],
        matcher_points [S,B,P,2]: inject the random numbers (see kernels.m2f_point_select / HungarianMatcher.match_steps)."""
        if "ood" in self.losses:
            self._refuse_host(outputs)
        self._check_losses()
        steps = _steps_of(outputs) if self.deep_supervision else _steps_of({k: v for k, v in outputs.items() if k != "aux_outputs"})
        S = len(steps)
        pixel_major = "pred_masks" not in steps[0]
        masks = [o["pred_masks_pixel_major" if pixel_major else "pred_masks"] for o in steps]
        logits = [o["pred_logits"] for o in steps]
        if not all(t.is_cuda for t in masks + logits):
            raise RuntimeError("SetCriterion runs on an MI355X only (CUDA tensors); there is no CPU path")
        dev = logits[0].device
        B, Q, C1 = logits[0].shape
        if C1 != self.num_classes + 1:
            raise ValueError(f"pred_logits have {C1} classes, the criterion {self.num_classes} + 1")
        packed = self.matcher._pack_targets(targets, dev)
        tmask, tstart, labels, counts = packed
        match = self.matcher.match_steps(steps, targets, point_coords=matcher_points, device_only=True, packed=packed)
        total_t = sum(counts)
        P = int(self.num_points)
        masks = [m.float() for m in masks]
        logits = [c.float() for c in logits]

        plan = _Plan()
        plan.tmask, plan.tstart, plan.labels, plan.match = tmask, tstart, labels, match
        plan.weight = self.empty_weight.to(device=dev, dtype=torch.float32)
        plan.num_points, plan.pixel_major, plan.Q, plan.S = P, pixel_major, Q, S
        plan.want_masks = "masks" in self.losses
        want_labels = "labels" in self.losses
        mode, n_cand, n_keep = self.selection()
        if self.mask_loss_with_pixel_selection:
            plan.split = sum(counts[:B // 2])                   # criterion.py:255: images b < B/2 are "original", the rest "aug"
            n_orig, n_aug = plan.split, total_t - plan.split
            plan.scales = (2.0 / n_orig if n_orig else 0.0, 1.0 / n_aug if n_aug else 0.0)
            sel_start, keys = plan.split, AUG_KEYS
        else:
            if num_masks is None:
                num_masks = max(total_t, 1)                     # criterion.py:447-453 for one process; over ranks M2FTrainStep passes ddp.global_num_masks
            plan.split = None
            plan.scales = (1.0 / float(num_masks),)
            sel_start, keys = 0, PLAIN_KEYS
        plan.points = None
        if plan.want_masks:
            with torch.no_grad():
                n_random = P if (sel_start > 0 or n_keep == 0) else P - n_keep
                if point_candidates is None and n_keep > 0:
                    point_candidates = torch.rand((S, total_t - sel_start, n_cand, 2), device=dev)
                if random_points is None:
                    random_points = torch.rand((S * total_t, n_random, 2), device=dev)
                plan.points = K.m2f_point_select([m.detach() for m in masks], tmask, tstart, match, point_candidates if n_keep > 0 else None,
                                                 random_points, n_keep, P, mode=mode, sel_start=sel_start, pixel_major=pixel_major, Q=Q)
        self.last_points, self.last_match = (plan.points, match) if self.keep_tables else (None, None)

        table = _CriterionFunction.apply(plan, *masks, *logits) if (want_labels or plan.want_masks) else None
        losses = {}
        for s in range(S):
            suffix = "" if s == 0 else f"_{s - 1}"
            for loss in self.losses:                            # criterion.py:455-467: per step, the losses in the order of self.losses
                if loss == "ood":
                    losses["loss_ood" + suffix] = self.loss_ood(steps[s], targets)["loss_ood"]
                    continue
                for j, key in enumerate(keys):
                    if (j == 0) == (loss == "labels"):
                        losses[key + suffix] = table[s, j]
        return losses

    def set_extra_loss(self, extra_loss):
        self.extra_loss = extra_loss

    def __repr__(self):
        pad = " " * 4
        shown = ("losses", "weight_dict", "num_classes", "eos_coef", "num_points", "oversample_ratio", "importance_sample_ratio")
        return "\n".join([f"Criterion {type(self).__name__}", f"{pad}matcher: {self.matcher.__repr__(_repr_indent=8)}"]
                         + [f"{pad}{k}: {getattr(self, k)}" for k in shown])
