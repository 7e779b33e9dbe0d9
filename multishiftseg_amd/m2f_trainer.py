"""The stage-2 training step of Mask2Former around the HIP optimizer (optim.AdamW): the parameter groups and the optimizer of
train_m2f.py:211-299, the weight dict of maskformer_model.py:143-153 and its application :253-258, and M2FTrainStep, which runs
zero_grad / head / criterion / weighted sum / backward / clipped AdamW step. The reference reads every value from a detectron2
config; here each is an argument.
Stage 1 (the epochs before warmup_epoch, train_m2f.py:437-447): M2FStage1Step trains class_embed2 alone under optim.Adam with
RelContrastiveLoss on MaskFormer.stage1_forward's (sem_seg, ood_score).

Data parallel (one process per GPU; the reference wraps the model in nn.DataParallel, train_m2f.py:121-123): both steps take a
process `group`. With torch.distributed initialised and more than one rank in it (or MSS_DDP_FORCE=1, the switch of
trainer.TrainStep) a step broadcasts rank 0's trainable parameters once, attaches one ddp.GradAllReduce to the optimizer's tensors
(hook mode, buckets in the reverse of the parameter-group order) and runs backward -> sync.backward_done() -> optimizer.step(), so
clipping and the update act on the averaged gradients and every rank makes the same update. Each rank steps on its own
[orig...; aug...] batch (ddp.shard_pairs): the pairing of the criterion and of the loss stays rank-local, and so do the returned
losses. Stage 2 normalises the mask losses by ddp.global_num_masks of all ranks' target counts (reference criterion.py:447-453),
one tiny collective per step. Without a process group nothing changes."""
import torch
from torch import nn

from . import ddp
from .optim import Adam, AdamW
from .trainer import configure_trainable_params

# train_m2f.py:233-244
NORM_MODULE_TYPES = (
    nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm, nn.GroupNorm, nn.InstanceNorm1d, nn.InstanceNorm2d,
    nn.InstanceNorm3d, nn.LayerNorm, nn.LocalResponseNorm,
)


def build_m2f_param_groups(model, base_lr, weight_decay, weight_decay_norm=0.0, weight_decay_embed=0.0, backbone_multiplier=0.1):
    """train_m2f.py:246-265: one {"params": [tensor], "lr", "weight_decay"} group per trainable tensor, in named_modules() order,
    each tensor once (by identity; a tensor shared under two names takes the rules of its first name). lr = base_lr, times
    backbone_multiplier where the MODULE name contains "backbone"; weight decay = weight_decay, then 0 for a parameter named
    relative_position_bias_table / absolute_pos_embed, then weight_decay_norm inside a norm module, then weight_decay_embed inside
    an nn.Embedding: a later rule overrides an earlier one."""
    groups, memo = [], set()
    for module_name, module in model.named_modules():
        for param_name, p in module.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in memo:
                continue
            memo.add(id(p))
            lr, wd = base_lr, weight_decay
            if "backbone" in module_name:
                lr = lr * backbone_multiplier
            if "relative_position_bias_table" in param_name or "absolute_pos_embed" in param_name:
                wd = 0.0
            if isinstance(module, NORM_MODULE_TYPES):
                wd = weight_decay_norm
            if isinstance(module, nn.Embedding):
                wd = weight_decay_embed
            groups.append({"params": [p], "lr": lr, "weight_decay": wd})
    return groups


def build_m2f_optimizer(model, base_lr=1e-5, weight_decay=0.05, weight_decay_norm=0.0, weight_decay_embed=0.0, backbone_multiplier=0.1,
                        optimizer="ADAMW", clip_value=0.01):
    """train_m2f.py:267-299 for OPTIMIZER "ADAMW" with CLIP_GRADIENTS of type "full_model": AdamW over build_m2f_param_groups with
    clip_grad_norm_(all parameters, clip_value) inside every step (clip_value 0 / None: no clipping, as the reference's
    `clip_norm_val > 0.0`). Defaults: anomaly_ft.yaml:5 and Base-Cityscapes-SemanticSegmentation.yaml:25-33."""
    if optimizer != "ADAMW":
        raise NotImplementedError(f"build_m2f_optimizer has ADAMW only (no optimizer type {optimizer})")
    groups = build_m2f_param_groups(model, base_lr, weight_decay, weight_decay_norm, weight_decay_embed, backbone_multiplier)
    return AdamW(groups, lr=base_lr, max_norm=clip_value or None)


def m2f_weight_dict(class_weight, mask_weight, dice_weight, ood_weight, dec_layers, deep_supervision):
    """maskformer_model.py:143-153: the eight weighted keys, and with deep supervision `<key>_<i>` for i < dec_layers - 1."""
    weight_dict = {"loss_ce": class_weight, "loss_mask": mask_weight, "loss_dice": dice_weight, "loss_ood": ood_weight,
                   "loss_original_mask": mask_weight, "loss_original_dice": dice_weight, "loss_aug_mask": mask_weight,
                   "loss_aug_dice": dice_weight}
    if deep_supervision:
        aux = {}
        for i in range(dec_layers - 1):
            aux.update({f"{k}_{i}": v for k, v in weight_dict.items()})
        weight_dict.update(aux)
    return weight_dict


def weighted_losses(losses, weight_dict):
    """maskformer_model.py:253-258 out of place: {k: losses[k] * weight_dict[k]} for the keys of `losses` that `weight_dict` has, in
    the order of `losses`; the others are dropped. A new dict of new tensors: the criterion's entries are views of one table."""
    return {k: v * weight_dict[k] for k, v in losses.items() if k in weight_dict}


def target_count(targets):
    """sum_b T_b of a batch's targets, from the host: an M2FTargets holds its counts, a list of dicts the label shapes."""
    packed = getattr(targets, "packed", None)
    if packed is not None:
        return int(sum(packed[3]))
    return sum(int(t["labels"].shape[0]) for t in targets)


def attach_grad_sync(params, module=None, group=None, bucket_bytes=64 << 20, sync_params=True, close_after_bytes=16 << 20):
    """The data-parallel half of a step's construction, or None where ddp.is_active(group) says one process: broadcast rank 0's
    `params` (sync_params), then one ddp.GradAllReduce over them in hook mode. Buckets follow the REVERSE of `params` (the
    parameter-group order runs backbone -> pixel decoder -> predictor, the backward the other way round; the order only matters
    for overlap, and it is the same on every rank because it never looks at a gradient). Names: the module's, else param<i>."""
    if not ddp.is_active(group):
        return None
    params = list(params)
    if sync_params:
        ddp.broadcast_params(params, group)
    names = {id(p): n for n, p in module.named_parameters()} if isinstance(module, nn.Module) else {}
    named = [(names.get(id(p), f"param{i}"), p) for i, p in enumerate(params)]
    return ddp.GradAllReduce(list(reversed(named)), bucket_bytes, group=group, force=True,
                             close_after_bytes=close_after_bytes).attach()


class M2FTrainStep:
    """One stage-2 step: optimizer.zero_grad() ; outputs = head(*head_args) ; criterion(outputs, targets, **criterion_kwargs) ;
    weighted_losses with the criterion's weight_dict ; sum ; backward ; optimizer.step(). `head` is any callable that returns the
    outputs dict (MultiScaleMaskedTransformerDecoder_GMA.set_trainable(), alone or behind the pixel decoder). Returns (the
    detached weighted losses, the total gradient norm before clipping as a 0-d device tensor, None without clipping).

    Over a process group (`group`; active as ddp.is_active says, `self.sync` is then the gradient sink and None otherwise): rank
    0's trainable parameters are broadcast at construction (sync_params), every rank calls the step on its own [orig...; aug...]
    batch, the gradients are averaged in buckets of `bucket_bytes` while the backward runs, and the optimizer -- the full-model
    clip included -- acts on the average: the returned norm is the norm of the averaged gradient, equal on every rank, and so is
    the update. The criterion runs with num_masks = max(sum over ranks of sum_b T_b / world, 1) (`self.last_num_masks`; a
    num_masks among criterion_kwargs wins; a criterion with mask_loss_with_pixel_selection normalises per half batch and ignores
    it). The returned losses are this rank's own, normalised that way: they are not averaged over ranks. One step at a time
    holds a model's tensors: building a second one over a process group raises until the first is close()d (the stage switch). loss_ood's
    RelContrastiveLoss may be sync="local" or "global" (the global form's gradients come multiplied by the world size, which the
    averaging undoes, see trainer.TrainStep). An exception before the optimizer step starts no further collective
    (sync.abort()) and is raised on."""

    def __init__(self, head, criterion, optimizer, group=None, bucket_bytes=64 << 20, sync_params=True):
        self.head, self.criterion, self.optimizer = head, criterion, optimizer
        self.sync = attach_grad_sync(optimizer.params, head, group, bucket_bytes, sync_params)
        self.counts = ddp.CountAllReduce(group) if self.sync is not None else None
        self.last_num_masks = None
        self.closed = False

    def close(self):
        """Release the parameters: the gradient hooks are removed, so that another step (the other stage, a new optimizer) can be
        built on the same model. A tensor hands its gradient to one sink at a time; a closed step raises when it is called."""
        if self.sync is not None:
            self.sync.detach()
        self.closed = True

    def _backward(self, head_args, targets, criterion_kwargs):
        given = self.sync is None or criterion_kwargs.get("num_masks") is not None
        if not given:
            self.counts.start(target_count(targets))             # travels beside the forward
        outputs = self.head(*head_args)
        if not given:
            criterion_kwargs["num_masks"] = self.counts.result()
        if self.sync is not None:
            self.last_num_masks = float(criterion_kwargs["num_masks"])
        losses = weighted_losses(self.criterion(outputs, targets, **criterion_kwargs), self.criterion.weight_dict)
        if not losses:
            raise ValueError("M2FTrainStep: no loss of the criterion has a weight in its weight_dict")
        sum(losses.values()).backward()
        return losses

    def __call__(self, *head_args, targets, **criterion_kwargs):
        if self.closed:
            raise RuntimeError("M2FTrainStep: the step was closed (its gradient hooks are gone); build a new one")
        self.optimizer.zero_grad(set_to_none=True)
        if self.sync is None:
            losses = self._backward(head_args, targets, criterion_kwargs)
        else:
            try:
                losses = self._backward(head_args, targets, criterion_kwargs)
            except BaseException:
                self.counts.drop()
                self.sync.abort()
                raise
            self.sync.backward_done()
        norm = self.optimizer.step()
        return {k: v.detach() for k, v in losses.items()}, norm


class M2FStage1Step:
    """One stage-1 step (train_m2f.py:414-456 for epoch < warmup_epoch; M2F.yaml:9, 24-27): only the parameters whose name contains
    one of `patterns` train (trainer.configure_trainable_params sets every requires_grad), under the HIP Adam with torch's L2
    weight decay. __call__(images, target): zero_grad ; (sem_seg, ood_score) = model.stage1_forward(images) ;
    loss(sem_seg, ood_score, target).mean() ; backward ; step -> the detached loss. `loss` is RelContrastiveLoss (it needs an even
    batch [orig...; aug...] and changes `target` in place, as the reference's does).

    Over a process group (as M2FTrainStep): the trained tensors are broadcast from rank 0 and their gradients averaged in ONE
    bucket (`self.sync`) before Adam; no other parameter receives a gradient. The returned loss is this rank's own. close()
    before M2FTrainStep is built on the same model."""

    def __init__(self, model, loss, lr=1e-4, weight_decay=1e-4, patterns=("class_embed2",), group=None, sync_params=True):
        self.model, self.loss = model, loss
        params, self.names = configure_trainable_params(model, tuple(patterns))
        if not params:
            raise ValueError(f"M2FStage1Step: no parameter name contains one of {tuple(patterns)}")
        self.optimizer = Adam(params, lr=lr, weight_decay=weight_decay)
        self.sync = attach_grad_sync(params, model, group, sum(p.numel() * p.element_size() for p in params), sync_params,
                                     close_after_bytes=0)
        self.closed = False

    def close(self):
        """The stage switch (train_m2f.py: update_trainable_params): remove the gradient hooks from the trained tensors, so that
        M2FTrainStep can be built on the same model; re-enabling requires_grad of the rest is the caller's. A closed step raises."""
        if self.sync is not None:
            self.sync.detach()
        self.closed = True

    def _backward(self, images, target):
        sem_seg, ood_score = self.model.stage1_forward(images)
        loss = self.loss(sem_seg, ood_score, target).mean()
        loss.backward()
        return loss

    def __call__(self, images, target):
        if self.closed:
            raise RuntimeError("M2FStage1Step: the step was closed (its gradient hooks are gone); build a new one")
        self.optimizer.zero_grad(set_to_none=True)
        if self.sync is None:
            loss = self._backward(images, target)
        else:
            try:
                loss = self._backward(images, target)
            except BaseException:
                self.sync.abort()
                raise
            self.sync.backward_done()
        self.optimizer.step()
        return loss.detach()
