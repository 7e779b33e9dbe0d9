"""Test helper: stage 1 of the reference's Mask2Former recipe restated in stock torch at a chosen dtype, differentiable.

    up      = F.interpolate(pred_masks, size=(Hp, Wp), mode="bilinear", align_corners=False)        maskformer_model.py:264-277
    semseg  = einsum("qc,qhw->chw", softmax(pred_logits, -1)[..., :-1], sigmoid(up))                 :343-345, per image
    sem_seg = semseg[:, :H, :W]                                  sem_seg_postprocess: the crop; its same-size resize is the identity
    logit   = sem_seg[:19]                                                                           train_m2f.py:439-442
    score   = 1 - max_c einsum("bqc,bqhw->bchw", softmax(pred_logits_ood)[..., :-1], sigmoid(up))[:, :, :H, :W]      :399-407
    loss    = RelContrastiveLoss(logit, score, target).mean()                                        :447, lib/loss.py:34-156
    step    = torch.optim.Adam(class_embed2, lr, weight_decay)                                       :454-456, M2F.yaml:9, 24-27

Mask logits are NCHW [B,Q,hm,wm] here. Where several classes share the maximum the lowest class index counts, the rule of the HIP
kernels (ref_class_mix.first_max). The loss is restated without pixel selection (M2F.yaml sets none); its three random
permutations are drawn from torch's default CPU generator in the reference's order, so the same torch.manual_seed gives the same
pairs as RelContrastiveLoss(pairing="reference")."""
import torch
import torch.nn.functional as F

from ref_class_mix import LOGIT_CHANNELS, first_max

IN_ID, VOID_ID = 99, 255


def upsampled(mask_logits, image_size):
    return F.interpolate(mask_logits, size=tuple(image_size), mode="bilinear", align_corners=False)


def class_maps(class_logits, mask_logits, image_size, size):
    """All C class maps [B,C,H,W] of a head on the upsampled masks, cropped."""
    prob = torch.softmax(class_logits, -1)[..., :-1]
    full = torch.einsum("bqc,bqhw->bchw", prob, torch.sigmoid(upsampled(mask_logits, image_size)))
    return full[:, :, :size[0], :size[1]]


def sem_seg(class_logits, mask_logits, image_size, size):
    return class_maps(class_logits, mask_logits, image_size, size)[:, :LOGIT_CHANNELS]


def ood_score(class_logits_ood, mask_logits, image_size, size):
    return 1 - first_max(class_maps(class_logits_ood, mask_logits, image_size, size))


def draw_perms(target):
    """The three torch.randperm draws of lib/loss.py:129-131 for `target`, from the default generator."""
    h = target.shape[0] // 2
    in_mask = target < IN_ID
    ood_mask = (target > IN_ID) & (target != VOID_ID)
    return tuple(torch.randperm(int(k)) for k in (in_mask[:h].sum(), in_mask[h:].sum(), ood_mask.sum()))


def rel_contrastive_loss(logits, score, target, params, perms):
    """lib/loss.py:34-88, 119-156 without pixel selection -> (loss, the hinge arguments of all three terms, for the kink check)."""
    w0, w1 = params.get("ce_weights", [1, 1])
    m = params["inoutaug_contras_margins_tri"]
    wc = params.get("contras_weight", 1.0)
    B = logits.shape[0]
    h = B // 2
    in_mask = target < IN_ID
    ood_mask = (target > IN_ID) & (target != VOID_ID)
    in_t = torch.where(in_mask, target, torch.full_like(target, VOID_ID))
    logp = F.log_softmax(logits, 1)
    ce_o = F.nll_loss(logp[:h], in_t[:h], ignore_index=VOID_ID, reduction="none").mean()
    ce_a = F.nll_loss(logp[h:], in_t[h:], ignore_index=VOID_ID, reduction="none").mean()
    mo, ma = in_mask.clone(), in_mask.clone()
    mo[h:] = False
    ma[:h] = False
    fo, fa, fd = score[mo], score[ma], score[ood_mask]
    n = min(int(target.numel() * params.get("sample_ratio", 1)), fd.shape[0], fo.shape[0], fa.shape[0])
    fo, fa, fd = fo[perms[0][:n]], fa[perms[1][:n]], fd[perms[2][:n]]
    t_o, t_a = fo + m[0] - fd, fa + m[1] - fd
    t_i = (score[h:] - score[:h] - m[2])[mo[:h] & ma[h:]]
    loss = w0 * ce_o + w1 * ce_a + wc * (F.relu(t_o).mean() + F.relu(t_a).mean() + F.relu(t_i).mean())
    return loss, torch.cat((t_o.detach(), t_a.detach(), t_i.detach()))


def train(dn, class_logits, mask_logits, weight, bias, image_size, size, target, params, seeds, lr, weight_decay, dtype):
    """len(seeds) stage-1 steps on class_embed2 = (weight, bias) from the frozen decoder_norm output dn [B,Q,256], the frozen
    pred_logits and low-resolution pred_masks, all at `dtype`; seeds[i] seeds the pairing of step i. -> dict of float64 host
    tensors: losses [steps], weight, bias after the last step, and of every step the class maps of the ood head (for the -max_c
    gap check), the scores and the hinge arguments."""
    t = lambda a: a.detach().cpu().to(dtype)
    dn, cls, x = t(dn), t(class_logits), t(mask_logits)
    w, b = t(weight).clone().requires_grad_(True), t(bias).clone().requires_grad_(True)
    opt = torch.optim.Adam([w, b], lr=lr, weight_decay=weight_decay)
    logit = sem_seg(cls, x, image_size, size)
    out = dict(losses=[], fulls=[], hinges=[], scores=[])
    for seed in seeds:
        opt.zero_grad()
        cls_ood = dn @ w.t() + b
        full = class_maps(cls_ood, x, image_size, size)
        score = 1 - first_max(full)
        torch.manual_seed(seed)
        loss, hinges = rel_contrastive_loss(logit, score, target, params, draw_perms(target))
        loss.backward()
        opt.step()
        out["losses"].append(loss.detach().double())
        out["fulls"].append(full.detach().double())
        out["scores"].append(score.detach().double())
        out["hinges"].append(hinges.double())
    out["losses"] = torch.stack(out["losses"])
    out["weight"], out["bias"], out["sem_seg"] = w.detach().double(), b.detach().double(), logit.double()
    return out
