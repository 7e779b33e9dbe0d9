"""Test helper: the class mix of SetCriterion.loss_ood (RCL branch) restated in stock torch at a chosen dtype, differentiable.

    P  = softmax(class_logits, -1)[..., :-1]                          [B,Q,C]
    M  = sum_q P[b,q,c] sigmoid(mask_logits[b,q,y,x])                 [B,C,h,w]      the mix, at the low resolution
    L  = bilinear(M[:, :19], size)[:, :, :Ht, :Wt]                    mode "logits"
    s  = -max_c bilinear(M, size)[:, :, :Ht, :Wt]                     mode "neg_max"

bilinear = F.interpolate(mode="bilinear", align_corners=False): the source coordinate of output pixel o is
max(0, (o + 0.5) * in / out - 0.5) with `out` the interpolation size, whatever the crop. Where several classes share the
maximum, the LOWEST class index is the one that counts (and takes the gradient): the rule of the HIP kernels, written out here
because torch.max leaves it unspecified."""
import torch
import torch.nn.functional as F

LOGIT_CHANNELS = 19


def mix(class_logits, mask_logits):
    """-> (M [B,C,h,w], P [B,Q,C])"""
    prob = torch.softmax(class_logits, -1)[..., :-1]
    return torch.einsum("bqc,bqhw->bchw", prob, torch.sigmoid(mask_logits)), prob


def bilinear(m, size, crop):
    return F.interpolate(m, size=tuple(size), mode="bilinear", align_corners=False)[:, :, :crop[0], :crop[1]]


def first_max(v):
    """max over dim 1 whose gradient goes to the lowest index among equal maxima"""
    eq = v == v.max(1, keepdim=True).values
    first = eq & (eq.cumsum(1) == 1)
    return (v * first).sum(1)


def upsample(m, size, crop, mode):
    if mode == "logits":
        return bilinear(m[:, :LOGIT_CHANNELS], size, crop)
    if mode == "neg_max":
        return -first_max(bilinear(m, size, crop))
    raise ValueError(mode)


def class_mix_upsample(class_logits, mask_logits, size, crop, mode):
    return upsample(mix(class_logits, mask_logits)[0], size, crop, mode)


def top_gap(full):
    """[B,C,Ht,Wt] -> the smallest difference between the two largest classes over all pixels"""
    top = full.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def loss_ood(step, size, sem_seg, extra_loss):
    """One step of SetCriterion.loss_ood: step = {pred_logits, pred_masks, pred_logits_ood, pred_masks_ood} (NCHW)."""
    crop = tuple(sem_seg.shape[-2:])
    logits = class_mix_upsample(step["pred_logits"], step["pred_masks"], size, crop, "logits")
    score = class_mix_upsample(step["pred_logits_ood"], step["pred_masks_ood"], size, crop, "neg_max")
    return extra_loss(logits, score, sem_seg.clone().long())
