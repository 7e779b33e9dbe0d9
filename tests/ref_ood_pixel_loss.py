"""Test helper: SetCriterion.loss_ood in its "margin" and "bce" branches (criterion.py:128-161) restated in stock torch at a chosen
dtype, differentiable, without boolean indexing (masked sums over the whole map: no host synchronisation, and n_id == 0 leaves the
gradient of the other term alone, as the reference's mean over an empty gather does).

    P = softmax(class_logits, -1)[..., :-1]                          [B,Q,C]
    M = sum_q P[b,q,c] sigmoid(mask_logits[b,q,y,x])                 [B,C,h,w]      the mix, at the low resolution
    t = -max_c M                                                     [B,h,w]        still at the low resolution
    s = interpolate(t, (H, W), bilinear, align_corners=True)         [B,H,W]        the size of ood_mask, no crop
    margin: 0.5 (mean_{ood == 0} s^2         + [n_ood > 0] mean_{ood == 1} max(margin - s, 0)^2)
    bce:    0.5 (mean_{ood == 0} softplus(s) + [n_ood > 0] mean_{ood == 1} softplus(-s)),   softplus(x) = max(x, 0) + log1p(exp(-|x|))

ood_mask: 1 = OOD, 0 = in-distribution, anything else belongs to neither set; the sets are counted over the whole batch. n_id == 0
gives NaN. Where several classes share the maximum, the LOWEST class index is the one that counts (and takes the gradient): the
rule of the HIP kernels, written out here because torch.max leaves it unspecified."""
import torch
import torch.nn.functional as F

KINDS = ("margin", "bce")


def mix(class_logits, mask_logits):
    """-> M [B,C,h,w]"""
    prob = torch.softmax(class_logits, -1)[..., :-1]
    return torch.einsum("bqc,bqhw->bchw", prob, torch.sigmoid(mask_logits))


def first_max(v):
    """max over dim 1 whose gradient goes to the lowest index among equal maxima"""
    eq = v == v.max(1, keepdim=True).values
    first = eq & (eq.cumsum(1) == 1)
    return (v * first).sum(1)


def neg_max(m):
    """M [B,C,h,w] -> t [B,h,w]"""
    return -first_max(m)


def score(t, size):
    """t [B,h,w] -> s [B,H,W]"""
    return F.interpolate(t.unsqueeze(1), size=tuple(size), mode="bilinear", align_corners=True).squeeze(1)


def softplus(x):
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def terms(s, kind, margin):
    """-> (the per-pixel term of an in-distribution pixel, that of an OOD pixel), each [B,H,W]"""
    if kind == "margin":
        return s ** 2, (margin - s).clamp(min=0) ** 2
    if kind == "bce":
        return softplus(s), softplus(-s)
    raise ValueError(kind)


def _masked_mean(term, mask, empty):
    n = mask.sum()
    mean = (term * mask).sum() / n.clamp(min=1)
    return torch.where(n > 0, mean, torch.full_like(mean, empty))


def pixel_loss(s, ood_mask, kind, margin=None):
    """s [B,H,W], ood_mask [B,H,W] of any dtype -> the 0-d loss at the dtype of s"""
    l_id, l_ood = terms(s, kind, margin)
    is_id, is_ood = (ood_mask == 0).to(s.dtype), (ood_mask == 1).to(s.dtype)
    return 0.5 * (_masked_mean(l_id, is_id, float("nan")) + _masked_mean(l_ood, is_ood, 0.0))


def loss_from_mix(m, ood_mask, kind, margin=None):
    return pixel_loss(score(neg_max(m), ood_mask.shape[-2:]), ood_mask, kind, margin)


def class_mix_ood_loss(class_logits, mask_logits, ood_mask, kind, margin=None):
    """One step of SetCriterion.loss_ood, NCHW mask logits."""
    return loss_from_mix(mix(class_logits, mask_logits), ood_mask, kind, margin)


def top_gap(m):
    """M [B,C,h,w] -> the smallest difference between the two largest classes over all low-resolution pixels"""
    if m.shape[1] < 2:
        return float("inf")
    top = m.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())
