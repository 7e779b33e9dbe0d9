"""SetCriterion.loss_ood, branches "margin" and "bce" (lib/network/mask2former/modeling/criterion.py:128-161), on the kernels of
libmss_ood.so (csrc/m2f_ood_loss.hip, include/mss_ood_hip.h) between the class mix of csrc/m2f_mix.hip and its backward.

    M = einsum("bqc,bqhw->bchw", softmax(class_logits, -1)[..., :-1], sigmoid(mask_logits))      kernels.m2f_class_mix
    t = -max_c M                                         at the low resolution                     ood_negmax
    s = interpolate(t, (H, W), bilinear, align_corners=True)                                       ood_pixel_loss
    margin: 0.5 (mean_{ood == 0} s^2         + [n_ood > 0] mean_{ood == 1} max(margin - s, 0)^2)
    bce:    0.5 (mean_{ood == 0} softplus(s) + [n_ood > 0] mean_{ood == 1} softplus(-s))

The two sets are counted over the whole batch; a mask byte other than 0 and 1 belongs to neither. No device-to-host copy, no float
atomics, no integer scratch (the pixel counts are doubles in the stats buffer, the arg-max is recomputed in the backward): two runs
give the same bits. Where classes tie for the maximum, the lowest class index takes the gradient. There is no CPU path.
"""
import math

import torch

from . import _lib_ood
from . import kernels as K
from ._lib import ptr

KINDS = _lib_ood.KINDS


def _kind(name, kind, margin):
    """-> (the kind's number, the margin as a float: 0.0 for "bce", which reads none)"""
    if kind not in KINDS:
        raise ValueError(f"{name}: kind {kind!r} is not one of {sorted(KINDS)}")
    if kind == "bce":
        return KINDS[kind], 0.0
    if margin is None or not math.isfinite(float(margin)):
        raise ValueError(f"{name}: kind 'margin' needs a finite margin, not {margin!r}")
    return KINDS[kind], float(margin)


def ood_mask_bytes(ood_mask):
    """[B,H,W] -> one byte per pixel, 1 = OOD, 0 = in-distribution, 255 = neither. A uint8 or bool tensor is used as it is (a bool
    is reinterpreted, not copied); any other dtype is mapped through == 1 / == 0, as criterion.py:131-132."""
    if ood_mask.dtype == torch.bool:
        return ood_mask.contiguous().view(torch.uint8)
    if ood_mask.dtype == torch.uint8:
        return ood_mask.contiguous()
    is_ood, is_id = ood_mask == 1, ood_mask == 0
    return (is_ood.to(torch.uint8) + (~(is_ood | is_id)).to(torch.uint8) * 255).contiguous()


def _need_mask(name, ood, B, device):
    if not ood.is_cuda or ood.dtype != torch.uint8 or ood.dim() != 3 or ood.shape[0] != B or ood.device != device:
        raise ValueError(f"{name}: ood_mask must be a uint8 CUDA tensor [B={B},H,W] on {device} (see ood_mask_bytes), got "
                         f"{ood.dtype} {tuple(ood.shape)} on {ood.device}")
    if ood.shape[1] < 1 or ood.shape[2] < 1:
        raise ValueError(f"{name}: an empty ood_mask {tuple(ood.shape)}")


def ood_negmax(mix):
    """-max over the classes of the mix [B,C,h,w] -> t [B,h,w] (criterion.py:141 / :152)."""
    name = "ood_negmax"
    K._need_f32_cuda(name, mix)
    if mix.dim() != 4 or min(mix.shape) < 1:
        raise ValueError(f"{name}: mix {tuple(mix.shape)} is not [B,C,h,w]")
    mix = mix.contiguous()
    B, C, h, w = mix.shape
    t = torch.empty((B, h, w), device=mix.device, dtype=torch.float32)
    _lib_ood.call("mss_ood_negmax_f32", ptr(mix), B, C, h, w, ptr(t))
    return t


def ood_pixel_loss(t, ood_mask, kind="margin", margin=1.0, want_score=False):
    """The loss of one step from the low-resolution score t [B,h,w] and ood_mask uint8 [B,H,W] (criterion.py:142-149 / :153-161).
    -> (loss 0-d float32, stats float64 [4] = (S_id, S_ood, n_id, n_ood): the sums of the per-pixel terms and the pixel counts,
    which ood_pixel_loss_backward reads, score [B,H,W] = the interpolated s or None). The per-workgroup partial sums are doubles
    added in index order. n_id == 0 gives NaN, as the reference's mean over an empty tensor."""
    name = "ood_pixel_loss"
    k, m = _kind(name, kind, margin)
    K._need_f32_cuda(name, t)
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{name}: t {tuple(t.shape)} is not [B,h,w]")
    t = t.contiguous()
    B, h, w = t.shape
    _need_mask(name, ood_mask, B, t.device)
    ood = ood_mask.contiguous()
    H, W = ood.shape[1:]
    rows = _lib_ood.value("mss_ood_loss_partials", B * H * W)
    if rows < 1:
        raise ValueError(f"{name}: {B} x {H} x {W} pixels exceed {_lib_ood.MSS_OOD_MAX_PIXELS}")
    partial = torch.empty((rows, 4), device=t.device, dtype=torch.float64)
    stats = torch.empty((4,), device=t.device, dtype=torch.float64)
    loss = torch.empty((), device=t.device, dtype=torch.float32)
    score = torch.empty((B, H, W), device=t.device, dtype=torch.float32) if want_score else None
    _lib_ood.call("mss_ood_pixel_loss_f32", ptr(t), ptr(ood), B, h, w, H, W, k, m, ptr(partial), ptr(stats), ptr(loss), ptr(score))
    return loss, stats, score


def ood_pixel_loss_backward(mix, t, ood_mask, stats, gloss, kind="margin", margin=1.0):
    """d loss / d mix of ood_pixel_loss(ood_negmax(mix), ...) -> dmix [B,C,h,w], written whole: a low-resolution pixel sums, rows then
    columns ascending, wy wx g over the output pixels whose taps contain it, g = gloss 0.5 l'(s) / n_set with s recomputed; minus
    that sum goes to the pixel's arg-max channel (recomputed from mix; among equal values the lowest class index), 0 to the others.
    gloss: the upstream gradient of the loss, a float32 device scalar; stats: as ood_pixel_loss left it."""
    name = "ood_pixel_loss_backward"
    k, m = _kind(name, kind, margin)
    K._need_f32_cuda(name, mix, t, gloss)
    if mix.dim() != 4 or tuple(t.shape) != (mix.shape[0],) + tuple(mix.shape[2:]) or min(mix.shape) < 1:
        raise ValueError(f"{name}: mix {tuple(mix.shape)} / t {tuple(t.shape)}")
    if not stats.is_cuda or stats.dtype != torch.float64 or stats.numel() != 4 or gloss.numel() != 1:
        raise ValueError(f"{name}: stats must be 4 float64 CUDA values and gloss one float32")
    mix, t = mix.contiguous(), t.contiguous()
    B, C, h, w = mix.shape
    _need_mask(name, ood_mask, B, mix.device)
    ood = ood_mask.contiguous()
    H, W = ood.shape[1:]
    dmix = torch.empty_like(mix)
    _lib_ood.call("mss_ood_pixel_loss_backward_f32", ptr(mix), ptr(t), ptr(ood), ptr(stats.contiguous()), ptr(gloss.contiguous()), B, C, h, w,
                  H, W, k, m, ptr(dmix))
    return dmix


class _ClassMixOodLoss(torch.autograd.Function):
    """One node for softmax, sigmoid, einsum, -max, interpolate, the two masked means and their sum."""

    @staticmethod
    def forward(ctx, class_logits, mask_logits, ood, kind, margin, pixel_major, Q):
        mix, prob = K.m2f_class_mix(class_logits, mask_logits, pixel_major=pixel_major, Q=Q)
        t = ood_negmax(mix)
        loss, stats, _ = ood_pixel_loss(t, ood, kind, margin)
        ctx.save_for_backward(class_logits, mask_logits, mix, prob, t, ood, stats)
        ctx.cfg = (kind, margin, pixel_major, Q)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        class_logits, mask_logits, mix, prob, t, ood, stats = ctx.saved_tensors
        kind, margin, pixel_major, Q = ctx.cfg
        dmix = ood_pixel_loss_backward(mix, t, ood, stats, g.contiguous().float(), kind, margin)
        dmasks, dcls = K.m2f_class_mix_backward(dmix, prob, class_logits, mask_logits, pixel_major=pixel_major, Q=Q,
                                                want_dmasks=ctx.needs_input_grad[1])
        return dcls, dmasks, None, None, None, None, None


def class_mix_ood_loss(class_logits, mask_logits, ood_mask, kind="margin", margin=1.0, pixel_major=False, Q=None):
    """loss_ood of one prediction step in its "margin" or "bce" branch (criterion.py:130-161) as ONE differentiable op -> 0-d float32.
    class_logits [B,Q,C+1], mask_logits [B,Q,h,w] or, with pixel_major, [B,h,w,ldq]; float32 on the device. ood_mask [B,H,W] on the
    device: uint8 or bool as it is (1 = OOD, 0 = in-distribution, any other byte = neither), other dtypes through == 1 / == 0.
    Gradients reach both logits; where classes tie for the maximum of the mix, the lowest class index takes the gradient."""
    name = "class_mix_ood_loss"
    _kind(name, kind, margin)
    if not ood_mask.is_cuda:
        raise RuntimeError(f"{name} runs on an MI355X only (CUDA tensors); there is no CPU path")
    margin = None if kind == "bce" else float(margin)
    return _ClassMixOodLoss.apply(class_logits.float().contiguous(), mask_logits.float().contiguous(), ood_mask_bytes(ood_mask), kind, margin,
                                  bool(pixel_major), None if Q is None else int(Q))
