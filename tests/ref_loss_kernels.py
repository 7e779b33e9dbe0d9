"""TEST INFRASTRUCTURE ONLY -- numpy restatements of the kernels of csrc/loss.hip one by one, each evaluated in the dtype it is
handed: float64 is the reference, float32 the same arithmetic at the kernels' precision (its distance from float64 is the floor
the tolerances of tests/test_gpu_loss_kernels.py are built on)."""
import numpy as np


def f2key(v):
    """f2key of csrc/loss.hip: order-preserving uint32 image of float32 bits."""
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def masks(target, C):
    """(in-distribution, OOD, flagged) of int64 labels: in-distribution is a class index below 99, OOD is above 99 and not 255, a
    label below 0 or in [C, 99) is flagged and belongs to neither; 99 and 255 belong to neither and are not flagged."""
    bad = (target < 99) & ((target < 0) | (target >= C))
    return (target < 99) & ~bad, (target > 99) & (target != 255), bad


def pass1(logit, score, target, w0, w1, m2, dtype):
    """rcl_pass1: lse [B,HW], ce_aug [half] (+inf off the in-distribution pixels), kind, the 16 counters and the gradient of
    every pixel at the weight w / half (the kernel writes the augmented half of it only without the selection)."""
    B, C, H, W = logit.shape
    h, HW = B // 2, H * W
    half = h * HW
    x = logit.reshape(B, C, HW).astype(dtype)
    t = target.reshape(B, HW)
    inm, ood, bad = masks(t, C)
    m = x.max(1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(1, dtype=dtype))
    picked = np.take_along_axis(x, np.where(inm, t, 0)[:, None], 1)[:, 0]
    ce = np.where(inm, lse - picked, dtype(0))
    s = score.reshape(B, HW).astype(dtype)
    same = inm[:h] & inm[h:]
    c = np.zeros(16, dtype=np.float64)
    c[0] = ce[:h].sum(dtype=dtype)
    c[1], c[2], c[3] = inm[:h].sum(), inm[h:].sum(), ood.sum()
    c[4] = (np.maximum(s[h:] - s[:h] - dtype(m2), 0) * same).sum(dtype=dtype)
    c[5] = same.sum()
    c[6] = ce[h:].sum(dtype=dtype)
    c[12] = bad.sum()
    g = np.zeros((B, HW), dtype=dtype)
    g[:h], g[h:] = dtype(w0) / dtype(half), dtype(w1) / dtype(half)
    d = softmax_grad(x, lse, t, inm, g * inm)
    return dict(lse=lse, ce_aug=np.where(inm[h:], ce[h:], dtype(np.inf)).reshape(-1), kind=np.where(inm, 1, np.where(ood, 2, 0)).astype(np.uint8),
                counters=c, dlogit=d.reshape(B, C, H, W), ce=ce)


def softmax_grad(x, lse, t, inm, g):
    """g * (softmax - onehot) of x [B,C,HW] with per-pixel weight g [B,HW] (0 outside `inm`, where the result is exact 0)."""
    d = np.exp(x - lse[:, None]) * g[:, None]
    b, p = np.nonzero(inm)
    d[b, t[b, p], p] -= g[b, p]
    return d          # x - lse <= 0, so exp() is finite and a weight of 0 gives exact 0


def pass2_grad(logit, lse32, target, chosen, w1, k, dtype):
    """rcl_pass2's gradient of the augmented half [h,C,HW]: w1 / k * (exp(x - lse) - onehot) on `chosen` [h,HW], 0 elsewhere; lse32
    is the float32 buffer the kernel reads."""
    B, C, H, W = logit.shape
    h, HW = B // 2, H * W
    x = logit.reshape(B, C, HW)[h:].astype(dtype)
    g = np.where(chosen, dtype(w1) / dtype(k if k else 1), dtype(0)).astype(dtype)
    return softmax_grad(x, lse32.reshape(B, HW)[h:].astype(dtype), target.reshape(B, HW)[h:], chosen, g)


def pairs(score, idx_a, perm_a, idx_o, perm_o, n, margin, grad_w, dtype):
    """rcl_pairs: (hinge sum, dscore, the open-hinge mask) over the n pairs (idx_a[perm_a[i]], idx_o[perm_o[i]])."""
    s = score.astype(dtype)
    pa, po = idx_a[perm_a[:n]], idx_o[perm_o[:n]]
    v = s[pa] + dtype(margin) - s[po]
    d = np.zeros(s.shape, dtype=dtype)
    if n:
        coef = dtype(grad_w) / dtype(n)
        np.add.at(d, pa[v > 0], coef)
        np.add.at(d, po[v > 0], -coef)
    return float(v[v > 0].sum(dtype=dtype)), d, v > 0


def ulp32(v):
    """One float32 ulp at |v|."""
    return float(np.spacing(np.abs(np.float32(v))))
