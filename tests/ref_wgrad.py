"""The weight gradient of a convolution, restated in float64 with explicit index arithmetic (a gather per filter tap, then one
matrix product): what mss_conv2d_wgrad_f32 computes, in its packed layout.

    dW[tap][k][c] = sum_m dy[m][k] * act(x[n, oy * stride + r * dil - pad, ox * stride + s * dil - pad, c])

with m = (n, oy, ox) over the output pixels, tap = r * S + s, act the optional prologue affine (one for all samples, or one per
sample) and / or ReLU, and zero outside the image. No convolution routine is called. The `wrong` argument computes deliberately
wrong variants (tests/test_wgrad_exact_cpu.py: the comparison must notice each of them); the kernels never see those."""
import torch


def act(x, scale=None, shift=None, relu=False, affine_of=None):
    """The prologue on x [N][H][W][C] in float64. scale / shift: [C] (one affine) or [N][C] (sample n uses row n; affine_of: a list
    that says which row each sample uses instead)."""
    a = x.double()
    if scale is not None or shift is not None:
        N, C = a.shape[0], a.shape[3]
        sc = torch.ones(C, dtype=torch.float64) if scale is None else scale.double()
        sh = torch.zeros(C, dtype=torch.float64) if shift is None else shift.double()
        if sc.dim() == 1:
            sc, sh = sc.expand(N, C), sh.expand(N, C)
        rows = list(range(N)) if affine_of is None else list(affine_of)
        a = a * sc[rows][:, None, None, :C] + sh[rows][:, None, None, :C]
    return torch.relu(a) if relu else a


def out_size(h, r, stride, dil, pad):
    return (h + 2 * pad - dil * (r - 1) - 1) // stride + 1


def wgrad(x, dy, R, S, stride=1, dil=1, pad=0, scale=None, shift=None, relu=False, Kpad=None, Cp=None, wrong=None, absolute=False):
    """x [N][H][W][C], dy [N][OH][OW][K] (any float dtype, CPU) -> [R*S][Kpad][Cp] float64, exact zeros in rows K.. and columns C...
    absolute: sum |dy| * |act(x)| instead (the magnitude an exact fp32 evaluation has to hold).
    wrong (all leave the shapes alone):
      ("drop", m)          output pixel m contributes nothing
      ("tap", t, dy, dx)   tap t reads its pixels dy rows / dx columns further
      ("swap",)            stride and dilation change places in the input coordinates
      ("affine", rows)     sample n takes the per-sample affine of row rows[n]"""
    N, H, W, C = x.shape
    _, OH, OW, K = dy.shape
    assert dy.shape[0] == N and OH == out_size(H, R, stride, dil, pad) and OW == out_size(W, S, stride, dil, pad)
    Kpad, Cp = Kpad or (K + 3) // 4 * 4, Cp or (C + 3) // 4 * 4
    kind = wrong[0] if wrong else None
    a = act(x, scale, shift, relu, affine_of=wrong[1] if kind == "affine" else None)
    M = N * OH * OW
    g = dy.double().reshape(M, K).clone()
    if kind == "drop":
        g[wrong[1]] = 0.0
    if absolute:
        a, g = a.abs(), g.abs()
    m = torch.arange(M)
    n, rem = m // (OH * OW), m % (OH * OW)
    oy, ox = rem // OW, rem % OW
    if kind == "swap":
        stride, dil = dil, stride
    out = torch.zeros((R * S, Kpad, Cp), dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            tap = r * S + s
            iy, ix = oy * stride + r * dil - pad, ox * stride + s * dil - pad
            if kind == "tap" and wrong[1] == tap:
                iy, ix = iy + wrong[2], ix + wrong[3]
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            rows = torch.zeros((M, C), dtype=torch.float64)
            rows[ok] = a[n[ok], iy[ok], ix[ok]]
            out[tap, :K, :C] = g.t() @ rows
    return out


def unpack(dwp, K, C, R, S):
    """[R*S][Kpad][Cp] -> [K][C][R][S], nn.Conv2d.weight's layout."""
    return dwp[:, :K, :C].reshape(R, S, K, C).permute(2, 3, 0, 1).contiguous()
