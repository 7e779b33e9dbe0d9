"""The forward convolution / GEMM of mss_conv2d_forward_f32, restated in float64 with explicit index arithmetic (one gather and one
matrix product per filter tap), and the three-term bf16 split of the split-bf16 kernels, emulated in float64.

    acc[m][k] = sum over taps (r, s) and channels c of act(x[n, oy * stride + r * dil - pad, ox * stride + s * dil - pad, c]) * w[k][c][r][s]
    y[m][k]   = max(gate or add(acc * out_scale[k] + out_shift[k], res[m][k]), 0 if out_relu)                      (csrc/mss_epilogue.h)
    stats[g]  = (sum, sum of squares) over rows 64 g .. 64 g + 63 (below M) of y AS STORED, per channel

with m = (n, oy, ox), act the optional prologue affine (one for all samples, or one per sample) followed by ReLU, zero outside the
image (padding is NOT activated). On the split route the product of two values is not the true product but the six products the
kernel keeps (include/mss_hip.h, above mss_gemm_split_weights_bf16x3): with a = hi + mid + lo on both sides,
hi hi + hi mid + mid hi + hi lo + lo hi + mid mid. No convolution routine is called. `wrong` computes deliberately wrong variants
(tests/test_fwd_exact_cpu.py: the comparison must notice each of them); the kernels never see those."""
import torch


def out_size(h, r, stride, dil, pad):
    return (h + 2 * pad - dil * (r - 1) - 1) // stride + 1


def granule(t):
    """The largest power of two, 1 at most, that divides every element of t (float64)."""
    t = t.double().flatten()
    for e in range(0, 64):
        s = t * 2.0 ** e
        if bool((s == s.round()).all()):
            return 2.0 ** -e
    raise AssertionError("not on a binary lattice")


def lattice_matmul(p, q):
    """p [rows][C] @ q [K][C]^T in float64 for operands on binary lattices, as a product of INTEGER matrices times the two granules:
    however a device library evaluates a float64 product (order, fused or not), small integers come out exactly."""
    gp, gq = granule(p), granule(q)
    return ((p / gp) @ (q / gq).t()) * (gp * gq)


def bf16_rne(v):
    """Round float64 values to bf16 (8 significant bits, round to nearest even), by arithmetic: torch.round rounds halves to even."""
    m, e = torch.frexp(v)                                   # v = m * 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def split3(v):
    """The split of mss_bf16x3::split_pair in float64: hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid). CPU tensors only."""
    assert v.device.type == "cpu"
    v = v.double()
    hi = bf16_rne(v)
    mid = bf16_rne(v - hi)
    lo = bf16_rne(v - hi - mid)
    return hi, mid, lo


def act(x, scale=None, shift=None, relu=False, affine_of=None):
    """The prologue on x [N][...][C] in float64. scale / shift: [C] or [N][C] (sample n uses row n, or row affine_of[n])."""
    a = x.double()
    if scale is not None:
        N, C = a.shape[0], a.shape[-1]
        sc, sh = scale.double(), shift.double()
        if sc.dim() == 1:
            sc, sh = sc.expand(N, C), sh.expand(N, C)
        rows = list(range(N)) if affine_of is None else list(affine_of)
        view = (N,) + (1,) * (a.dim() - 2) + (C,)
        a = a * sc[rows].view(view) + sh[rows].view(view)
    return torch.relu(a) if relu else a


def conv(a, w, stride=1, dil=1, pad=0, wrong=None, only=None):
    """a [N][H][W][C] (activated, float64), w [K][C][R][R] float64 -> [N][OH][OW][K] float64.
    wrong: ("tap", t) tap t contributes nothing; ("chunk", c0) input channels c0 .. c0 + 15 contribute nothing;
           ("row", m) output pixel m gets no product (its accumulator stays 0).
    only: the same three forms, but the named piece ALONE contributes: conv(wrong=p) + conv(only=p) == conv() term by term."""
    N, H, W, C = a.shape
    K, _, R, S = w.shape
    OH, OW = out_size(H, R, stride, dil, pad), out_size(W, S, stride, dil, pad)
    kind = wrong[0] if wrong else None
    M = N * OH * OW
    m = torch.arange(M)
    n, rem = m // (OH * OW), m % (OH * OW)
    oy, ox = rem // OW, rem % OW
    chan = torch.ones(C, dtype=torch.float64)
    if kind == "chunk":
        chan[wrong[1]:wrong[1] + 16] = 0.0
    if only and only[0] == "chunk":
        chan = torch.zeros(C, dtype=torch.float64)
        chan[only[1]:only[1] + 16] = 1.0
    out = torch.zeros((M, K), dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            if (kind == "tap" and wrong[1] == r * S + s) or (only and only[0] == "tap" and only[1] != r * S + s):
                continue
            iy, ix = oy * stride + r * dil - pad, ox * stride + s * dil - pad
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            if only and only[0] == "row":
                ok &= m == only[1]
            if not bool(ok.any()):
                continue
            rows = a[n[ok], iy[ok], ix[ok]] * chan
            out[ok] += rows @ w[:, :, r, s].t()
    if kind == "row":
        out[wrong[1]] = 0.0
    return out.view(N, OH, OW, K)


def live_taps(H, W, R, stride, dil, pad):
    """The taps that reach a pixel of the image from some output pixel."""
    OH, OW = out_size(H, R, stride, dil, pad), out_size(W, R, stride, dil, pad)
    live = []
    for r in range(R):
        for s in range(R):
            if any(0 <= oy * stride + r * dil - pad < H for oy in range(OH)) and any(0 <= ox * stride + s * dil - pad < W for ox in range(OW)):
                live.append(r * R + s)
    return live


def product(a, w, split, stride=1, dil=1, pad=0, wrong=None, absolute=False, only=None):
    """The accumulator: conv(a, w), or on the split route the six kept products of the two splits. absolute: the sum of the
    magnitudes of the same terms instead (what an exact evaluation has to hold)."""
    def f(p, q):
        return conv(p.abs(), q.abs(), stride, dil, pad) if absolute else conv(p, q, stride, dil, pad, wrong, only)
    if not split:
        return f(a, w.double())
    ah, am, al = split3(a)
    wh, wm, wl = split3(w)
    if absolute:
        return f(ah, wh.abs() + wm.abs() + wl.abs()) + f(am, wh.abs() + wm.abs()) + f(al, wh)
    return f(ah, wh + wm + wl) + f(am, wh + wm) + f(al, wh)


def epilogue(acc, out_scale=None, out_shift=None, res=None, res_mask=False, out_relu=False):
    """acc [..][K] float64 -> y as stored (csrc/mss_epilogue.h)."""
    lin = acc if out_scale is None else acc * out_scale.double() + out_shift.double()
    if res is not None:
        lin = torch.where(res.double() > 0, lin, torch.zeros_like(lin)) if res_mask else lin + res.double()
    return torch.relu(lin) if out_relu else lin


def stats(y):
    """y [M][K] float64 -> [ceil(M / 64)][2][K]: per 64-row group the column sums and sums of squares of the stored values."""
    M, K = y.shape
    groups = -(-M // 64)
    padded = torch.zeros((groups * 64, K), dtype=y.dtype, device=y.device)
    padded[:M] = y
    padded = padded.view(groups, 64, K)
    return torch.stack([padded.sum(1), (padded * padded).sum(1)], dim=1)
