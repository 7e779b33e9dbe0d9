"""TEST INFRASTRUCTURE ONLY -- float64 multi-scale deformable attention with the bilinear CELL of every sample as an input.

oracle/msda.py picks the cell of a sample with floor(); at a pixel coordinate that is an integer (a "kink" of the piecewise
bilinear surface) to within rounding, which of the two neighbouring cells an implementation lands in depends on how it rounds
loc * size - 0.5. Here the cell (y0, x0) and the inside flag are arguments and lh = y - y0, lw = x - x0 are taken whatever their
range, so the bilinear formula is the polynomial extension of that cell: out, grad_value and grad_attn are continuous across
a kink (both cells give the same numbers there), grad_loc is the one-sided derivative of the chosen cell.
`cells(loc, shapes, shift)` returns floor(p + shift) and `inside` of the true p; with shift = 0 everything here equals
oracle/msda.py (tests/test_msda_cells_ref_cpu.py).

`lattice_inputs` is the dyadic input recipe of tests/test_gpu_msda_lattice.py: level extents that are powers of two and
coordinates / values / weights / gradients on coarse dyadic grids, so that every product and sum of the op is exact in fp32.
"""
import numpy as np


def level_starts(shapes):
    shp = np.asarray(shapes, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(shp.prod(1))[:-1]]).astype(np.int64)


def pixel_coords(loc, shapes):
    """loc [N,Lq,M,L,P,2] (x, y) in [0, 1] units -> pixel coordinates p = loc * (W, H) - 0.5 in float64 (.cuh:290-291)."""
    shp = np.asarray(shapes, dtype=np.int64)
    return np.asarray(loc, dtype=np.float64) * shp[None, None, None, :, None, ::-1].astype(np.float64) - 0.5


def cells(loc, shapes, shift=0.0):
    """-> (y0, x0, inside), each [N,Lq,M,L,P]: the cell floor(p + shift) and the inside test of .cuh:293 on the true p.
    Samples that fail the test (NaN and infinite coordinates among them) get cell (0, 0); they contribute nothing."""
    shp = np.asarray(shapes, dtype=np.int64)
    p = pixel_coords(loc, shapes)
    x, y = p[..., 0], p[..., 1]
    H = shp[None, None, None, :, None, 0].astype(np.float64)
    W = shp[None, None, None, :, None, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (y > -1) & (x > -1) & (y < H) & (x < W)
    y0 = np.floor(np.where(inside, y, 0.0) + shift).astype(np.int64)
    x0 = np.floor(np.where(inside, x, 0.0) + shift).astype(np.int64)
    return y0, x0, inside


def _level(value, shapes, starts, loc, y0, x0, inside, l):
    """Corner values [4][N,Lq,M,P,D], their flags and flat positions, and lh / lw [N,Lq,M,P] of level l."""
    N, S, M, D = value.shape
    H, W = int(shapes[l][0]), int(shapes[l][1])
    ins = inside[:, :, :, l]
    x = np.where(ins, loc[:, :, :, l, :, 0] * W - 0.5, 0.0)
    y = np.where(ins, loc[:, :, :, l, :, 1] * H - 0.5, 0.0)
    yy0, xx0 = y0[:, :, :, l], x0[:, :, :, l]
    lh = np.where(ins, y - yy0, 0.0)
    lw = np.where(ins, x - xx0, 0.0)
    vl = value[:, int(starts[l]):int(starts[l]) + H * W]
    n_idx = np.arange(N)[:, None, None, None]
    m_idx = np.arange(M)[None, None, :, None]
    vs, oks, poss = [], [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = yy0 + dy, xx0 + dx
        ok = ins & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        pos = np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)
        vs.append(np.where(ok[..., None], vl[n_idx, pos, m_idx], 0.0))
        oks.append(ok)
        poss.append(pos)
    return H, W, ins, lh, lw, vs, oks, poss


def forward(value, shapes, starts, loc, attn, y0, x0, inside):
    """value [N,S,M,D], loc [N,Lq,M,L,P,2], attn / y0 / x0 / inside [N,Lq,M,L,P] -> [N,Lq,M*D], float64."""
    value, loc, attn = (np.asarray(a, dtype=np.float64) for a in (value, loc, attn))
    N, S, M, D = value.shape
    Lq, L = loc.shape[1], loc.shape[3]
    out = np.zeros((N, Lq, M, D))
    for l in range(L):
        H, W, ins, lh, lw, (v1, v2, v3, v4), _, _ = _level(value, shapes, starts, loc, y0, x0, inside, l)
        hh, hw = 1 - lh, 1 - lw
        val = (hh * hw)[..., None] * v1 + (hh * lw)[..., None] * v2 + (lh * hw)[..., None] * v3 + (lh * lw)[..., None] * v4
        a = np.where(ins, attn[:, :, :, l], 0.0)
        out += (a[..., None] * val).sum(axis=3)
    return out.reshape(N, Lq, M * D)


def _scatter_rows(dst, idx, src):
    """dst[idx[i]] += src[i] over rows (np.add.at without its per-element cost)."""
    order = np.argsort(idx, kind="stable")
    idx_s = idx[order]
    first = np.flatnonzero(np.concatenate([[True], idx_s[1:] != idx_s[:-1]]))
    dst[idx_s[first]] += np.add.reduceat(src[order], first, axis=0)


def backward(value, shapes, starts, loc, attn, grad_out, y0, x0, inside, want_value=True):
    """-> (grad_value, grad_loc, grad_attn) in float64, shapes of value / loc / attn (grad_value None unless want_value)."""
    value, loc, attn, grad_out = (np.asarray(a, dtype=np.float64) for a in (value, loc, attn, grad_out))
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    g = grad_out.reshape(N, Lq, M, 1, D)
    grad_value = np.zeros((N * S * M, D)) if want_value else None
    grad_loc = np.zeros(loc.shape)
    grad_attn = np.zeros(attn.shape)
    n_idx = np.arange(N)[:, None, None, None]
    m_idx = np.arange(M)[None, None, :, None]
    for l in range(L):
        H, W, ins, lh, lw, vs, oks, poss = _level(value, shapes, starts, loc, y0, x0, inside, l)
        hh, hw = 1 - lh, 1 - lw
        a = np.where(ins, attn[:, :, :, l], 0.0)
        tgv = a[..., None] * g                                                        # top_grad_value, .cuh:125
        v1, v2, v3, v4 = vs
        if want_value:
            for w, ok, pos in zip((hh * hw, hh * lw, lh * hw, lh * lw), oks, poss):
                rows = ((n_idx * S + int(starts[l]) + pos) * M + m_idx)[ok]
                _scatter_rows(grad_value, rows, (w[..., None] * tgv)[ok])
        val = (hh * hw)[..., None] * v1 + (hh * lw)[..., None] * v2 + (lh * hw)[..., None] * v3 + (lh * lw)[..., None] * v4
        gw = -hh[..., None] * v1 + hh[..., None] * v2 - lh[..., None] * v3 + lh[..., None] * v4
        gh = -hw[..., None] * v1 - lw[..., None] * v2 + hw[..., None] * v3 + lw[..., None] * v4
        grad_attn[:, :, :, l] = np.where(ins, (g * val).sum(-1), 0.0)                  # .cuh:161
        grad_loc[:, :, :, l, :, 0] = np.where(ins, W * (gw * tgv).sum(-1), 0.0)        # .cuh:162
        grad_loc[:, :, :, l, :, 1] = np.where(ins, H * (gh * tgv).sum(-1), 0.0)        # .cuh:163
    if want_value:
        grad_value = grad_value.reshape(N, S, M, D)
    return grad_value, grad_loc, grad_attn


def lattice_coords(rng, shapes, N, Lq, M, P):
    """Pixel coordinates p [N,Lq,M,L,P,2] (x, y): integers(-2, E + 2) + one of 0, 0, 0, .25, .5, .75 per level and axis."""
    L = len(shapes)
    p = np.empty((N, Lq, M, L, P, 2))
    for l, (H, W) in enumerate(shapes):
        for ax, E in ((0, int(W)), (1, int(H))):
            assert E & (E - 1) == 0, "level extents must be powers of two"
            p[:, :, :, l, :, ax] = rng.integers(-2, E + 2, (N, Lq, M, P)) + rng.choice([0, 0, 0, .25, .5, .75], (N, Lq, M, P))
    return p


def lattice_inputs(seed, shapes, N, Lq, M, P, D):
    """The dyadic recipe: dict of float64 arrays value [N,S,M,D], loc, attn, grad_out [N,Lq,M*D], p (pixel coordinates), plus
    shapes / starts (int64). Every array converts to float32 without loss (asserted for loc)."""
    rng = np.random.default_rng(seed)
    shp = np.asarray(shapes, dtype=np.int64)
    S, L = int(shp.prod(1).sum()), len(shapes)
    p = lattice_coords(rng, shapes, N, Lq, M, P)
    loc = (p + 0.5) / shp[None, None, None, :, None, ::-1].astype(np.float64)
    assert np.array_equal(loc.astype(np.float32).astype(np.float64), loc)
    value = rng.integers(-8, 9, (N, S, M, D)) / 8.0
    attn = rng.choice([0, 1 / 16, 1 / 8, 1 / 4], (N, Lq, M, L, P))
    grad_out = rng.integers(-4, 5, (N, Lq, M * D)) / 4.0
    return dict(value=value, loc=loc, attn=attn, grad_out=grad_out, p=p, shapes=shp, starts=level_starts(shp))
