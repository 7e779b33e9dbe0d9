"""Float64 restatement of the Winograd F(m x m, 3 x 3) transforms of csrc/winograd.hip, m = 2, 4, 6, independent of the kernels'
own constants: the F(4x4) and F(6x6) matrices come from the exact rational construction in tools/wino_matrices.py, the F(2x2)
ones are the textbook matrices written out, and the tile geometry is restated from the layout documented in include/mss_hip.h:

    Hs = ceil(H / d), tH = ceil(Hs / m) (the same for W), P = m + 2, T = N * d * d * tH * tW
    tile index t = (((n * d + a) * d + b) * tH + ty) * tW + tx
    element (i, j) of the input tile of sub-grid (a, b) is image pixel ((m * ty + i - 1) * d + a, (m * tx + j - 1) * d + b),
    element (u, v) of its output tile is pixel ((m * ty + u) * d + a, (m * tx + v) * d + b); zero / not written outside the image
    X' [P*P][T][C] and Y' [P*P][T][K] at position xi * P + nu, U [P*P][Kpad][Cp]

Activations are NHWC tensors [N][H][W][C] (what the kernels read), weights [K][C][3][3]. Every transform is a sandwich L X R with
constant L and R; its magnitude companion (`*_mag`) is the same expression on |L|, |X|, |R|, which is what a running-error bound
of the fp32 evaluation is stated in. Everything runs in torch on the device of its input, in `dtype` (float64 unless a chain asks
for float32)."""
import importlib.util
import os

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_wino_matrices", os.path.join(_ROOT, "tools", "wino_matrices.py"))
wino_matrices = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wino_matrices)

U32 = 2.0 ** -24            # unit roundoff of float32

# F(2x2, 3x3), Lavin & Gray 2015
_AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]
_G2 = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
_BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]


def rational_matrices(tile):
    """(At, G, Bt) as exact Fractions for tile 4 or 6: what the literal check prints with wino_matrices.c_init."""
    return wino_matrices.matrices(wino_matrices.POINTS, 4) if tile == 4 else wino_matrices.matrices(wino_matrices.POINTS6, 6)


def mats(tile, dtype=torch.float64, device="cpu"):
    """At [m][P], G [P][3], Bt [P][P]; below float64 they are rounded once from the exact values, as the kernels' literals are."""
    assert tile in (2, 4, 6)
    rows = (_AT2, _G2, _BT2) if tile == 2 else [[[float(v) for v in r] for r in mat] for mat in rational_matrices(tile)]
    return tuple(torch.tensor(mat, dtype=torch.float64, device=device).to(dtype) for mat in rows)


def geom(N, H, W, dil, tile):
    Hs, Ws = -(-H // dil), -(-W // dil)
    tH, tW = -(-Hs // tile), -(-Ws // tile)
    return dict(Hs=Hs, Ws=Ws, tH=tH, tW=tW, T=N * dil * dil * tH * tW)


def _tile_pixels(N, H, W, dil, tile, halo, device):
    """n [T], iy [T][E], ix [T][E], oky, okx (bool [T][E]) of the E = tile + 2 * halo rows / columns of every tile, in tile order."""
    g = geom(N, H, W, dil, tile)
    r = [torch.arange(k, device=device) for k in (N, dil, dil, g["tH"], g["tW"])]
    n, a, b, ty, tx = (v.reshape(-1) for v in torch.meshgrid(*r, indexing="ij"))          # tx fastest: the tile index order
    e = torch.arange(tile + 2 * halo, device=device)
    sy, sx = tile * ty[:, None] + e[None] - halo, tile * tx[:, None] + e[None] - halo     # sub-grid coordinates
    iy, ix = sy * dil + a[:, None], sx * dil + b[:, None]
    return n, iy, ix, (sy >= 0) & (iy < H), (sx >= 0) & (ix < W)


def _gather_tiles(x, dil, tile, halo):
    """x [N][H][W][C] -> [T][E][E][C], zero outside the image."""
    N, H, W, _ = x.shape
    n, iy, ix, oky, okx = _tile_pixels(N, H, W, dil, tile, halo, x.device)
    d = x[n[:, None, None], iy.clamp(0, H - 1)[:, :, None], ix.clamp(0, W - 1)[:, None, :]]
    return torch.where((oky[:, :, None] & okx[:, None, :])[..., None], d, torch.zeros((), dtype=x.dtype, device=x.device))


def _prologue(x, scale, shift, relu, dtype):
    v = x.to(dtype)
    if scale is not None:
        v = v * scale.to(dtype) + shift.to(dtype)
    return torch.relu(v) if relu else v


def _input(x, dil, tile, mag, dtype):
    Bt = mats(tile, dtype, x.device)[2]
    d = _gather_tiles(x, dil, tile, 1)                                                    # [T][P][P][C]
    if mag:
        Bt, d = Bt.abs(), d.abs()
    P = tile + 2
    return torch.einsum("ik,tklc,jl->ijtc", Bt, d, Bt).reshape(P * P, d.shape[0], d.shape[3])


def input_transform(x, dil, tile, scale=None, shift=None, relu=False, dtype=torch.float64):
    """X' [P*P][T][C] = B^T d B per tile of relu?(x * scale + shift); the padding is zero AFTER the prologue."""
    return _input(_prologue(x, scale, shift, relu, dtype), dil, tile, False, dtype)


def input_transform_mag(x, dil, tile, scale=None, shift=None, relu=False):
    return _input(_prologue(x, scale, shift, relu, torch.float64), dil, tile, True, torch.float64)


def input_prologue_error(x, dil, tile, scale, shift):
    """|B^T| E |B| with E = 2 * 2^-24 * (|x * scale| + |shift|): what the fp32 prologue (one multiply and one add, or one fused
    multiply-add; ReLU is 1-Lipschitz) adds to the transform's error."""
    e = 2.0 * U32 * ((x.double() * scale.double()).abs() + shift.double().abs())
    return _input(e, dil, tile, True, torch.float64)


def _pack(w, tile, Kpad, Cp, mag, dtype):
    G = mats(tile, dtype, w.device)[1]
    K, C = w.shape[0], w.shape[1]
    g = w.to(dtype)
    if mag:
        G, g = G.abs(), g.abs()
    P = tile + 2
    u = torch.zeros((P * P, Kpad, Cp), dtype=dtype, device=w.device)
    u[:, :K, :C] = torch.einsum("ir,kcrs,js->ijkc", G, g, G).reshape(P * P, K, C)
    return u


def pack_weights(w, tile, Kpad, Cp, dtype=torch.float64):
    """U [P*P][Kpad][Cp] = G g G^T per (k, c), zero in the padding rows and columns."""
    return _pack(w, tile, Kpad, Cp, False, dtype)


def pack_weights_mag(w, tile, Kpad, Cp):
    return _pack(w, tile, Kpad, Cp, True, torch.float64)


def _output(yt, N, H, W, dil, tile, mag, dtype):
    At = mats(tile, dtype, yt.device)[0]
    P = tile + 2
    T, K = yt.shape[1], yt.shape[2]
    assert yt.shape[0] == P * P and T == geom(N, H, W, dil, tile)["T"]
    m = yt.to(dtype).reshape(P, P, T, K)
    if mag:
        At, m = At.abs(), m.abs()
    tiles = torch.einsum("vj,ujtk->tuvk", At, torch.einsum("ui,ijtk->ujtk", At, m))        # [T][m][m][K]
    n, oy, ox, oky, okx = _tile_pixels(N, H, W, dil, tile, 0, yt.device)
    ok = oky[:, :, None] & okx[:, None, :]
    y = torch.full((N, H, W, K), float("nan"), dtype=dtype, device=yt.device)
    nn = n[:, None, None].expand_as(ok)
    y[nn[ok], oy[:, :, None].expand_as(ok)[ok], ox[:, None, :].expand_as(ok)[ok]] = tiles[ok]
    return y                                                                              # a pixel no tile owns would stay NaN


def output_transform(yt, N, H, W, dil, tile, res=None, dtype=torch.float64):
    """y [N][H][W][K] = A^T Y' A per tile (+ res)."""
    y = _output(yt, N, H, W, dil, tile, False, dtype)
    return y if res is None else y + res.to(dtype)


def output_transform_mag(yt, N, H, W, dil, tile):
    return _output(yt, N, H, W, dil, tile, True, torch.float64)


def _grad_output(dy, dil, tile, mag, dtype):
    At = mats(tile, dtype, dy.device)[0]
    d = _gather_tiles(dy.to(dtype), dil, tile, 0)                                         # [T][m][m][K]
    if mag:
        At, d = At.abs(), d.abs()
    P = tile + 2
    return torch.einsum("ui,tuvk,vj->ijtk", At, d, At).reshape(P * P, d.shape[0], d.shape[3])


def grad_output_transform(dy, dil, tile, dtype=torch.float64):
    """dY' [P*P][T][K] = A dY A^T per tile, dY zero outside the image."""
    return _grad_output(dy, dil, tile, False, dtype)


def grad_output_transform_mag(dy, dil, tile):
    return _grad_output(dy, dil, tile, True, torch.float64)


def _weight_grad(du, K, C, tile, mag, dtype):
    G = mats(tile, dtype, du.device)[1]
    P = tile + 2
    m = du.reshape(P, P, du.shape[1], du.shape[2])[:, :, :K, :C].to(dtype)               # the padding is never read
    if mag:
        G, m = G.abs(), m.abs()
    return torch.einsum("ir,ijkc,js->kcrs", G, m, G)


def weight_grad_transform(du, K, C, tile, dtype=torch.float64):
    """dg [K][C][3][3] = G^T dU G per (k, c) of dU [P*P][Kpad][Cp]."""
    return _weight_grad(du, K, C, tile, False, dtype)


def weight_grad_transform_mag(du, K, C, tile):
    return _weight_grad(du, K, C, tile, True, torch.float64)


def transform_bound(mag, n):
    """Running-error bound of a two-pass transform whose dot products have at most n terms and whose coefficients are rounded to
    fp32: one rounding per coefficient, per product and per addition in each pass, (2n + 4) * 2^-24 * |L| |X| |R| to first order."""
    return (2 * n + 4) * U32 * mag


def conv_chain(x, w, dil, tile, dtype, scale=None, shift=None, relu=False, res=None):
    """3x3 / stride 1 / padding = dilation convolution of x [N][C][H][W] with w [K][C][3][3] through the three Winograd steps, every
    operation in `dtype`: input transform (of relu?(x * scale + shift)), per-position product over C, output transform (+ res
    [N][K][H][W]). Returns [N][K][H][W]."""
    N, C, H, W = x.shape
    K = w.shape[0]
    xt = input_transform(x.permute(0, 2, 3, 1).to(dtype), dil, tile, scale, shift, relu, dtype)      # [PP][T][C]
    u = pack_weights(w.to(dtype), tile, K, C, dtype)                                                  # [PP][K][C]
    yt = torch.bmm(xt, u.transpose(1, 2))                                                             # [PP][T][K]
    r = None if res is None else res.permute(0, 2, 3, 1)
    return output_transform(yt, N, H, W, dil, tile, r, dtype).permute(0, 3, 1, 2)


def wgrad_chain(x, dy, dil, tile, dtype, scale=None, shift=None, relu=False):
    """Weight gradient [K][C][3][3] of the same convolution for the output gradient dy [N][K][H][W], in the Winograd domain:
    dU[p] = dY'[p]^T X'[p] summed over the tiles, then G^T dU G."""
    K, C = dy.shape[1], x.shape[1]
    xt = input_transform(x.permute(0, 2, 3, 1).to(dtype), dil, tile, scale, shift, relu, dtype)      # [PP][T][C]
    dyt = grad_output_transform(dy.permute(0, 2, 3, 1).to(dtype), dil, tile, dtype)                   # [PP][T][K]
    du = torch.bmm(dyt.transpose(1, 2), xt)                                                           # [PP][K][C]
    return weight_grad_transform(du, K, C, tile, dtype)
