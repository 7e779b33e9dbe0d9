"""GPU: the stride-2 data-gradient kernel (csrc/conv_dgrad_s2.hip, MssConvArgs.stride == -2) alone, exactly.

Lattice data: dz integers in [-4, 4], weights integers in [-3, 3], prologue scales powers of two, integer shifts and residuals.
Every product and every partial sum is then a multiple of 1/2 far below 2^24 (at most 9 taps x 64 channels x 9 x 3), so the fp32
result is exact whatever the summation order and is compared with torch.equal against F.conv_transpose2d in float64 on the CPU.
The output buffer is pre-filled with NaN, padding columns included: columns [0, K) must all be finite (the tap-less parity classes
are written too) and the columns behind them untouched."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# dx sizes (N, OH, OW): the smallest, one with a single odd row, odd, even (the last odd row / column has an out-of-range source),
# and 2 x 24 x 40 whose parity classes have 480 pixels: they cross 128-pixel tiles and the two images
DX_SIZES = [(1, 1, 1), (1, 2, 2), (1, 2, 3), (1, 9, 13), (1, 8, 12), (2, 24, 40)]
CHANNELS = [(16, 16), (16, 80), (64, 64), (64, 80), (64, 16), (16, 64)]        # (C of dz, K of dx); K = 80 exercises the Kpad padding
VARIANTS = ("plain", "in_scale", "res", "res_mask", "slice")


def _lattice(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _grid(oh, r):
    return (oh + 2 * (r // 2) - r) // 2 + 1


def _reference(dz, w, oh, ow, r, scale=None, shift=None):
    """float64 dx [N, K, OH, OW] of the stride-2 convolution with weight w [C, K, r, r] and padding r // 2 at output gradient dz."""
    z = dz.double()
    if scale is not None:
        z = z * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    pad = r // 2
    base = ((z.shape[2] - 1) * 2 - 2 * pad + r, (z.shape[3] - 1) * 2 - 2 * pad + r)
    return F.conv_transpose2d(z, w.double(), stride=2, padding=pad, output_padding=(oh - base[0], ow - base[1]))


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("size", DX_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ck", CHANNELS, ids=lambda s: f"C{s[0]}K{s[1]}")
def test_exact_against_conv_transpose(r, size, ck):
    from multishiftseg_amd import kernels as K
    n, oh, ow = size
    c, k = ck
    h, wd = _grid(oh, r), _grid(ow, r)
    gen = torch.Generator().manual_seed(1000 * r + 100 * oh + ow + c + k)
    dz = _lattice((n, c, h, wd), -4, 4, gen)
    w = _lattice((c, k, r, r), -3, 3, gen)                        # the forward convolution's weight: dz channels x dx channels
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=gen)]
    shift = _lattice((c,), -1, 1, gen)
    res = _lattice((n, k, oh, ow), -4, 4, gen)
    pw = K.pack_weight(w.cuda(), flip=True)
    assert (pw.K, pw.C, pw.R) == (k, c, r)
    dz_act = K.Act.from_nchw(dz.cuda())
    res_act = K.Act.from_nchw(res.cuda())
    aff = (scale.cuda(), shift.cuda())
    plain = _reference(dz, w, oh, ow, r)
    for variant in VARIANTS:
        ld, c0 = (k + 16, 4) if variant == "slice" else (k, 0)
        buf = torch.full((n, oh, ow, ld), float("nan"), device="cuda")
        out = K.Act(buf, k, c0)
        if variant == "in_scale":
            got, want = K.conv2d_dgrad_s2(dz_act, pw, (oh, ow), in_affine=aff, out=out), _reference(dz, w, oh, ow, r, scale, shift)
        elif variant == "res":
            got, want = K.conv2d_dgrad_s2(dz_act, pw, (oh, ow), res=res_act, out=out), plain + res.double()
        elif variant == "res_mask":
            got, want = K.conv2d_dgrad_s2(dz_act, pw, (oh, ow), res=res_act, res_mask=True, out=out), plain * (res > 0)
        else:
            got, want = K.conv2d_dgrad_s2(dz_act, pw, (oh, ow), out=out), plain
        assert got is out
        full = buf.cpu()
        inside = full[..., c0:c0 + k]
        assert torch.isfinite(inside).all(), f"{variant}: an element of dx was not written"
        outside = torch.cat([full[..., :c0], full[..., c0 + k:]], dim=-1)
        assert torch.isnan(outside).all(), f"{variant}: a column outside [0, K) was written"
        assert torch.equal(inside.permute(0, 3, 1, 2).double(), want), f"{variant}: max diff {(inside.permute(0, 3, 1, 2) - want).abs().max()}"


def test_allocates_its_output_and_ignores_the_split_route():
    """Without `out` the wrapper allocates dx; under set_gemm_route("bf16x3") the product stays on the native kernel (no split planes
    are made for the pack) and the result is the same, exact, one."""
    from multishiftseg_amd import kernels as K
    gen = torch.Generator().manual_seed(3)
    dz, w = _lattice((1, 64, 5, 7), -4, 4, gen), _lattice((64, 256, 3, 3), -3, 3, gen)
    want = _reference(dz, w, 9, 13, 3)
    pw = K.pack_weight(w.cuda(), flip=True)
    a = K.conv2d_dgrad_s2(K.Act.from_nchw(dz.cuda()), pw, (9, 13))
    K.set_gemm_route("bf16x3")
    try:
        b = K.conv2d_dgrad_s2(K.Act.from_nchw(dz.cuda()), pw, (9, 13))
    finally:
        K.set_gemm_route(None)
    assert pw.planes is None
    assert (a.N, a.H, a.W, a.C) == (1, 9, 13, 256)
    assert torch.equal(a.nchw().double().cpu(), want) and torch.equal(b.buf, a.buf)


def _lib_ptr(t):
    from multishiftseg_amd import _lib
    return _lib.ptr(t)


def _args(K, r=3, oh=9, ow=13, c=16, k=16, dil=1, stats=False):
    gen = torch.Generator().manual_seed(0)
    pad = r // 2
    h, wd = _grid(9, r), _grid(13, r)              # the grid of a 9 x 13 dx, whatever `oh` and `ow` claim
    dz = K.Act.from_nchw(_lattice((1, c, h, wd), -4, 4, gen).cuda())
    pw = K.pack_weight(_lattice((c, k, r, r), -3, 3, gen).cuda(), flip=True)
    out = K.Act.empty(1, oh, ow, k, "cuda")
    a = K._conv_args(dz, pw, out, -2, dil, pad, None, False, None, False, None, split=False)
    a.OH, a.OW, a.ldy = oh, ow, out.ld
    keep = [dz, pw, out]
    if stats:
        keep.append(torch.empty((8, 2, k), device="cuda"))
        a.stats = _lib_ptr(keep[-1])
    return a, keep


def test_return_codes_and_route():
    from multishiftseg_amd import _lib, kernels as K

    def rc(**kw):
        a, keep = _args(K, **kw)
        code = _lib.status("mss_conv2d_forward_f32", ctypes.byref(a))
        torch.cuda.synchronize()
        return code

    assert rc() == 0
    assert rc(oh=11) == _lib.MSS_ERR_BAD_ARG                       # a 9 x 13 grid's dz cannot come from an 11-row input
    assert rc(ow=12) == _lib.MSS_ERR_BAD_ARG
    assert rc(dil=2) == _lib.MSS_ERR_UNSUPPORTED
    assert rc(r=5) == _lib.MSS_ERR_UNSUPPORTED
    assert rc(stats=True) == _lib.MSS_ERR_UNSUPPORTED
    a, keep = _args(K)
    assert _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) == 6
