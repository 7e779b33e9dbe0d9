"""The two-source ASPP input transform (mss_wino_input_transform_aspp3_src2_f32) alone: X' of the never-stored map
w = [relu(x0 * scale0 + shift0) ; relu(x1 * scale1 + shift1)] for the three dilations d, 2d, 3d, every element equal to what
mss_affine_relu_nhwc_f32 into one buffer followed by mss_wino_input_transform_aspp3_f32 writes; its column sums / global average in
the full and in the sums-only mode; and what it refuses."""
import ctypes

import pytest
import torch

from multishiftseg_amd import _lib
from multishiftseg_amd._lib import call, ptr, status

pytestmark = pytest.mark.gpu

CANARY = 64


def _off(t, floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def _with_canary(n):
    return torch.full((n + CANARY,), float("nan"), device="cuda", dtype=torch.float32)


def _src2(a0, ld0, C0, sc0, sh0, a1, ld1, C1, sc1, sh1, N, H, W, d, tiles, xts, sums, gap):
    return status("mss_wino_input_transform_aspp3_src2_f32", a0, ld0, C0, ptr(sc0), ptr(sh0), 0, a1, ld1, C1, ptr(sc1), ptr(sh1), C1,
                  N, H, W, d, (ctypes.c_int * 3)(*tiles), ptr(xts[0]), ptr(xts[1]), ptr(xts[2]), ptr(sums), ptr(gap))


# (n, H, W, C0, C1, d, tiles): 1 x 2-pixel sub-grids; a channel chunk that straddles the two sources (36 is no multiple of the 32- or
# 64-channel chunks); odd sizes on F(6x6) everywhere; more channel chunks in source 0 than in source 1
CASES = [(2, 12, 16, 32, 32, 12, (4, 4, 4)), (2, 45, 75, 36, 32, 6, (6, 4, 6)), (1, 37, 41, 64, 64, 6, (6, 6, 6)),
         (2, 24, 36, 128, 64, 2, (4, 6, 4))]


@pytest.mark.parametrize("n,H,W,C0,C1,d,tiles", CASES)
def test_two_source_transform_equals_materialise_then_transform(n, H, W, C0, C1, d, tiles):
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W + C0)
    C = C0 + C1
    # the sources are channel slices of wider buffers (ld > C), mixed sign
    ld0, ld1, o0, o1 = C0 + 8, C1 + 12, 4, 8
    b0 = torch.randn((n, H, W, ld0), device="cuda", generator=g)
    b1 = torch.randn((n, H, W, ld1), device="cuda", generator=g)
    a0, a1 = _off(b0, o0), _off(b1, o1)
    # positive shifts: a prologue applied to padding would leave relu(shift) > 0 there. Source 0: one affine for all samples;
    # source 1: per sample, (scale, shift) * mask with about half of the masks exactly 0 (Dropout2d folded into the affine)
    sc0 = torch.randn(C0, device="cuda", generator=g)
    sh0 = torch.rand(C0, device="cuda", generator=g) + 0.25
    mask = (torch.rand((n, C1), device="cuda", generator=g) >= 0.5).float() * 2.0
    assert 0 < int((mask == 0).sum()) < n * C1
    sc1 = (torch.randn(C1, device="cuda", generator=g)[None] * mask).contiguous()
    sh1 = ((torch.rand(C1, device="cuda", generator=g) + 0.25)[None] * mask).contiguous()
    Ts = [_lib.value("mss_wino_num_tiles", n, H, W, (m + 1) * d, t) for m, t in enumerate(tiles)]
    sizes = [(t + 2) ** 2 * T * C for t, T in zip(tiles, Ts)]

    # reference: w materialised, then the single-source kernel
    w = torch.empty((n, H, W, C), device="cuda")
    call("mss_affine_relu_nhwc_f32", a0, ld0, ptr(w), C, n * H * W, C0, ptr(sc0), ptr(sh0), 1)
    for i in range(n):
        call("mss_affine_relu_nhwc_f32", _off(b1, i * H * W * ld1 + o1), ld1, _off(w, i * H * W * C + C0), C, H * W, C1, ptr(sc1[i]),
             ptr(sh1[i]), 1)
    assert float(w.min()) == 0.0 and float(w.max()) > 0.0
    want = [_with_canary(s) for s in sizes]
    call("mss_wino_input_transform_aspp3_f32", ptr(w), C, n, H, W, C, d, (ctypes.c_int * 3)(*tiles), *[ptr(t) for t in want])

    got = [_with_canary(s) for s in sizes]
    sums, gap = _with_canary(n * d * d * C), _with_canary(n * C)
    rc = _src2(a0, ld0, C0, sc0, sh0, a1, ld1, C1, sc1, sh1, n, H, W, d, tiles, got, sums, gap)
    assert rc == 0, rc
    for m in range(3):
        assert not torch.isnan(want[m][:sizes[m]]).any()
        assert torch.equal(got[m][:sizes[m]], want[m][:sizes[m]]), f"dilation {(m + 1) * d}"
        assert torch.isnan(got[m][sizes[m]:]).all() and torch.isnan(want[m][sizes[m]:]).all()
    assert torch.isnan(sums[n * d * d * C:]).all() and torch.isnan(gap[n * C:]).all()

    # sums-only mode: the same bits
    sums2, gap2 = _with_canary(n * d * d * C), _with_canary(n * C)
    rc = _src2(a0, ld0, C0, sc0, sh0, a1, ld1, C1, sc1, sh1, n, H, W, d, tiles, [None, None, None], sums2, gap2)
    assert rc == 0, rc
    assert torch.equal(sums2[:n * d * d * C], sums[:n * d * d * C]) and torch.equal(gap2[:n * C], gap[:n * C])
    assert torch.isnan(sums2[n * d * d * C:]).all() and torch.isnan(gap2[n * C:]).all()

    # against float64 sums of the materialised map, per channel: every fp32 addition of at most H*W terms rounds by at most
    # 2^-24 of a partial sum <= sum|w|
    ref = w.double().sum(dim=(1, 2))                                       # [n, C]
    bound = H * W * 2.0 ** -24 * w.double().abs().sum(dim=(1, 2))
    worst = 0.0
    for name, s in (("full", (sums, gap)), ("sums-only", (sums2, gap2))):
        col = s[0][:n * d * d * C].view(n, d * d, C).double().sum(dim=1)
        mean = s[1][:n * C].view(n, C).double() * (H * W)
        for what, v in (("column sums", col), ("gap * HW", mean)):
            err = (v - ref).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), (name, what, ratio)
    print(f"aspp3_src2 sums n={n} {H}x{W} C={C0}+{C1} d={d}: worst |err| / bound = {worst:.3e}")


def test_two_source_transform_refuses_what_it_does_not_take():
    x = torch.zeros(1, 16, 16, 16, device="cuda")
    v = torch.ones(16, device="cuda")
    o = torch.zeros(1 << 20, device="cuda")
    xo = [o, o, o]

    def run(tiles=(4, 4, 4), xts=xo, sums=o, gap=o, C0=8, C1=8, H=16, W=16, d=4, src=x, ld=16, null_tiles=False, scale=v):
        ct = None if null_tiles else (ctypes.c_int * 3)(*tiles)
        return status("mss_wino_input_transform_aspp3_src2_f32", ptr(src), ld, C0, ptr(scale), ptr(v), 0, _off(src, 8), ld, C1, ptr(v), ptr(v), 0,
                      1, H, W, d, ct, ptr(xts[0]), ptr(xts[1]), ptr(xts[2]), ptr(sums), ptr(gap))
    assert run() == 0
    assert run(tiles=(2, 4, 4)) == _lib.MSS_ERR_UNSUPPORTED                      # a 2 x 2 tile
    big = torch.zeros(1, 512, 1024, 8, device="cuda")                            # 43 x 86 base sub-grids: more than LDS holds
    assert run(tiles=(6, 6, 6), C0=4, C1=4, H=512, W=1024, d=12, src=big, ld=8) == _lib.MSS_ERR_UNSUPPORTED
    # the host query says so beforehand (what aspp_plan asks, so that no caller meets the refusal at a launch)
    assert _lib.value("mss_wino_aspp3_supported", 1, 512, 1024, 8, 12, (ctypes.c_int * 3)(6, 6, 6), 1) == 0
    assert _lib.value("mss_wino_aspp3_supported", 1, 16, 16, 16, 4, (ctypes.c_int * 3)(2, 4, 4), 1) == 0
    assert _lib.value("mss_wino_aspp3_supported", 1, 16, 16, 16, 4, (ctypes.c_int * 3)(4, 4, 4), 1) == 1
    assert run(null_tiles=True) == _lib.MSS_ERR_BAD_ARG
    assert run(scale=None) == _lib.MSS_ERR_BAD_ARG                               # both sources carry a prologue
    assert run(C0=6, C1=8) == _lib.MSS_ERR_BAD_ARG                               # channel counts in quads
    assert run(xts=[o, None, o]) == _lib.MSS_ERR_BAD_ARG                         # all three X' or none
    assert run(xts=[None, None, None], sums=None, gap=None) == _lib.MSS_ERR_BAD_ARG      # nothing asked for
    assert run(sums=o, gap=None) == _lib.MSS_ERR_BAD_ARG                         # the sums come with their average
    torch.cuda.synchronize()
