"""Every base Winograd transform kernel of csrc/winograd.hip alone against the float64 restatement in tests/ref_winograd.py (exact
rational matrices, geometry restated from include/mss_hip.h): mss_wino_input_transform_f32 in each of its seven kernel variants,
mss_wino_pack_weights_f32, mss_wino_output_transform_f32 (whole-tile-per-thread and LDS-staged, every lane mapping, statistics),
mss_wino_grad_output_transform_f32 and mss_wino_weight_grad_transform_f32, and the argument checks of all five.

The bound is derived, not measured. A transform is two passes of dot products of at most n terms (n = m + 2; 3 for the weight pack)
with coefficients rounded to fp32, so by the standard running-error bound every element satisfies
    |got - float64| <= (2n + 4) * 2^-24 * (|L| |X| |R|)
componentwise, the right side evaluated in float64 (floor 1e-300: where it is 0, the kernel must write an exact 0 -- tile positions
outside the image, padding rows and columns of U). The BatchNorm+ReLU prologue adds |L| E |R| with E = 2 * 2^-24 * (|x * scale| +
|shift|), a residual adds 2^-24 * |y|. Inputs are mixed-sign normal with one channel in eight scaled by 1e3 and one by 1e-3, so that
the componentwise bound holds the small channels to their own size. Outputs carry a NaN canary tail, inputs are channel slices of
wider buffers. The worst |err| / bound per kernel goes to winograd_kernels.json in the report directory (test_reports/ in the tree,
or what MSS_REPORT_DIR names).

Left out: the LDS input transform's chunk-slowest grid (`chunk_fast == false`), which needs 2^31 workgroups. The LDS output
transform's lane mapping for K > 128 walks one tile per wave iteration, so "a tile count that is no multiple of the tiles per
iteration" does not exist there."""
import ctypes
import json
import os

import pytest
import torch

import ref_winograd as R
from conftest import ROOT
from multishiftseg_amd import _lib
from multishiftseg_amd._lib import call, ptr, status, value

pytestmark = pytest.mark.gpu

CANARY = 64
NAN = float("nan")


@pytest.fixture(scope="module")
def report():
    worst = {}
    yield worst
    if not worst:
        return
    out = os.environ.get("MSS_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "winograd_kernels.json"), "a") as f:
            f.write(json.dumps({k + "_worst_ratio_to_bound": v for k, v in worst.items()}, sort_keys=True) + "\n")
    except OSError:
        pass


def _note(report, key, ratio):
    report[key] = max(report.get(key, 0.0), ratio)


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1009 + int(v)
    return torch.Generator(device="cuda").manual_seed(s)


def _scaled(t):
    """One channel (last dimension) in eight times 1e3, one in eight times 1e-3."""
    c = torch.arange(t.shape[-1], device=t.device)
    f = torch.ones(t.shape[-1], device=t.device)
    f[c % 8 == 1] = 1e3
    f[c % 8 == 5] = 1e-3
    return t * f


def _wide(shape, g, pad=8, off=4):
    """A mixed-sign map [..., C] as the channel slice [off, off + C) of a wider NaN-free buffer (ld = C + pad); (view, pointer, ld)."""
    C = shape[-1]
    buf = torch.randn(tuple(shape[:-1]) + (C + pad,), device="cuda", generator=g) * 7.0
    view = buf[..., off:off + C]
    view.copy_(_scaled(torch.randn(tuple(shape), device="cuda", generator=g)))
    return view, ctypes.c_void_p(buf.data_ptr() + 4 * off), C + pad


def _canary(n):
    return torch.full((n + CANARY,), NAN, device="cuda", dtype=torch.float32)


def _check(got, ref, bound, what):
    """Componentwise |got - ref| <= max(bound, 1e-300); returns the worst ratio."""
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    assert not torch.isnan(got).any(), what
    err = (got.double() - ref).abs()
    b = bound.clamp_min(1e-300)
    ratio = float((err / b).max())
    print(f"{what}: worst |err| / bound = {ratio:.3e}")
    assert bool((err <= b).all()), (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------- input transform
# (variant, tile, env MSS_WINO_INPUT_LDS (None: the default policy), N, H, W, C, dil, prologue)
INPUT_CASES = [
    # one thread per tile
    ("thread2", 2, None, 2, 7, 9, 12, 1, True), ("thread2", 2, None, 1, 5, 7, 8, 3, False), ("thread2", 2, None, 1, 2, 7, 8, 3, True),
    ("thread4", 4, "0", 2, 9, 11, 12, 2, True), ("thread4", 4, "0", 1, 6, 7, 8, 1, False), ("thread4", 4, None, 1, 13, 40, 8, 6, True),
    ("thread6", 6, "0", 2, 9, 15, 12, 2, True), ("thread6", 6, "0", 1, 13, 7, 8, 1, False),
    # LDS F(4x4), 2 x 4 tile blocks, 64-channel chunks: default policy (9 x 11 tiles fill 82 % of 5 x 3 blocks), then forced
    ("lds4_2x4", 4, None, 2, 69, 84, 68, 2, True), ("lds4_2x4", 4, "2", 2, 21, 19, 20, 2, True), ("lds4_2x4", 4, "2", 1, 11, 18, 132, 1, False),
    # LDS F(4x4), 1 x 2 tile blocks, 256-channel chunks
    ("lds4_1x2", 4, None, 2, 7, 16, 132, 2, True), ("lds4_1x2", 4, "2", 1, 4, 11, 516, 1, False), ("lds4_1x2", 4, "2", 2, 10, 3, 8, 1, True),
    # LDS F(6x6), 2 x 2 tile blocks, 64-channel chunks
    ("lds6_2x2", 6, None, 2, 27, 30, 20, 2, True), ("lds6_2x2", 6, None, 1, 14, 17, 132, 1, False),
    # LDS F(6x6), 1 x 2 tile blocks, 128-channel chunks
    ("lds6_1x2", 6, None, 2, 11, 34, 68, 2, True), ("lds6_1x2", 6, None, 1, 15, 5, 260, 1, False), ("lds6_1x2", 6, None, 1, 2, 20, 8, 3, True),
]


def _input_plan(tile, env, geo, dil):
    """The branch wino_input_transform_impl takes, restated: the variant's name and, for the LDS variants, the channel chunk, the
    tile-block shape and the fill of the tile-block grid."""
    if tile == 2 or env == "0":
        return dict(name=f"thread{tile}", fill=None)
    big = (geo["tH"] >= 2 and geo["tW"] >= 3) if tile == 4 else (geo["tH"] >= 2 and geo["tW"] >= 2)
    tyb, txb = (2 if big else 1), (4 if big and tile == 4 else 2)
    fill = geo["tH"] * geo["tW"] / (-(-geo["tH"] // tyb) * tyb * -(-geo["tW"] // txb) * txb)
    if not ((fill >= 0.8 and dil <= 4) or env == "2" or tile == 6):
        return dict(name=f"thread{tile}", fill=fill)
    return dict(name=f"lds{tile}_{tyb}x{txb}", fill=fill, cb=1024 // (tyb * txb * (2 if tile == 4 else 4)), tyb=tyb, txb=txb)


@pytest.mark.parametrize("variant,tile,env,N,H,W,C,dil,prologue", INPUT_CASES)
def test_input_transform(variant, tile, env, N, H, W, C, dil, prologue, monkeypatch, report):
    if env is None:
        monkeypatch.delenv("MSS_WINO_INPUT_LDS", raising=False)
    else:
        monkeypatch.setenv("MSS_WINO_INPUT_LDS", env)
    geo = R.geom(N, H, W, dil, tile)
    plan = _input_plan(tile, env, geo, dil)
    assert plan["name"] == variant, (geo, plan)
    if (tile, env, dil) == (4, None, 6):
        assert plan["fill"] >= 0.8 and dil > 4                  # full tile blocks: the dilation alone keeps it off the LDS kernel
    T, P = geo["T"], tile + 2
    assert T == value("mss_wino_num_tiles", N, H, W, dil, tile)
    g = _gen(N, H, W, C, dil, tile)
    x, xp, ld = _wide((N, H, W, C), g)
    scale = shift = None
    if prologue:                      # positive shifts (a prologue applied to the padding would show), about half the scales negative
        sign = torch.where(torch.arange(C, device="cuda") % 3 == 0, -1.0, 1.0) * torch.where(torch.arange(C, device="cuda") % 8 < 4, 1.0, -1.0)
        scale = (torch.rand(C, device="cuda", generator=g) + 0.5) * sign
        shift = torch.rand(C, device="cuda", generator=g) + 0.25
        assert abs(int((scale < 0).sum()) - C // 2) <= max(2, C // 8)
    size = P * P * T * C
    xt = _canary(size)
    call("mss_wino_input_transform_f32", xp, ld, N, H, W, C, dil, tile, ptr(scale), ptr(shift), int(prologue), ptr(xt))
    torch.cuda.synchronize()
    assert torch.isnan(xt[size:]).all()
    got = xt[:size].view(P * P, T, C)
    ref = R.input_transform(x, dil, tile, scale, shift, prologue)
    mag = R.input_transform_mag(x, dil, tile, scale, shift, prologue)
    bound = R.transform_bound(mag, P)
    if prologue:
        bound = bound + R.input_prologue_error(x, dil, tile, scale, shift)
    # tile positions outside the image are the transform of zeros: an exact 0 wherever no pixel of the image reaches the element
    reach = R.input_transform_mag(torch.ones_like(x), dil, tile)
    assert bool((got[reach == 0] == 0).all())
    if H < dil:
        assert bool((reach.amax(dim=(0, 2)) == 0).any())        # the tiles of an empty residue sub-grid
    _note(report, "input_" + variant, _check(got, ref, bound, f"input {variant} {N}x{H}x{W}x{C} d={dil} prologue={prologue}"))


def test_input_transform_cases_reach_every_variant_and_edge():
    """The shapes above against the launch plan: every kernel variant is reached, with and without the prologue; every LDS variant
    sees a channel count below one chunk, three or more chunks with a ragged last one, a tile-block grid that is ragged in every
    direction in which its block has more than one tile, residue sub-grids of different sizes (H % d != 0) and two samples; and the
    F(4x4) variants are reached under the default policy too."""
    seen = {}
    for variant, tile, env, N, H, W, C, dil, prologue in INPUT_CASES:
        geo = R.geom(N, H, W, dil, tile)
        plan = _input_plan(tile, env, geo, dil)
        s = seen.setdefault(plan["name"], set())
        s.add("prologue" if prologue else "plain")
        if env is None:
            s.add("default policy")
        if "cb" not in plan:
            continue
        if C < plan["cb"]:
            s.add("below a chunk")
        if C > 2 * plan["cb"] and C % plan["cb"]:
            s.add("ragged chunks")
        if geo["tW"] % plan["txb"] and (plan["tyb"] == 1 or geo["tH"] % plan["tyb"]):
            s.add("ragged grid")
        if H % dil:
            s.add("uneven sub-grids")
        if N == 2:
            s.add("two samples")
    assert set(seen) == {"thread2", "thread4", "thread6", "lds4_2x4", "lds4_1x2", "lds6_2x2", "lds6_1x2"}
    for name, s in seen.items():
        assert {"prologue", "plain"} <= s, (name, s)
        if name.startswith("lds"):
            assert {"below a chunk", "ragged chunks", "ragged grid", "uneven sub-grids", "two samples"} <= s, (name, s)
        if "4" in name:
            assert "default policy" in s, (name, s)


# ------------------------------------------------------------------------------------------------------------------ pack weights
WEIGHT_SHAPES = [(36, 20, 128, 32), (132, 48, 256, 48)]          # K < Kpad, C < Cp; C == Cp


def _weights(K, C, g):
    """Mixed sign, one input channel in eight times 1e3 and one times 1e-3."""
    return _scaled(torch.randn((K, 3, 3, C), device="cuda", generator=g)).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("K,C,Kpad,Cp", WEIGHT_SHAPES)
@pytest.mark.parametrize("tile", [2, 4, 6])
def test_pack_weights(tile, K, C, Kpad, Cp, report):
    P = tile + 2
    w = _weights(K, C, _gen(tile, K, C))
    size = P * P * Kpad * Cp
    u = _canary(size)
    call("mss_wino_pack_weights_f32", ptr(w), ptr(u), K, C, Kpad, Cp, tile)
    torch.cuda.synchronize()
    assert torch.isnan(u[size:]).all()
    got = u[:size].view(P * P, Kpad, Cp)
    assert bool((got[:, K:, :] == 0).all()) and bool((got[:, :, C:] == 0).all())
    _note(report, "pack_weights", _check(got, R.pack_weights(w, tile, Kpad, Cp), R.transform_bound(R.pack_weights_mag(w, tile, Kpad, Cp), 3),
                                         f"pack_weights F({tile}x{tile}) K={K} C={C}"))


# --------------------------------------------------------------------------------------------------------------- output transform
def _qw_log2(K):
    """wino_output_qw_log2 restated: channel quads per tile inside a wave of the LDS output transform."""
    l = 6
    while l > 2 and (1 << (l - 1)) >= K // 4:
        l -= 1
    return l


def _run_output(N, H, W, K, dil, tile, with_res, with_stats, wide_y, report, key):
    geo = R.geom(N, H, W, dil, tile)
    T, P = geo["T"], tile + 2
    g = _gen(N, H, W, K, dil, tile)
    yt = _scaled(torch.randn((P * P, T, K), device="cuda", generator=g))
    res = rp = None
    ldres = 0
    if with_res:
        res, rp, ldres = _wide((N, H, W, K), g)
        assert ldres > K
    ldy, off = (K + 8, 4) if wide_y else (K, 0)
    pixels = N * H * W
    ybuf = _canary(pixels * ldy)
    parts = value("mss_wino_output_stats_parts", N, H, W, K, dil, tile)
    assert parts >= 1
    stats = _canary(parts * 2 * K) if with_stats else None
    call("mss_wino_output_transform_f32", ptr(yt), N, H, W, K, dil, tile, rp, ldres, ctypes.c_void_p(ybuf.data_ptr() + 4 * off), ldy,
         ptr(stats))
    torch.cuda.synchronize()
    assert torch.isnan(ybuf[pixels * ldy:]).all()
    rows = ybuf[:pixels * ldy].view(N, H, W, ldy)
    if wide_y:
        assert torch.isnan(rows[..., :off]).all() and torch.isnan(rows[..., off + K:]).all()
    got = rows[..., off:off + K]
    y0 = R.output_transform(yt, N, H, W, dil, tile)
    assert not torch.isnan(y0).any()
    bound = R.transform_bound(R.output_transform_mag(yt, N, H, W, dil, tile), P)
    ref = y0
    if with_res:
        ref = y0 + res.double()
        bound = bound + R.U32 * ref.abs()
    what = f"output F({tile}x{tile}) {N}x{H}x{W}x{K} d={dil} res={with_res} stats={with_stats}"
    _note(report, key, _check(got, ref, bound, what))
    if with_stats:
        n = parts * 2 * K
        assert torch.isnan(stats[n:]).all() and not torch.isnan(stats[:n]).any()
        s = stats[:n].view(parts, 2, K).double().sum(dim=0)
        yd = got.double()
        for i, (name, want, sbound) in enumerate((("sum", yd.sum(dim=(0, 1, 2)), pixels * R.U32 * yd.abs().sum(dim=(0, 1, 2))),
                                                  ("sum of squares", (yd * yd).sum(dim=(0, 1, 2)), pixels * R.U32 * (yd * yd).sum(dim=(0, 1, 2))))):
            _note(report, key + "_stats", _check(s[i], want, sbound, what + " " + name))
    return geo, parts


@pytest.mark.parametrize("tile,N,H,W,K,dil,with_res,with_stats,wide_y", [
    (2, 2, 7, 9, 12, 1, True, True, False), (2, 1, 5, 7, 8, 3, False, False, True), (2, 1, 9, 6, 260, 2, True, False, False),
    (4, 2, 9, 11, 132, 2, True, True, False), (4, 1, 6, 7, 260, 1, False, True, True), (4, 1, 13, 5, 8, 3, True, False, False),
])
def test_output_transform_per_thread(tile, N, H, W, K, dil, with_res, with_stats, wide_y, report):
    """F(2x2), and F(4x4) below 2^25 output elements: one thread per (tile, channel quad)."""
    assert N * H * W * K < 1 << 25
    _run_output(N, H, W, K, dil, tile, with_res, with_stats, wide_y, report, f"output_thread{tile}")


@pytest.mark.parametrize("K,l", [(8, 2), (24, 3), (48, 4), (100, 5), (272, 6)])
@pytest.mark.parametrize("N,H,W,dil,with_res,with_stats,wide_y", [(1, 13, 17, 1, True, True, False), (1, 11, 39, 3, False, False, True),
                                                                  (2, 8, 27, 2, False, True, False)])
def test_output_transform_lds_f6_every_lane_mapping(K, l, N, H, W, dil, with_res, with_stats, wide_y, report):
    """F(6x6): every value of the lane mapping's quad-group size (K / 4 no multiple of it for K = 100 and 272), and tile counts 9, 27
    and 24 against 16, 8, 4, 2 and 1 tiles per iteration."""
    assert _qw_log2(K) == l
    geo = R.geom(N, H, W, dil, 6)
    tpi = 64 >> l
    if (N, dil) != (2, 2):
        assert geo["T"] % 2 == 1 and (tpi == 1 or geo["T"] % tpi)
    if K in (100, 272):
        assert (K // 4) % (1 << l)
    _run_output(N, H, W, K, dil, 6, with_res, with_stats, wide_y, report, "output_lds6")


def test_output_transform_lds_f6_several_iterations(report):
    """More tile groups than workgroup rows: the workgroups walk the tiles in several iterations, the last one ragged."""
    N, H, W, K, dil = 1, 197, 190, 272, 1
    geo = R.geom(N, H, W, dil, 6)
    parts = value("mss_wino_output_stats_parts", N, H, W, K, dil, 6)
    assert _qw_log2(K) == 6 and parts < geo["T"] and geo["T"] % parts
    _run_output(N, H, W, K, dil, 6, True, True, False, report, "output_lds6")


def test_output_transform_lds_f4_at_2_pow_25(report):
    """wino_output_transform_lds_kernel<4>, which only maps of at least 2^25 output elements take: ragged for the tile in both
    directions, dilation 2, residual and statistics."""
    N, H, W, K, dil = 1, 127, 259, 1024, 2
    assert N * H * W * K >= 1 << 25
    geo = R.geom(N, H, W, dil, 4)
    assert H % dil and W % dil                                 # the residue sub-grids differ in size, and of those ...
    assert any(-(-(H - a) // dil) % 4 for a in range(dil)) and any(-(-(W - b) // dil) % 4 for b in range(dil))    # ... some are ragged
    _, parts = _run_output(N, H, W, K, dil, 4, True, True, False, report, "output_lds4")
    assert parts == 512 and geo["T"] % parts          # the LDS kernel's plan (2048 / 4 workgroup rows), several ragged iterations


# ---------------------------------------------------------------------------------------------------------- grad-output transform
@pytest.mark.parametrize("K", [4, 132])
@pytest.mark.parametrize("dil", [1, 3])
@pytest.mark.parametrize("tile", [2, 4, 6])
def test_grad_output_transform(tile, dil, K, report):
    N, H, W = 2, 13, 19
    geo = R.geom(N, H, W, dil, tile)
    assert geo["Hs"] % tile and geo["Ws"] % tile and (dil == 1 or (H % dil and W % dil))
    T, P = geo["T"], tile + 2
    dy, dp, ld = _wide((N, H, W, K), _gen(tile, dil, K))
    assert ld > K
    size = P * P * T * K
    dyt = _canary(size)
    call("mss_wino_grad_output_transform_f32", dp, ld, N, H, W, K, dil, tile, ptr(dyt))
    torch.cuda.synchronize()
    assert torch.isnan(dyt[size:]).all()
    got = dyt[:size].view(P * P, T, K)
    reach = R.grad_output_transform_mag(torch.ones_like(dy), dil, tile)
    assert bool((got[reach == 0] == 0).all())
    assert bool((reach == 0).any())                            # e.g. the last Winograd row of a tile whose last pixel row is outside
    _note(report, "grad_output", _check(got, R.grad_output_transform(dy, dil, tile), R.transform_bound(R.grad_output_transform_mag(dy, dil, tile), P),
                                        f"grad_output F({tile}x{tile}) {N}x{H}x{W}x{K} d={dil}"))


# ----------------------------------------------------------------------------------------------------------- weight-grad transform
@pytest.mark.parametrize("K,C,Kpad,Cp", WEIGHT_SHAPES)
@pytest.mark.parametrize("tile", [2, 4, 6])
def test_weight_grad_transform(tile, K, C, Kpad, Cp, report):
    P = tile + 2
    g = _gen(tile, K, C, 7)
    du = torch.full((P * P, Kpad, Cp), NAN, device="cuda")                    # the padding is never read
    du[:, :K, :C] = _scaled(torch.randn((P * P, K, C), device="cuda", generator=g))
    size = K * C * 9
    dw = _canary(size)
    call("mss_wino_weight_grad_transform_f32", ptr(du), ptr(dw), K, C, Kpad, Cp, tile)
    torch.cuda.synchronize()
    assert torch.isnan(dw[size:]).all()
    _note(report, "weight_grad", _check(dw[:size].view(K, C, 3, 3), R.weight_grad_transform(du, K, C, tile),
                                        R.transform_bound(R.weight_grad_transform_mag(du, K, C, tile), P), f"weight_grad F({tile}x{tile}) K={K} C={C}"))


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    BAD = _lib.MSS_ERR_BAD_ARG
    o = torch.zeros(1 << 16, device="cuda")
    v = torch.ones(16, device="cuda")

    def inp(C=8, ld=8, tile=4, dil=1, scale=None, shift=None):
        return status("mss_wino_input_transform_f32", ptr(o), ld, 1, 8, 8, C, dil, tile, ptr(scale), ptr(shift), 0, ptr(o))
    assert inp() == 0 and inp(scale=v, shift=v) == 0
    assert inp(C=6) == BAD and inp(ld=10) == BAD and inp(tile=3) == BAD and inp(dil=0) == BAD and inp(scale=v) == BAD

    def out(K=8, ldy=8, ldres=8, tile=4, dil=1, res=o):
        return status("mss_wino_output_transform_f32", ptr(o), 1, 8, 8, K, dil, tile, ptr(res), ldres, ptr(o), ldy, None)
    assert out() == 0 and out(res=None, ldres=3) == 0
    assert out(K=6) == BAD and out(ldy=10) == BAD and out(ldres=10) == BAD and out(tile=3) == BAD and out(dil=0) == BAD
    assert value("mss_wino_output_stats_parts", 1, 8, 8, 6, 1, 4) == -1 and value("mss_wino_output_stats_parts", 1, 8, 8, 8, 0, 4) == -1
    assert value("mss_wino_output_stats_parts", 1, 8, 8, 8, 1, 3) == -1 and value("mss_wino_num_tiles", 1, 8, 8, 1, 3) == -1
    assert value("mss_wino_num_tiles", 1, 8, 8, 0, 4) == -1

    def gout(K=8, ld=8, tile=4, dil=1):
        return status("mss_wino_grad_output_transform_f32", ptr(o), ld, 1, 8, 8, K, dil, tile, ptr(o))
    assert gout() == 0
    assert gout(K=6) == BAD and gout(ld=10) == BAD and gout(tile=3) == BAD and gout(dil=0) == BAD

    def pack(name, K=8, C=8, Kpad=8, Cp=8, tile=4):
        return status(name, ptr(o), ptr(o), K, C, Kpad, Cp, tile)
    for name in ("mss_wino_pack_weights_f32", "mss_wino_weight_grad_transform_f32"):
        assert pack(name) == 0
        assert pack(name, Kpad=4) == BAD and pack(name, Cp=4) == BAD and pack(name, tile=3) == BAD
    torch.cuda.synchronize()
