"""MSDeformAttn on the sample locations the other MSDA tests avoid: pixel coordinates that are integers (the kinks of the
piecewise bilinear surface -- a third of all coordinates when training starts) and the image borders -1, 0, E-1, E.

Sections 1-2 use the dyadic recipe of tests/ref_msda_cells.py (power-of-two level extents, coordinates / values / weights /
gradients on coarse dyadic grids): every product and sum of the op is exact in fp32 -- the forward, the three gradients, the
64-bit fixed-point accumulation and the halo merge of the binned backward -- so EVERY route must return the float64
reference bit for bit (tests/test_msda_cells_ref_cpu.py proves the recipe exact and the reference equal to oracle/msda.py).
Section 3 is the encoder's state at initialisation, where the reference is evaluated in both cells next to each kink.
Section 4 puts NaN, infinite and absurd coordinates through every route: they fail the inside test and contribute nothing."""
import ctypes

import numpy as np
import pytest
import torch

import ref_msda_cells as R
from oracle import msda as omsda

pytestmark = pytest.mark.gpu

M, P = 8, 4
# Tile classes of msda_bin_geom (csrc/msda.hip) at these sizes, target 750 records per tile:
#  "tiles": (32,64) -> 16x16 tiles, 2x4 of them; (8,8) -> 4x4, 2x2 (the dense class); (16,32) -> 8x16, 2x2: halos in both
#           directions on every level.
#  "thin":  (1,256) / (256,1) -> tile edge capped at 143: two ragged tiles each, no second row / column, so h0 + 1 <= H - 1 is
#           never true; (4,4) -> one 4x4 tile.
GEOM = {"tiles": ([(32, 64), (8, 8), (16, 32)], 2, 1024), "thin": ([(1, 256), (256, 1), (4, 4)], 2, 300)}
FWD_TOL = dict(rtol=1e-4, atol=2e-5)          # the fp32 tolerances of tests/test_gpu_msda.py
GRAD_TOL = dict(rtol=1e-3, atol=1e-4)
NAMES = ("grad_value", "grad_loc", "grad_attn")

_inputs, _fwd_ref, _bwd_ref = {}, {}, {}


def lattice(tag, D):
    if (tag, D) not in _inputs:
        shapes, N, Lq = GEOM[tag]
        g = R.lattice_inputs(41 + D, shapes, N, Lq, M, P, D)
        for l, (H, W) in enumerate(shapes):               # the edge values are really there
            for ax, E in ((0, W), (1, H)):
                for edge in (-1, 0, E - 1, E):
                    assert (g["p"][:, :, :, l, :, ax] == edge).any(), (tag, l, ax, edge)
        for a in g.values():
            a.setflags(write=False)
        _inputs[tag, D] = g
    return _inputs[tag, D]


def forward_ref(tag, D):
    if (tag, D) not in _fwd_ref:
        g = lattice(tag, D)
        out = R.forward(g["value"], g["shapes"], g["starts"], g["loc"], g["attn"], *R.cells(g["loc"], g["shapes"]))
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out) and np.abs(out).max() > 0
        out.setflags(write=False)
        _fwd_ref[tag, D] = out
    return _fwd_ref[tag, D]


def backward_ref(tag, D):
    if (tag, D) not in _bwd_ref:
        g = lattice(tag, D)
        res = R.backward(g["value"], g["shapes"], g["starts"], g["loc"], g["attn"], g["grad_out"], *R.cells(g["loc"], g["shapes"]))
        for a in res:
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.abs(a).max() > 0
            a.setflags(write=False)
        _bwd_ref[tag, D] = res
    return _bwd_ref[tag, D]


def dev(a, dtype=np.float32):
    a = np.asarray(a)
    return torch.from_numpy(np.array(a, dtype=dtype if a.dtype.kind == "f" else a.dtype, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def assert_same(got, want, name):
    """Equality by value (-0 == 0); on failure names the first differing element."""
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(~(got == want))
        i = tuple(bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} elements differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


ROUTES = {"d32": (32, np.float32, None), "d32_atomics": (32, np.float32, "0"), "d16": (16, np.float32, None),
          "d64": (64, np.float32, None), "d24_generic": (24, np.float32, None), "f64": (32, np.float64, None)}


def op_args(g, dtype):
    return [dev(g["value"], dtype), dev(g["shapes"]), dev(g["starts"]), dev(g["loc"], dtype), dev(g["attn"], dtype)]


# ---- 2. exact tests on dyadic inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["d32", "d16", "d64", "d24_generic", "f64"])
@pytest.mark.parametrize("tag", ["tiles", "thin"])
def test_forward_is_exact_on_the_lattice(tag, route):
    """The record kernel with 8 / 4 / 16 lanes per head (D = 32 / 16 / 64), the generic fp32 kernel (D = 24) and float64."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    D, dtype, _ = ROUTES[route]
    out = MSDA.ms_deform_attn_forward(*op_args(lattice(tag, D), dtype), 128)
    assert_same(out, forward_ref(tag, D), "out")


@pytest.mark.parametrize("route", ["d32", "d32_atomics", "d16", "d64", "f64"])
@pytest.mark.parametrize("tag", ["tiles", "thin"])
def test_backward_is_exact_on_the_lattice(monkeypatch, tag, route):
    """D = 32 on the binned owner-computes route (fixed-point tiles, halo merge, gather pass) and on the generic kernel with
    float atomics; D = 16 / 64: the generic kernel with 32 / 64 lanes per pair; float64."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    D, dtype, binned = ROUTES[route]
    monkeypatch.setenv("MSS_MSDA_BWD_BINNED", binned or "1")
    g = lattice(tag, D)
    got = MSDA.ms_deform_attn_backward(*op_args(g, dtype), dev(g["grad_out"], dtype), 128)
    for a, want, name in zip(got, backward_ref(tag, D), NAMES):
        assert_same(a, want, name)


@pytest.mark.parametrize("tag", ["tiles", "thin"])
def test_binned_backward_is_exact_on_nan_filled_workspace_and_outputs(tag):
    """mss_msda_backward_binned_f32 called directly, once on a zeroed workspace and once with the workspace and all three
    outputs filled with NaN bit patterns: every word it reads it has written first (counts, scan, records, halos), so both
    runs give the reference's bits."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    from multishiftseg_amd import _lib
    from multishiftseg_amd._lib import call, ptr
    g = lattice(tag, 32)
    shapes, N, Lq = GEOM[tag]
    L, S = len(shapes), g["value"].shape[1]
    value, shp, starts, loc, attn = op_args(g, np.float32)
    gout = dev(g["grad_out"])
    hs = MSDA.host_shapes(shp)
    nbytes = _lib.value("mss_msda_backward_workspace_bytes", hs, N, M, 32, L, Lq, P)
    assert nbytes > 0 and nbytes % 4 == 0
    for fill in (0.0, float("nan")):
        ws = torch.full((nbytes // 4,), fill, device="cuda", dtype=torch.float32)
        assert ws.data_ptr() % 256 == 0
        gv, gl, ga = (torch.full_like(t, fill) for t in (value, loc, attn))
        call("mss_msda_backward_binned_f32", ptr(value), ptr(shp), ptr(starts), hs, ptr(loc), ptr(attn), ptr(gout), N, S, M, 32, L, Lq, P,
             ptr(gv), ptr(gl), ptr(ga), ptr(ws), nbytes)
        for a, want, name in zip((gv, gl, ga), backward_ref(tag, 32), NAMES):
            assert_same(a, want, f"{name} (workspace filled with {fill})")


@pytest.mark.parametrize("binned", ["1", "0"])
def test_zero_output_gradient_gives_exact_zeros(monkeypatch, binned):
    """grad_out == 0 everywhere: the binned route's scale bound max|grad_out| * max|attn| is 0. Zeros, not NaN."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    monkeypatch.setenv("MSS_MSDA_BWD_BINNED", binned)
    g = lattice("tiles", 32)
    args = op_args(g, np.float32)
    gv, gl, ga = (torch.full_like(t, float("nan")) for t in (args[0], args[3], args[4]))       # dirty the allocator's blocks
    del gv, gl, ga
    got = MSDA.ms_deform_attn_backward(*args, torch.zeros_like(dev(g["grad_out"])), 128)
    for a, name in zip(got, NAMES):
        assert_same(a, np.zeros(a.shape), name)


def fused_inputs():
    """Levels (16,32), (8,8), L*P = 8, every pixel a query; reference points are the pixel centres, offsets are the lattice
    coordinate minus the query's own pixel coordinate on that level, logits are 0: softmax gives exactly 1/8 and
    ref + off / size is exactly the lattice location."""
    shapes, N, D = [(16, 32), (8, 8)], 2, 32
    shp = np.asarray(shapes, dtype=np.int64)
    S, L = int(shp.prod(1).sum()), len(shapes)
    rng = np.random.default_rng(77)
    centres = np.concatenate([np.stack(np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij"), -1)
                              .reshape(-1, 2)[:, ::-1] for h, w in shapes])                   # [S, 2] (x, y)
    ref = np.broadcast_to(centres[None, :, None, :], (N, S, L, 2)).copy()
    size = shp[None, None, None, :, None, ::-1].astype(np.float64)
    p = R.lattice_coords(rng, shapes, N, S, M, P)
    own = ref[:, :, None, :, None, :] * size - 0.5                                            # the query's pixel coordinate per level
    off = p - own
    loc = (p + 0.5) / size
    f32 = np.float32
    assert np.array_equal((ref.astype(f32)[:, :, None, :, None, :] + off.astype(f32) / size.astype(f32)).astype(np.float64), loc)
    for a in (ref, off, loc):
        assert np.array_equal(a.astype(f32).astype(np.float64), a)
    attn = np.full((N, S, M, L, P), 0.125)
    value = rng.integers(-8, 9, (N, S, M, D)) / 8.0
    gout = rng.integers(-4, 5, (N, S, M * D)) / 4.0
    starts = R.level_starts(shp)
    c = R.cells(loc, shp)
    out = R.forward(value, shp, starts, loc, attn, *c)
    gv, gl, ga = R.backward(value, shp, starts, loc, attn, gout, *c)
    d_off = gl / size
    d_log = (attn * (ga - (attn * ga).sum((-1, -2), keepdims=True))).reshape(N, S, M, L * P)
    for a in (out, gv, d_off, d_log):
        assert np.array_equal(a.astype(f32).astype(np.float64), a) and np.abs(a).max() > 0
    return dict(shapes=shp, starts=starts, ref=ref, off=off, loc=loc, attn=attn, value=value, gout=gout, out=out, gv=gv,
                d_off=d_off, d_log=d_log, N=N, S=S, L=L, D=D)


@pytest.fixture(scope="module")
def fused():
    return fused_inputs()


def test_fused_forward_entry_points_are_exact_and_save_the_prepare_kernels_locations(fused):
    """mss_msda_forward_fused_f32 / _ld_f32 / _save_f32 and mss_msda_prepare_f32 + the op: the exact output; the locations
    the save form writes are bitwise those of the prepare kernel (both form ref + off / size) -- what lets
    _FusedSampleFn.backward land in the forward's cell."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    from multishiftseg_amd import _lib
    from multishiftseg_amd._lib import call, ptr
    f = fused
    N, S, L, D, Lq = f["N"], f["S"], f["L"], f["D"], f["S"]
    value, shp, starts, off, ref = dev(f["value"]), dev(f["shapes"]), dev(f["starts"]), dev(f["off"]), dev(f["ref"])
    lg = torch.zeros(N, Lq, M, L * P, device="cuda")
    out = torch.full((N, Lq, M * D), float("nan"), device="cuda")
    call("mss_msda_forward_fused_f32", ptr(value), ptr(shp), ptr(starts), ptr(off), ptr(lg), ptr(ref), N, S, M, D, L, Lq, P, ptr(out))
    assert_same(out, f["out"], "fused")
    ko, ka = M * L * P * 2, M * L * P
    ld = ko + ka + 4
    both = torch.full((N, Lq, ld), float("nan"), device="cuda")
    both[..., :ko] = off.view(N, Lq, ko)
    both[..., ko:ko + ka] = 0
    plog = ctypes.c_void_p(both.data_ptr() + 4 * ko)
    out = torch.full((N, Lq, M * D), float("nan"), device="cuda")
    call("mss_msda_forward_fused_ld_f32", ptr(value), ptr(shp), ptr(starts), ptr(both), ld, plog, ld, ptr(ref), N, S, M, D, L, Lq, P, ptr(out))
    assert_same(out, f["out"], "fused_ld")
    out = torch.full((N, Lq, M * D), float("nan"), device="cuda")
    loc_k, aw_k = torch.full_like(off, float("nan")), torch.full((N, Lq, M, L, P), float("nan"), device="cuda")
    rc = _lib.status("mss_msda_forward_fused_save_f32", ptr(value), ptr(shp), ptr(starts), ptr(both), ld, plog, ld, ptr(ref), N, S, M, D, L,
                     Lq, P, ptr(out), ptr(loc_k), ptr(aw_k))
    assert rc == 0
    assert_same(out, f["out"], "fused_save")
    loc_p, aw_p = torch.full_like(off, float("nan")), torch.full((N, Lq, M, L, P), float("nan"), device="cuda")
    call("mss_msda_prepare_f32", ptr(off), ptr(lg), ptr(ref), ptr(shp), N, Lq, M, L, P, ptr(loc_p), ptr(aw_p))
    assert torch.equal(loc_k, loc_p)
    assert_same(loc_p, f["loc"], "prepared locations")
    assert_same(aw_p, f["attn"], "prepared weights")
    assert_same(aw_k, f["attn"], "saved weights")
    assert_same(MSDA.ms_deform_attn_forward(value, shp, starts, loc_p, aw_p, 128), f["out"], "prepare + op")


@pytest.mark.parametrize("binned", ["1", "0"])
def test_fused_backward_forms_are_exact(monkeypatch, fused, binned):
    """d(offsets), d(logits) and grad_value of MSDA.ms_deform_attn_backward_proj (the module's backward folded into the
    gather pass; binned route only) and of _FusedSampleFn's own backward."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    from multishiftseg_amd.ms_deform_attn import _FusedSampleFn
    monkeypatch.setenv("MSS_MSDA_BWD_BINNED", binned)
    monkeypatch.setenv("MSS_MSDA_BWD_PROJ", "1")
    f = fused
    N, S, L, D, Lq = f["N"], f["S"], f["L"], f["D"], f["S"]
    shp, starts, ref, gout = dev(f["shapes"]), dev(f["starts"]), dev(f["ref"]), dev(f["gout"])
    ko, ka = M * L * P * 2, M * L * P
    if binned == "1":
        one = torch.full((N, Lq, ko + ka), float("nan"), device="cuda")
        gv = MSDA.ms_deform_attn_backward_proj(dev(f["value"]), shp, starts, dev(f["loc"]), dev(f["attn"]), gout, one, ko)
        assert gv is not None
        assert_same(gv, f["gv"], "proj grad_value")
        assert_same(one[..., :ko].reshape(f["d_off"].shape), f["d_off"], "proj d(offsets)")
        assert_same(one[..., ko:].reshape(f["d_log"].shape), f["d_log"], "proj d(logits)")
    value, off = dev(f["value"]).requires_grad_(True), dev(f["off"]).requires_grad_(True)
    lg = torch.zeros(N, Lq, M, L * P, device="cuda", requires_grad=True)
    out = _FusedSampleFn.apply(value, shp, starts, off, lg, ref)
    out.backward(gout)
    assert_same(out, f["out"], "out")
    assert_same(value.grad, f["gv"], "grad_value")
    assert_same(off.grad, f["d_off"], "d(offsets)")
    assert_same(lg.grad, f["d_log"], "d(logits)")


# ---- 3. the encoder's state at initialisation, C4 geometry ------------------------------------------------------------------
def either(got, lo, hi, rtol, atol):
    """Elementwise: within tolerance of the low-side or of the high-side evaluation."""
    ok = (np.abs(got - lo) <= atol + rtol * np.abs(lo)) | (np.abs(got - hi) <= atol + rtol * np.abs(hi))
    return ok


def test_encoder_state_at_initialisation(monkeypatch):
    """Levels 22^2 / 44^2 / 88^2, every pixel a query, offsets = the bias MSDeformAttn._reset_parameters sets (zero weight):
    a third of all sampling coordinates sit within rounding of an integer. The float64 reference is evaluated on the fp32
    location bits in the cell below and in the cell above every such coordinate (shift -2e-5 / +2e-5: the threshold
    tests/test_gpu_msda.py uses to EXCLUDE kinks). out, grad_value and grad_attn are continuous across a kink; each grad_loc
    component must be the one-sided derivative of one of the two cells (or zero where the coordinate is at -1 / at the level
    size, in or out by rounding); and the fused and the unfused form, on both backward routes, must pick the same side."""
    from multishiftseg_amd.ms_deform_attn import MSDeformAttn, MSDeformAttnFunction, _FusedSampleFn, _PrepareFn
    from multishiftseg_amd.msdeformattn_encoder import MSDeformAttnTransformerEncoder
    shapes = [(22, 22), (44, 44), (88, 88)]
    shp = np.asarray(shapes, dtype=np.int64)
    starts = R.level_starts(shp)
    S, L, N, D = int(shp.prod(1).sum()), 3, 1, 32
    torch.manual_seed(5)
    bias = MSDeformAttn(256, 3, 8, 4).sampling_offsets.bias.detach().view(1, 1, M, L, P, 2)
    off_h = bias.expand(N, S, M, L, P, 2).contiguous()
    ref_h = MSDeformAttnTransformerEncoder.get_reference_points(torch.from_numpy(shp), torch.ones(N, L, 2), "cpu").contiguous()
    lg_h = 0.1 * torch.randn(N, S, M, L * P)
    value_h, gout_h = torch.randn(N, S, M, D), torch.randn(N, S, M * D)
    shp_t, st_t, ref = dev(shp), dev(starts), ref_h.cuda()

    runs = {}
    for binned in ("1", "0"):
        monkeypatch.setenv("MSS_MSDA_BWD_BINNED", binned)
        value, off, lg = (t.cuda().requires_grad_(True) for t in (value_h, off_h, lg_h))
        loc, attn = _PrepareFn.apply(off, lg, ref, shp_t)
        loc.retain_grad()
        attn.retain_grad()
        out = MSDeformAttnFunction.apply(value, shp_t, st_t, loc, attn, 128)
        out.backward(gout_h.cuda())
        runs["op", binned] = dict(out=host(out), gv=host(value.grad), gl=host(loc.grad), ga=host(attn.grad), d_off=host(off.grad),
                                  loc=loc.detach().cpu().numpy(), attn=attn.detach().cpu().numpy())
        value, off, lg = (t.cuda().requires_grad_(True) for t in (value_h, off_h, lg_h))
        out = _FusedSampleFn.apply(value, shp_t, st_t, off, lg, ref)
        out.backward(gout_h.cuda())
        runs["fused", binned] = dict(out=host(out), gv=host(value.grad), d_off=host(off.grad))

    loc32, attn32 = runs["op", "1"]["loc"], runs["op", "1"]["attn"]
    assert np.array_equal(runs["op", "0"]["loc"], loc32)
    loc64, attn64 = loc32.astype(np.float64), attn32.astype(np.float64)
    p = R.pixel_coords(loc64, shp)
    near = np.abs(p - np.round(p)) < 2e-5
    share = float(near.mean())
    print(f"kink share {share:.4f}, exact integers {float((p == np.round(p)).mean()):.4f}")
    assert share >= 0.3, share

    qs = np.sort(np.random.default_rng(8).choice(S, size=1500, replace=False))
    v64, g64 = value_h.numpy().astype(np.float64), gout_h.numpy().astype(np.float64)
    sub = dict(lo={}, hi={})
    for side, shift in (("lo", -2e-5), ("hi", 2e-5)):
        c = R.cells(loc64[:, qs], shp, shift)
        sub[side]["out"] = R.forward(v64, shp, starts, loc64[:, qs], attn64[:, qs], *c)
        _, sub[side]["gl"], sub[side]["ga"] = R.backward(v64, shp, starts, loc64[:, qs], attn64[:, qs], g64[:, qs], *c, want_value=False)
    want_gv = omsda.backward_sampled(v64, shp, starts, loc64, attn64, g64)[0]
    size = shp[None, None, None, :, None, ::-1].astype(np.float64)
    scale = max(float(np.abs(sub["lo"]["gl"]).max()), float(np.abs(sub["hi"]["gl"]).max()))
    bound = 2e-5 * scale + 1e-3
    ps = p[:, qs]
    at_border = (np.abs(ps + 1) < 2e-5) | (np.abs(ps - size) < 2e-5)
    assert at_border.any() and near[:, qs].mean() >= 0.3

    for (form, binned), r in runs.items():
        tag = f"{form}, MSS_MSDA_BWD_BINNED={binned}"
        bad = ~either(r["out"][:, qs], sub["lo"]["out"], sub["hi"]["out"], **FWD_TOL)
        assert not bad.any(), (tag, "out", int(bad.sum()), np.argwhere(bad)[0])
        np.testing.assert_allclose(r["gv"], want_gv, err_msg=tag, **GRAD_TOL)
        if form != "op":
            continue
        bad = ~either(r["ga"][:, qs], sub["lo"]["ga"], sub["hi"]["ga"], **GRAD_TOL)
        assert not bad.any(), (tag, "grad_attn", int(bad.sum()), np.argwhere(bad)[0])
        gl = r["gl"][:, qs]
        ok = (np.abs(gl - sub["lo"]["gl"]) < bound) | (np.abs(gl - sub["hi"]["gl"]) < bound) | (at_border & (np.abs(gl) < bound))
        assert ok.all(), (tag, "grad_loc", int((~ok).sum()), np.argwhere(~ok)[0], bound)
        # away from kinks the two evaluations coincide and the check above is the ordinary one
        assert np.abs(sub["lo"]["gl"] - sub["hi"]["gl"])[~near[:, qs]].max() < 1e-9

    # forward / backward consistency: d(offsets) x level size = grad_loc; all four runs landed on the same side of every kink
    base = runs["op", "1"]["d_off"] * size
    for key, r in runs.items():
        err = np.abs(r["d_off"] * size - base)
        assert float(err.max()) < bound, (key, float(err.max()), np.unravel_index(err.argmax(), err.shape))
        assert np.abs(r["out"] - runs["op", "1"]["out"]).max() <= 1e-5 * np.abs(runs["op", "1"]["out"]).max(), key


# ---- 4. locations that fail the inside test ---------------------------------------------------------------------------------
BAD_LOCATIONS = [(0, 0, 0, 0, 0, 0, float("nan")), (0, 1, 2, 1, 3, 1, float("inf")), (1, 6, 7, 0, 2, 0, float("-inf")),
                 (1, 3, 4, 1, 0, 1, 3e38), (0, 5, 1, 0, 1, 0, -3e38), (1, 0, 0, 1, 1, 1, 1e30), (0, 0, 0, 0, 1, 1, float("nan")),
                 (1, 6, 7, 1, 3, 0, float("inf"))]


@pytest.mark.parametrize("route", list(ROUTES))
def test_locations_failing_the_inside_test_contribute_nothing(monkeypatch, route):
    """A NaN, infinite or absurd coordinate fails h_im > -1 && w_im > -1 && h_im < H && w_im < W (.cuh:293): the sample adds
    nothing to the output and gets zero gradient, on every forward and backward route. Reference: float64 on the same inputs
    with those samples' weight 0 and location (0.5, 0.5)."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    D, dtype, binned = ROUTES[route]
    monkeypatch.setenv("MSS_MSDA_BWD_BINNED", binned or "1")
    shapes, N, Lq = [(6, 4), (3, 2)], 2, 7
    shp = np.asarray(shapes, dtype=np.int64)
    starts = R.level_starts(shp)
    S, L = int(shp.prod(1).sum()), 2
    rng = np.random.default_rng(13)
    value = rng.standard_normal((N, S, M, D), dtype=np.float32).astype(np.float64)
    loc = rng.random((N, Lq, M, L, P, 2), dtype=np.float32).astype(np.float64)
    attn = rng.random((N, Lq, M, L, P), dtype=np.float32).astype(np.float64)
    gout = rng.standard_normal((N, Lq, M * D), dtype=np.float32).astype(np.float64)
    cl, ca = loc.copy(), attn.copy()
    hit = np.zeros(attn.shape, bool)
    for n, q, m, l, pt, ax, v in BAD_LOCATIONS:
        loc[n, q, m, l, pt, ax] = v
        cl[n, q, m, l, pt] = 0.5
        ca[n, q, m, l, pt] = 0
        hit[n, q, m, l, pt] = True
    c = R.cells(cl, shp)
    want_out = R.forward(value, shp, starts, cl, ca, *c)
    want = list(R.backward(value, shp, starts, cl, ca, gout, *c))
    want[2][hit] = 0
    with np.errstate(over="ignore"):
        args = [dev(value, dtype), dev(shp), dev(starts), dev(loc, dtype), dev(attn, dtype)]
    out = host(MSDA.ms_deform_attn_forward(*args, 2))
    assert np.isfinite(out).all(), np.argwhere(~np.isfinite(out))[0]
    np.testing.assert_allclose(out, want_out, **FWD_TOL)
    if route == "d24_generic":          # forward-only route (its backward is d16's kernel)
        return
    gv, gl, ga = (host(t) for t in MSDA.ms_deform_attn_backward(*args, dev(gout, dtype), 2))
    for a, name in zip((gv, gl, ga), NAMES):
        assert np.isfinite(a).all(), (name, np.argwhere(~np.isfinite(a))[0])
    assert (gl[hit] == 0).all() and (ga[hit] == 0).all()
    np.testing.assert_allclose(gv, want[0], **GRAD_TOL)
    np.testing.assert_allclose(ga, want[2], **GRAD_TOL)
    assert np.abs(gl - want[1]).max() < 2e-5 * np.abs(want[1]).max() + 1e-3
