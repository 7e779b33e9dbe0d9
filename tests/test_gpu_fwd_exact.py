"""Every forward conv / GEMM kernel behind mss_conv2d_forward_f32 alone, exactly, at its tile and plan edges: each row of
tests/fwd_cases.py through ONE raw mss_conv2d_forward_f32 call (and through kernels.conv2d where the wrapper can express it) against
float64, with EQUALITY -- the data lie on lattices on which fp32 is exact in any summation order (tests/test_fwd_exact_cpu.py checks
that condition, the reference and the expected plans without a GPU; on the split route the reference is the sum of the six products
the kernel keeps).

Every case: x, res and the affine vectors live inside larger NaN-filled buffers (guard rows before, behind and between batch entries,
NaN in the channels between C / K and the row pitch, NaN behind each image's extent in the per-image forms); y and the statistics
start NaN-filled with NaN behind them; the weights go through the library's own pack and split functions; the route code (and for
the split kernels the matrix instruction) is asserted around the launch; every element of the output window equals the reference,
everything outside it is still NaN, and a second run gives the same bits. One line per case: name, plan, number of unequal elements."""
import ctypes

import pytest
import torch

import fwd_cases as fc
from multishiftseg_amd import _lib
from multishiftseg_amd import kernels as K
from multishiftseg_amd._lib import call

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = fc.GUARD
TAIL = 64           # NaN floats behind the statistics


def _rows(c, per_entry):
    """A NaN-filled buffer of pixel rows: GUARD rows, then per batch entry `per_entry` rows (+ GUARD between entries), GUARD rows."""
    return GUARD + c.nb * (per_entry + (GUARD if c.batch > 1 else 0)) + GUARD


def _embed(c, data, ld, c0):
    """data [nb][rows][width] (CPU) -> (NaN-filled device buffer [all rows][ld] with the data at channel c0, view of the entries
    [nb][rows (+ GUARD)][ld], address of the first data element)."""
    nb, rows, width = data.shape
    buf = torch.full((_rows(c, rows), ld), NAN, device="cuda")
    body = buf[GUARD:buf.shape[0] - GUARD].view(nb, -1, ld)
    body[:, :rows, c0:c0 + width] = data.cuda()
    return buf, body, buf.data_ptr() + 4 * (GUARD * ld + c0)


def _vector(v):
    """A per-channel vector ([C], [N][C] or [K]) between NaN guards: the view of the values (16-byte aligned)."""
    buf = torch.full((v.numel() + 16,), NAN, device="cuda")
    view = buf[8:8 + v.numel()].view(v.shape)
    view.copy_(v)
    return view


def _weights(c, w):
    """w [nw][K][C][R][R] (CPU) -> (packed [nw][taps][Kpad][C] by mss_conv2d_pack_weights_f32, split planes or None)."""
    taps = c.R * c.R
    wd = w.cuda().contiguous()
    packed = torch.zeros((c.nw, taps, c.Kpad, c.C), device="cuda")
    for i in range(c.nw):
        call("mss_conv2d_pack_weights_f32", wd[i].data_ptr(), packed[i].data_ptr(), c.K, c.C, c.R, c.R, c.Kpad, c.C, 0, None, 0, 0)
    planes = None
    if c.split:
        entries = taps if taps > 1 else c.nw
        nbytes = _lib.value("mss_gemm_split_weights_bytes", entries, c.Kpad, c.C)
        assert nbytes == entries * c.Kpad * c.C * 6
        planes = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
        if taps > 1:
            call("mss_conv_split_weights_bf16x3", packed.data_ptr(), planes.data_ptr(), taps, c.Kpad, c.C)
        else:
            call("mss_gemm_split_weights_bf16x3", packed.data_ptr(), planes.data_ptr(), c.nw, c.Kpad, c.C, c.Kpad * c.C)
    return packed, planes


def launch_twice(c, ops):
    """The case's operands on the device and two raw calls into fresh NaN-filled outputs: (the two (y buffer, view of its entries,
    statistics), the views of x's and res's entries, the vectors). The environment switches are the caller's."""
    xin = ops["x"].clone().view(c.nb, c.N, -1, c.C)
    for b, per_image in enumerate(c.extents()):                  # x of an image exists up to its extent only
        for n, ext in enumerate(per_image):
            xin[b, n, :, ext:] = NAN
    xbuf, xbody, xptr = _embed(c, xin.view(c.nb, -1, c.C), c.ldx, c.x_c0)
    resbuf = resbody = resptr = None
    if c.res:
        resbuf, resbody, resptr = _embed(c, ops["res"], c.ldy, c.y_c0)
    vec = {k: (_vector(ops[k]) if ops[k] is not None else None) for k in ("scale", "shift", "out_scale", "out_shift")}
    packed, planes = _weights(c, ops["w"])
    steps = torch.tensor(c.k_steps, dtype=torch.int32, device="cuda") if c.k_steps else None
    groups = -(-c.M // 64)
    code = fc.CODES[c.expect["kernel"]]
    outs = []
    for _ in range(2):
        ybuf = torch.full((_rows(c, c.M), c.ldy), NAN, device="cuda")
        ybody = ybuf[GUARD:ybuf.shape[0] - GUARD].view(c.nb, -1, c.ldy)
        st = torch.full((groups * 2 * c.K + TAIL,), NAN, device="cuda") if c.stats else None

        def addr(t):
            return None if t is None else t.data_ptr()
        a = fc.conv_args(c, xptr, packed.data_ptr(), ybuf.data_ptr() + 4 * (GUARD * c.ldy + c.y_c0), addr(vec["scale"]), addr(vec["shift"]),
                         addr(vec["out_scale"]), addr(vec["out_shift"]), resptr, addr(st), addr(planes), addr(steps))
        assert _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) == code, c.name
        call("mss_conv2d_forward_f32", ctypes.byref(a))
        torch.cuda.synchronize()
        if c.split:
            assert _lib.value("mss_gemm_split_last_mfma") == c.expect["mfma"], c.name
        outs.append((ybuf, ybody, st))
    return outs, xbody, resbody, vec


@pytest.mark.parametrize("c", fc.CASES, ids=lambda c: c.name)
def test_forward_equals_float64(c, monkeypatch):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    ops = fc.operands(c)
    ref, ref_stats = fc.reference(c, ops, "cpu" if c.ref == "cpu" else "cuda")
    ref = ref.cuda()
    assert torch.equal(ref, (ref * 2.0 ** 20).round() / 2.0 ** 20)          # the reference itself lies on the lattice (granule 1/4, or 2^-19 at the least)
    outs, xbody, resbody, vec = launch_twice(c, ops)
    groups = -(-c.M // 64)
    ybuf, ybody, st = outs[0]
    got = ybody[:, :c.M, c.y_c0:c.y_c0 + c.K]
    unequal = int((got.double() != ref).sum())                   # (a NaN is unequal to everything)
    stats_unequal = 0
    if c.stats:
        stats_unequal = int((st[:groups * 2 * c.K].view(groups, 2, c.K).double() != ref_stats.cuda()).sum())
    p = c.expect
    print(f"{c.name}: {p['kernel']} {p['BM']}x{p['BN']}x{p['BK']} variant {p['variant']} affine {p['affine']} per_sample {p['per_sample']} mfma {p['mfma']}"
          f" mode {p['mode']} full {p['full']} rem {p['rem']} tiles {p['mtiles']}x{p['ntiles']} [{c.data}]: {unequal} unequal of {got.numel()}"
          + (f", statistics {stats_unequal} unequal of {groups * 2 * c.K}" if c.stats else ""))
    assert unequal == 0 and stats_unequal == 0
    assert torch.equal(got.double(), ref)
    outside = torch.ones_like(ybuf, dtype=torch.bool)
    outside[GUARD:ybuf.shape[0] - GUARD].view(c.nb, -1, c.ldy)[:, :c.M, c.y_c0:c.y_c0 + c.K] = False
    assert bool(torch.isnan(ybuf[outside]).all())                # guard rows, the rows between entries, the columns around the window
    if c.stats:
        assert bool(torch.isnan(st[groups * 2 * c.K:]).all())
        assert torch.equal(st.view(torch.int32), outs[1][2].view(torch.int32))
    assert torch.equal(ybuf.view(torch.int32), outs[1][0].view(torch.int32))                # the same bits on a second run
    if c.wrapper:
        K.set_gemm_route("bf16x3" if c.split else "native")
        try:
            pw = K.pack_weight(ops["w"][0].cuda())
            xa = K.Act(xbody[0, :c.N * c.H * c.W].view(c.N, c.H, c.W, c.ldx), c.C, c.x_c0)
            ybuf2 = torch.full((c.N, c.OH, c.OW, c.ldy), NAN, device="cuda")
            out = K.conv2d(xa, pw, c.stride, c.dil, c.pad, in_affine=(vec["scale"], vec["shift"]) if c.affine else None, in_relu=bool(c.affine),
                           out_affine=(vec["out_scale"], vec["out_shift"]) if c.out_affine else None, out_relu=c.out_relu,
                           res=K.Act(resbody[0, :c.M].view(c.N, c.OH, c.OW, c.ldy), c.K, c.y_c0) if c.res else None,
                           out=K.Act(ybuf2, c.K, c.y_c0), want_stats=c.stats, res_mask=c.res == "mask")
        finally:
            K.set_gemm_route(None)
        assert torch.equal(ybuf2.view(-1, c.ldy).view(torch.int32), ybody[0, :c.M].view(torch.int32))
        if c.stats:
            assert torch.equal(out.stats.double(), ref_stats.cuda())
