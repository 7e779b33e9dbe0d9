"""Every weight-gradient kernel alone, exactly, at its plan edges: each row of tests/wgrad_cases.py through a raw
mss_conv2d_wgrad_f32 call (and through kernels.conv2d_wgrad where the wrapper can express it) against float64, with EQUALITY -- the
data are small integers, so fp32 is exact in any summation order (tests/test_wgrad_exact_cpu.py checks that condition, the
reference and the expected plans without a GPU).

Every case: dwp and the scratch start NaN-filled with NaN behind them; x, dy and the affine vectors live inside larger NaN-filled
buffers (guard rows before and behind, between the positions of a batched case, NaN in the channels between C / K and the row
pitch); the plan (kernel, splits, reduce group) is asserted through mss_conv2d_wgrad_plan with the real pointers BEFORE the launch;
the result equals the reference in every element, padding rows and columns included as exact zeros, and is identical on a second
run. One line per case: name, kernel, splits, reduce group, number of unequal elements."""
import ctypes

import pytest
import torch

import ref_wgrad
import wgrad_cases as wc
from multishiftseg_amd import _lib
from multishiftseg_amd import kernels as K
from multishiftseg_amd._lib import call

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 3           # NaN rows before, behind and between
TAIL = 64           # NaN floats behind dwp and the scratch


def _embed(data, ld, c0, gap=0):
    """data [rows][width] or [P][T][width] (CPU) -> (NaN-filled device buffer of rows of `ld` floats with the data at channel c0,
    the view of the buffer's data rows [rows or P * (T + gap)][ld], the address of the first data element)."""
    if data.dim() == 3:
        P, T, width = data.shape
        body_rows = P * (T + gap)
    else:
        body_rows, width = data.shape
    buf = torch.full((GUARD + body_rows + GUARD, ld), NAN, device="cuda")
    body = buf[GUARD:GUARD + body_rows]
    if data.dim() == 3:
        body.view(P, T + gap, ld)[:, :T, c0:c0 + width] = data.cuda()
    else:
        body[:, c0:c0 + width] = data.cuda()
    return buf, body, buf.data_ptr() + 4 * (GUARD * ld + c0)


def _vector(v):
    """A scale / shift vector ([C] or [N][C]) between NaN guards: (buffer, view of the values)."""
    buf = torch.full((v.numel() + 2 * 8,), NAN, device="cuda")
    view = buf[8:8 + v.numel()].view(v.shape)
    view.copy_(v)
    return buf, view


def _reference(c, x, dy, scale, shift):
    """float64 [positions][Kpad][Cp] on the device, and the mask of elements the call must leave unwritten (per-image form) or None."""
    if c.ref == "cpu":
        return ref_wgrad.wgrad(x, dy, c.R, c.R, c.stride, c.dil, c.pad, scale, shift, c.relu, c.Kpad, c.Cp).cuda(), None
    xd, dyd = x.cuda().double(), dy.cuda().double()
    if not c.batch:                       # 1x1 / stride 1: one matrix product
        a = xd.view(-1, c.C)
        if scale is not None:
            a = a * scale.cuda().double() + shift.cuda().double()
        if c.relu:
            a = torch.relu(a)
        ref = torch.zeros((1, c.Kpad, c.Cp), dtype=torch.float64, device="cuda")
        ref[0, :c.K, :c.C] = dyd.view(-1, c.K).t() @ a
        return ref, None
    ref = torch.zeros((c.batch, c.Kpad, c.Cp), dtype=torch.float64, device="cuda")
    for p0 in range(0, c.batch, 16):
        ref[p0:p0 + 16, :c.K, :c.C] = torch.einsum("ptk,ptc->pkc", dyd[p0:p0 + 16], xd[p0:p0 + 16])
    if not c.k_steps:
        return ref, None
    # per-image form: entry b holds image b % n; columns from its extent on are exact zeros up to the end of their tile, and the
    # tiles behind stay unwritten
    unwritten = torch.zeros(ref.shape, dtype=torch.bool, device="cuda")
    n = len(c.k_steps)
    for i, ks in enumerate(c.k_steps):
        ext = 16 * (c.k_base + ks)
        done = -(-ext // 128) * 128
        ref[i::n, :, ext:] = 0.0
        unwritten[i::n, :, done:] = True
    return ref, unwritten


@pytest.mark.parametrize("c", wc.CASES, ids=lambda c: c.name)
def test_wgrad_equals_float64(c, monkeypatch):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    x, dy, scale, shift = wc.operands(c)
    if c.k_steps:                         # x of an entry exists up to its image's extent only
        n = len(c.k_steps)
        for i, ks in enumerate(c.k_steps):
            x[i::n, :, 16 * (c.k_base + ks):] = 0.0
    ref, unwritten = _reference(c, x, dy, scale, shift)
    gap = GUARD if c.batch else 0
    xin = x if c.batch else x.view(-1, c.C)
    if c.k_steps:
        xin = x.clone()
        for i, ks in enumerate(c.k_steps):
            xin[i::len(c.k_steps), :, 16 * (c.k_base + ks):] = NAN
    xbuf, xbody, xptr = _embed(xin, c.ldx, c.x_c0, gap)
    dybuf, dybody, dyptr = _embed(dy if c.batch else dy.view(-1, c.K), c.lddy, c.dy_c0, gap)
    sc = sh = (None, None)
    if c.affine:
        sc, sh = _vector(scale), _vector(shift)
    steps = torch.tensor(c.k_steps, dtype=torch.int32, device="cuda") if c.k_steps else None
    a = wc.conv_args(c, xptr, sc[1].data_ptr() if c.affine else None, sh[1].data_ptr() if c.affine else None,
                     steps.data_ptr() if c.k_steps else None, gap)
    ws_bytes = _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a), c.Cp)
    size = ref.numel()
    outs = []
    for _ in range(2):
        dwp = torch.full((size + TAIL,), NAN, device="cuda")
        ws = torch.full((ws_bytes // 4 + TAIL,), NAN, device="cuda")
        got, pl = wc.answered_plan(c, a, dyptr, dwp.data_ptr(), ws_bytes)
        assert got == c.expect, (c.name, got)
        call("mss_conv2d_wgrad_f32", ctypes.byref(a), dyptr, c.lddy, dwp.data_ptr(), c.Cp, ws.data_ptr() if ws_bytes else None, ws_bytes)
        assert torch.isnan(dwp[size:]).all() and torch.isnan(ws[ws_bytes // 4:]).all()
        outs.append(dwp[:size].view(ref.shape))
    res = outs[0].double()
    wrong = res != ref                                              # (a NaN is unequal to everything)
    if unwritten is not None:
        wrong = (wrong & ~unwritten) | (~torch.isnan(outs[0]) & unwritten)
    unequal = int(wrong.sum())
    print(f"{c.name}: {got['kernel']} splits {got['splits']} reduce group {got['reduce_group']}"
          + (f" parts {got['parts']}" if "parts" in got else "") + f": {unequal} unequal of {size}")
    assert unequal == 0
    if unwritten is None:
        assert torch.equal(res, ref)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))                # the same bits on a second run
    if c.wrapper:
        xa = K.Act(xbody.view(c.N, c.H, c.W, c.ldx), c.C, c.x_c0)
        dya = K.Act(dybody.view(c.N, c.OH, c.OW, c.lddy), c.K, c.dy_c0)
        grad = K.conv2d_wgrad(xa, dya, c.K, c.C, c.R, c.R, c.stride, c.dil, c.pad, in_affine=(sc[1], sh[1]) if c.affine else None, in_relu=c.relu)
        assert torch.equal(grad.double(), ref_wgrad.unpack(ref, c.K, c.C, c.R, c.R))
