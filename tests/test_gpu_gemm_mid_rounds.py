"""Single-position GEMMs between one and two rounds of wide tiles (csrc/gemm_rounds.h): by default 512 wide tiles and
then the rest as narrow tiles in a second launch, with MSS_GEMM_TAIL=0 all narrow tiles as before. Every output element is the same
sum in the same order on either tile, so the two results are equal bit for bit -- compared into NaN-filled outputs, so an element no
launch wrote shows -- and a sample of rows is checked against float64 with the bound of
test_gpu_ops.test_gemm_hybrid_last_round_is_bitwise_the_wide_result."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T,C,Ko,affine", [
    (4603, 256, 4096, False),        # 36 x 16 = 576 wide tiles: 512 + 64, partial last row tile
    (7168, 256, 4096, True),         # 56 x 16 = 896 = 512 + 384, the train step's tiling with a short reduction; BatchNorm + ReLU prologue
])
def test_mid_rounds_hybrid_is_bitwise_the_all_narrow_result(monkeypatch, T, C, Ko, affine):
    from multishiftseg_amd import _lib
    from multishiftseg_amd._lib import MssConvArgs, call, ptr
    torch.manual_seed(T + C)
    x = torch.randn(T, C, device="cuda")
    kpad = _lib.value("mss_conv2d_kpad", Ko)
    w = torch.zeros(kpad, C, device="cuda")
    w[:Ko] = torch.randn(Ko, C, device="cuda") / C ** 0.5
    sc = torch.rand(C, device="cuda") + 0.5
    sh = torch.randn(C, device="cuda") * 0.1
    outs = {}
    for tail in ("0", None):
        if tail is None:
            monkeypatch.delenv("MSS_GEMM_TAIL", raising=False)
        else:
            monkeypatch.setenv("MSS_GEMM_TAIL", tail)
        y = torch.full((T, Ko), float("nan"), device="cuda")
        a = MssConvArgs()
        a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
        a.N, a.H, a.W, a.C, a.ldx = 1, 1, T, C, C
        a.OH, a.OW, a.K, a.Kpad, a.ldy = 1, T, Ko, kpad, Ko
        a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
        if affine:
            a.in_scale, a.in_shift, a.in_relu = ptr(sc), ptr(sh), 1
        call("mss_conv2d_forward_f32", ctypes.byref(a))
        outs[tail] = y
    assert not torch.isnan(outs[None]).any() and not torch.isnan(outs["0"]).any()
    assert torch.equal(outs["0"], outs[None])
    rows = torch.randint(0, T, (64,), device="cuda")
    rows[0], rows[1] = 0, T - 1
    xin = x[rows].double()
    if affine:
        xin = torch.relu(xin * sc.double() + sh.double())
    want = xin @ w[:Ko].double().t()
    err = (outs[None][rows].double() - want).abs().max().item()
    print(f"T {T}: max |y - float64| over 64 rows {err:.3e}")
    assert err < 1e-4
