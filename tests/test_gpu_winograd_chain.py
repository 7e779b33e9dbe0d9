"""The whole Winograd convolutions (forward with prologue and residual, data gradient through the flipped filter, weight gradient)
held to float64 at a floor measured on the spot: the float32 run of tests/ref_winograd.py's own chain -- the same three steps, plain
torch on the CPU -- on the same inputs. max|hip - float64| <= 8 * max|chain_float32 - float64|: the reference's float32 error sets
the bar, never the kernel's; 8 x is the project's margin for a different but equally sound summation order (tests/test_gpu_matcher.py).
The fixed-tolerance op tests in tests/test_gpu_ops.py stay as they are; this file adds the tight bar beside them. Floors, deviations
and ratios are printed and the worst ratios appended to winograd_kernels.json in the report directory."""
import functools
import json
import os

import pytest
import torch

import ref_winograd as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

# (N, H, W, C, K, dil)
SHAPES = [(2, 13, 11, 32, 36, 1), (1, 14, 19, 48, 100, 2), (1, 30, 41, 64, 64, 12)]


@pytest.fixture(scope="module")
def K():
    from multishiftseg_amd import kernels
    return kernels


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


def _bchw(v):
    return v[None, :, None, None]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs of shape i (float32, CPU) and the float64 references: direct convolution and autograd. Shared, never modified."""
    N, H, W, C, Kc, dil = SHAPES[i]
    g = torch.Generator().manual_seed(77 + i)
    x = torch.randn((N, C, H, W), generator=g)
    w = torch.randn((Kc, C, 3, 3), generator=g) / (9 * C) ** 0.5
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    scale = (torch.rand(C, generator=g) + 0.5) * sign
    shift = torch.rand(C, generator=g) + 0.25
    res = torch.randn((N, Kc, H, W), generator=g)
    dy = torch.randn((N, Kc, H, W), generator=g)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    act = torch.relu(xd * _bchw(scale.double()) + _bchw(shift.double()))
    y0 = torch.nn.functional.conv2d(act, wd, dilation=dil, padding=dil)
    dw, = torch.autograd.grad(y0, wd, dy.double())                       # weight gradient behind the prologue
    dx, = torch.autograd.grad(torch.nn.functional.conv2d(xd, wd, dilation=dil, padding=dil), xd, dy.double())   # plain data gradient
    # the data gradient as a convolution of dy with the flipped filter; its channel count padded to the 16 the packed filter needs
    Kp = -(-Kc // 16) * 16
    dyp = torch.zeros((N, Kp, H, W))
    dyp[:, :Kc] = dy
    wp = torch.zeros((Kp, C, 3, 3))
    wp[:Kc] = w
    return dict(x=x, w=w, scale=scale, shift=shift, res=res, dy=dy, dyp=dyp, wp=wp, y=(y0 + res.double()).detach(), dw=dw.detach(),
                dx=dx.detach())


@functools.lru_cache(maxsize=None)
def _floors(i, tile):
    """max|chain_float32 - float64| of the three chains."""
    c, dil = _case(i), SHAPES[i][5]
    y32 = R.conv_chain(c["x"], c["w"], dil, tile, torch.float32, scale=c["scale"], shift=c["shift"], relu=True, res=c["res"])
    dx32 = R.conv_chain(c["dyp"], c["wp"].flip(2, 3).transpose(0, 1), dil, tile, torch.float32)
    dw32 = R.wgrad_chain(c["x"], c["dy"], dil, tile, torch.float32, scale=c["scale"], shift=c["shift"], relu=True)
    assert y32.dtype == dx32.dtype == dw32.dtype == torch.float32
    return dict(y=float((y32.double() - c["y"]).abs().max()), dx=float((dx32.double() - c["dx"]).abs().max()),
                dw=float((dw32.double() - c["dw"]).abs().max()))


def _hold(report, what, key, got, ref, floor):
    dev = float((got.double().cpu() - ref).abs().max())
    bound = 8.0 * floor
    print(f"{what}: float32 chain floor {floor:.3e}, |hip - float64| {dev:.3e}, bound {bound:.3e}, max|ref| {float(ref.abs().max()):.3e}")
    assert floor > 0.0
    report[key] = max(report.get(key, 0.0), dev / bound)
    assert dev <= bound, (what, dev, bound)


@pytest.mark.parametrize("i", range(len(SHAPES)))
@pytest.mark.parametrize("tile", [2, 4, 6])
def test_forward_with_prologue_and_residual(K, tile, i, gemm_route, report):
    c, dil = _case(i), SHAPES[i][5]
    y = K.conv2d_winograd(K.Act.from_nchw(c["x"].cuda()), K.pack_weight_wino(c["w"].cuda(), tile=tile), dil=dil,
                          in_affine=(c["scale"].cuda(), c["shift"].cuda()), in_relu=True, res=K.Act.from_nchw(c["res"].cuda()))
    _hold(report, f"forward F({tile}x{tile}) {SHAPES[i]} {gemm_route}", "chain_forward", y.nchw(), c["y"], _floors(i, tile)["y"])


@pytest.mark.parametrize("i", range(len(SHAPES)))
@pytest.mark.parametrize("tile", [2, 4, 6])
def test_data_gradient_through_flipped_filter(K, tile, i, gemm_route, report):
    c, dil = _case(i), SHAPES[i][5]
    dx = K.conv2d_winograd(K.Act.from_nchw(c["dyp"].cuda()), K.pack_weight_wino(c["wp"].cuda(), flip=True, tile=tile), dil=dil)
    _hold(report, f"data gradient F({tile}x{tile}) {SHAPES[i]} {gemm_route}", "chain_data_gradient", dx.nchw(), c["dx"], _floors(i, tile)["dx"])


@pytest.mark.parametrize("i", range(len(SHAPES)))
@pytest.mark.parametrize("tile", [2, 4, 6])
def test_weight_gradient(K, tile, i, gemm_route, report):
    c = _case(i)
    N, H, W, C, Kc, dil = SHAPES[i]
    dw = K.conv2d_wgrad_winograd(K.Act.from_nchw(c["x"].cuda()), K.Act.from_nchw(c["dy"].cuda()), Kc, C, dil=dil,
                                 in_affine=(c["scale"].cuda(), c["shift"].cuda()), in_relu=True, tile=tile)
    _hold(report, f"weight gradient F({tile}x{tile}) {SHAPES[i]} {gemm_route}", "chain_weight_gradient", dw, c["dw"], _floors(i, tile)["dw"])
