"""The float64 Winograd restatement (tests/ref_winograd.py) validated before any kernel is compared with it: its whole chains,
geometry included, equal a direct float64 convolution and float64 autograd; and the 9-digit literals of WinoMat<4> / WinoMat<6> in
csrc/winograd.hip are the ones the exact rational construction prints. Needs no GPU."""
import os
import re

import pytest
import torch

import ref_winograd as R
from conftest import ROOT

# (N, H, W): ragged for every m * d of the grid below; fewer sub-grid rows than tiles have rows; one pixel row (smaller than any tile)
SIZES = [(2, 13, 11), (1, 7, 20), (1, 1, 3)]
C_IN, K_OUT = 3, 4


def _case(N, H, W, dil):
    g = torch.Generator().manual_seed(100 * H + 10 * W + dil)
    x = torch.randn((N, C_IN, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((K_OUT, C_IN, 3, 3), generator=g, dtype=torch.float64)
    dy = torch.randn((N, K_OUT, H, W), generator=g, dtype=torch.float64)
    return x, w, dy


@pytest.mark.parametrize("N,H,W", SIZES)
@pytest.mark.parametrize("dil", [1, 2, 3])
@pytest.mark.parametrize("tile", [2, 4, 6])
def test_float64_chains_equal_direct_convolution_and_autograd(tile, dil, N, H, W):
    x, w, dy = _case(N, H, W, dil)
    w.requires_grad_(True)
    ref = torch.nn.functional.conv2d(x, w, dilation=dil, padding=dil)
    ref.backward(dy)
    got = R.conv_chain(x, w.detach(), dil, tile, torch.float64)
    assert got.shape == ref.shape and not torch.isnan(got).any()                    # every pixel belongs to exactly one tile
    assert float((got - ref.detach()).abs().max()) <= 1e-12 * float(ref.detach().abs().max())
    gw = R.wgrad_chain(x, dy, dil, tile, torch.float64)
    assert gw.shape == w.grad.shape
    assert float((gw - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())


@pytest.mark.parametrize("tile", [2, 4, 6])
def test_float64_chain_with_prologue_and_residual(tile):
    """The padding is zero after the prologue (a positive shift must not leak into it), and the residual is added once."""
    x, w, res = _case(2, 9, 14, 2)
    g = torch.Generator().manual_seed(5)
    scale = torch.randn(C_IN, generator=g, dtype=torch.float64)
    shift = torch.rand(C_IN, generator=g, dtype=torch.float64) + 0.25
    act = torch.relu(x * scale[None, :, None, None] + shift[None, :, None, None])
    ref = torch.nn.functional.conv2d(act, w, dilation=2, padding=2) + res
    got = R.conv_chain(x, w, 2, tile, torch.float64, scale=scale, shift=shift, relu=True, res=res)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("tile", [4, 6])
@pytest.mark.parametrize("which", ["Bt", "G", "At"])
def test_kernel_literals_are_the_rational_construction(tile, which):
    with open(os.path.join(ROOT, "multishiftseg_amd", "csrc", "winograd.hip")) as f:
        src = re.sub(r"\s+", "", f.read())
    at, g, bt = R.rational_matrices(tile)
    want = re.sub(r"\s+", "", R.wino_matrices.c_init(which, {"Bt": bt, "G": g, "At": at}[which]))
    assert src.count(want) == 1, want


def test_magnitude_companions_dominate():
    """|L X R| <= |L| |X| |R| elementwise and in the same layout: a sanity check of the expressions the GPU bounds are stated in."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn((1, 9, 10, 4), generator=g, dtype=torch.float64)
    w = torch.randn((4, 4, 3, 3), generator=g, dtype=torch.float64)
    for tile in (2, 4, 6):
        P = tile + 2
        T = R.geom(1, 9, 10, 2, tile)["T"]
        yt = torch.randn((P * P, T, 4), generator=g, dtype=torch.float64)
        du = torch.randn((P * P, 8, 8), generator=g, dtype=torch.float64)
        for val, mag in ((R.input_transform(x, 2, tile), R.input_transform_mag(x, 2, tile)),
                         (R.pack_weights(w, tile, 8, 8), R.pack_weights_mag(w, tile, 8, 8)),
                         (R.output_transform(yt, 1, 9, 10, 2, tile), R.output_transform_mag(yt, 1, 9, 10, 2, tile)),
                         (R.grad_output_transform(x, 2, tile), R.grad_output_transform_mag(x, 2, tile)),
                         (R.weight_grad_transform(du, 4, 4, tile), R.weight_grad_transform_mag(du, 4, 4, tile))):
            assert val.shape == mag.shape and bool((val.abs() <= mag * (1 + 1e-12)).all())
