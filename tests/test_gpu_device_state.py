"""Every launcher asks csrc/mss_device.h what its device allows (DESIGN "per-device state"): occupancy and CU count size the grids of
the persistent GEMM kernels, and a kernel with more than 48 KB of dynamic LDS has its limit raised once per device. Three checks:

* same grid: one product per kernel whose grid comes from the cache -- gemm_nt_kernel on the 128- and the 256-wide tile, the split-bf16
  kernel, gemm_tn_wgrad_kernel -- at the smallest shape mss_conv2d_forward_route / the weight-gradient route sends there, bit for bit
  what the build before the cache wrote (SHA-256 in tests/golden/device_state_parent.json, recorded by tools/device_state_parity.py);
* limit raised once: the three launchers that used to raise the limit before every launch (or once per process) run three times in a
  row, each run checked against the reference of the test that already covers the kernel;
* second device: those three launches, one native GEMM and the TN weight gradient on device 0 and then on device 1 of one process, the
  same bits (skipped on a one-device machine; the per-device logic is then carried by tests/device_cache_check.cpp alone).

Inputs come from numpy's generator on the host, so the recorded digests do not depend on the device or its CU count."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _randn(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32))


# --------------------------------------------------------------------------------------------------------------- the five launches
def gemm(dev, rows, C, Ko, split=False):
    """(route code, y) of one rows x C -> Ko product. Rows repeat a 1024-row block scaled by powers of two (exact), so the 131072-row
    case costs no more host time than the small ones."""
    from multishiftseg_amd import _lib, kernels as K
    from multishiftseg_amd._lib import MssConvArgs, ptr
    base = _randn(rows + C, min(rows, 1024), C).to(dev)
    r = torch.arange(rows, device=dev)
    x = (base[r % 1024] * torch.exp2(-(r // 1024 % 8).float())[:, None]).contiguous()
    kpad = _lib.value("mss_conv2d_kpad", Ko)
    w = torch.zeros(kpad, C, device=dev)
    w[:Ko] = _randn(Ko, Ko, C).to(dev) / C ** 0.5
    y = torch.full((rows, Ko), float("nan"), device=dev)
    a = MssConvArgs()
    a.N, a.H, a.W, a.OH, a.OW = 1, 1, rows, 1, rows
    a.R = a.S = a.stride = a.dil = 1
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
    a.C, a.ldx, a.K, a.Kpad, a.ldy = C, C, Ko, kpad, Ko
    if split:
        planes = K.split_planes(w, kpad, C)
        a.w_split = ptr(planes)
    code = _lib.value("mss_conv2d_forward_route", ctypes.byref(a))
    _lib.call("mss_conv2d_forward_f32", ctypes.byref(a))
    torch.cuda.synchronize()
    return code, y


def wgrad_tn_lds(dev):
    """dw of a 1x1 layer over 300 pixels, 128 -> 128 channels: the TN route, too few jobs for the LDS-free kernel, C no multiple of
    256 -- gemm_tn_wgrad_kernel (wgrad_route.h: WG_TN_LDS, three row splits), the smallest K and C the TN route takes."""
    from multishiftseg_amd import kernels as K
    x, dy = K.Act(_randn(5, 1, 20, 15, 128).to(dev)), K.Act(_randn(6, 1, 20, 15, 128).to(dev))
    return K.conv2d_wgrad(x, dy, 128, 128, 1, 1)


def same_grid_outputs(dev="cuda:0"):
    """name -> output tensor; the route codes are asserted here: 1 = gemm_nt_kernel, 3 = gemm_nt_bf16x3_kernel."""
    out = {}
    with torch.cuda.device(dev):
        # 300 rows x 136 channels: three row tiles, two 128-wide column tiles, the last of each ragged
        code, out["gemm_nt_bn128"] = gemm(dev, 300, 64, 136)
        assert code == 1
        # the 256-wide tile starts at two rounds of 512 tiles (gemm_rounds.h): 1024 row tiles x one column tile
        code, out["gemm_nt_bn256"] = gemm(dev, 131072, 256, 256)
        assert code == 1
        code, out["split_bf16x3"] = gemm(dev, 300, 64, 136, split=True)
        assert code == 3
        out["wgrad_tn_lds"] = wgrad_tn_lds(dev)
        torch.cuda.synchronize()
    return out


def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


ASPP = dict(N=2, H=13, W=5, C=68, d=1, tiles=(4, 4, 4))


def aspp_lds_bytes(N, H, W, C, d, tiles):
    """aspp3_geometry (csrc/winograd.hip) restated: LDS of wino_input_transform_aspp_kernel."""
    Hs, Ws = -(-H // d), -(-W // d)
    cols = Ws
    for m, ts in enumerate(tiles):
        tW = -(-(-(-W // ((m + 1) * d))) // ts)
        cols = max(cols, (m + 1) * ts * tW + m + 1)
    px = (Hs + 1) * (3 + cols)
    return px * ((64 if px * 68 * 4 <= 80 * 1024 else 32) + 4) * 4


def aspp_transform(dev):
    """(got, want): X' of one map for dilations d, 2d, 3d from mss_wino_input_transform_aspp3_f32 and from three calls of
    mss_wino_input_transform_f32, as tests/test_gpu_ops.py::test_aspp_fused_input_transform_is_bitwise_the_three_separate_ones."""
    from multishiftseg_amd import _lib
    from multishiftseg_amd._lib import call, ptr
    n, h, w, c, d, tiles = (ASPP[k] for k in ("N", "H", "W", "C", "d", "tiles"))
    x = _randn(7, n, h, w, c).to(dev)
    want, got = [], []
    for m, ts in enumerate(tiles):
        size = (ts + 2) ** 2 * _lib.value("mss_wino_num_tiles", n, h, w, (m + 1) * d, ts) * c
        want.append(torch.full((size + 64,), float("nan"), device=dev))
        got.append(torch.full((size + 64,), float("nan"), device=dev))
        call("mss_wino_input_transform_f32", ptr(x), c, n, h, w, c, (m + 1) * d, ts, None, None, 0, ptr(want[m]))
    call("mss_wino_input_transform_aspp3_f32", ptr(x), c, n, h, w, c, d, (ctypes.c_int * 3)(*tiles), *[ptr(t) for t in got])
    torch.cuda.synchronize()
    return torch.cat(got), torch.cat(want)


def igemm_bk32(dev):
    """(y, float64 reference): a 3x3 convolution 2048 -> 256 channels on one 9 x 11 image: fwd_route.h gives conv_igemm_kernel its
    128 x 128 x 32 tile (C >= 2048, K <= 256), whose 73,744 bytes of LDS need the raised limit."""
    from multishiftseg_amd import kernels as K
    x, wt = _randn(8, 1, 9, 11, 2048).to(dev), _randn(9, 256, 2048, 3, 3).to(dev) / (2048 * 9) ** 0.5
    y = K.conv2d(K.Act(x), K.pack_weight(wt), dil=2, pad=2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), dilation=2, padding=2).permute(0, 2, 3, 1)
    return y.buf[..., :256].contiguous(), ref


MSDA = dict(value=_randn(10, 1, 1, 1, 32).numpy(), shapes=np.array([(1, 1)], dtype=np.int64), starts=np.zeros(1, dtype=np.int64),
            loc=np.array([0.4, 0.7], dtype=np.float32).reshape(1, 1, 1, 1, 1, 2), attn=np.ones((1, 1, 1, 1, 1), dtype=np.float32),
            gout=_randn(11, 1, 1, 32).numpy())


def msda_binned_backward(dev):
    """[grad_value, grad_loc, grad_attn] of the binned backward at the smallest shape it takes: one image, one query, one head of 32
    channels (the only head dimension it has), one level of 1 x 1 cells, one point."""
    from multishiftseg_amd import _lib, MultiScaleDeformableAttention as M
    t = {k: torch.from_numpy(v).to(dev) for k, v in MSDA.items()}
    assert _lib.value("mss_msda_backward_workspace_bytes", M.host_shapes(t["shapes"]), 1, 1, 32, 1, 1, 1) > 0      # the binned path takes it
    return M.ms_deform_attn_backward(t["value"], t["shapes"], t["starts"], t["loc"], t["attn"], t["gout"], 1)


# --------------------------------------------------------------------------------------------------------------------------- tests
def test_same_grid_as_the_parent_build():
    with open(os.path.join(GOLDEN, "device_state_parent.json")) as f:
        parent = json.load(f)
    ours = {name: digest(t) for name, t in same_grid_outputs().items()}
    assert ours == parent


def test_aspp_transform_limit_raised_once_and_three_launches_agree():
    """ASPP above: (Hs + 1) * WsT = 14 * (3 + 15) = 252 staged pixels (the third job's last tap reaches column 3 * 4 + 3 = 15) of
    64 + 4 floats = 68,544 bytes > 65,536; one row less (H = 12: 13 * 18 = 234 pixels, 63,648 bytes) stays below."""
    assert aspp_lds_bytes(**ASPP) == 68544 and aspp_lds_bytes(**dict(ASPP, H=ASPP["H"] - 1)) <= 65536
    for _ in range(3):
        got, want = aspp_transform("cuda:0")
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 3 * 64      # the canaries alone
        assert torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


def test_igemm_128x128x32_limit_raised_once_and_three_launches_agree():
    """Bound: tests/test_gpu_ops.py::test_conv_vs_oracle's rtol = atol = 1e-4 on outputs of unit scale (tests/test_gpu_fwd_route.py, code 0)."""
    for _ in range(3):
        y, ref = igemm_bk32("cuda:0")
        assert ref.abs().max().item() > 0.1 and bool(((y.double() - ref).abs() <= 1e-4 + 1e-4 * ref.abs()).all())


def test_msda_binned_backward_limit_raised_once_and_three_launches_agree():
    """Bounds: tests/test_gpu_msda.py::test_backward_formulations_vs_oracle."""
    from oracle import msda as omsda
    want = omsda.backward(MSDA["value"], MSDA["shapes"], MSDA["starts"], MSDA["loc"], MSDA["attn"], MSDA["gout"])
    assert np.abs(want[0]).max() > 0.01
    for _ in range(3):
        got = msda_binned_backward("cuda:0")
        for g, w, atol in zip(got, want, (1e-4, 3e-3, 1e-4)):
            np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-3, atol=atol)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="one device: tests/device_cache_check.cpp carries the per-device logic alone")
def test_second_device_same_bits():
    def everything(dev):
        with torch.cuda.device(dev):
            out = dict(gemm=gemm(dev, 300, 64, 136)[1], wgrad=wgrad_tn_lds(dev), aspp=aspp_transform(dev)[0].nan_to_num(0.0), igemm=igemm_bk32(dev)[0])
            out.update({f"msda{i}": g for i, g in enumerate(msda_binned_backward(dev))})
            torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}
    first, second = everything("cuda:0"), everything("cuda:1")
    for name in first:
        assert torch.equal(first[name], second[name]), name
