"""CPU: the stem form of mss_conv2d_wgrad_f32 (csrc/stem7_wgrad.hip) as the host sees it -- what the plan query answers and refuses
(fake aligned addresses, no device), what hipcc makes of its kernels for gfx950, and the bookkeeping of ResNet.set_trainable(stem=True).
STEM_SIZES is shared with tests/test_gpu_stem7_wgrad.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from multishiftseg_amd import _lib

TH, TW, MAX_SPLITS = 4, 16, 1024                 # csrc/wgrad_route.h: WG_STEM7_TH / _TW / _MAX_SPLITS
# (N, H, W): the sizes of the issue; MULTI has 3 x 3 = 9 tiles = 4 splits of 2 tiles + 1 of one; LONG has 32 x 65 = 2080 tiles, more
# than 2 x 1024, so 3 tiles per split (and one in the last)
MULTI = (1, 23, 70)
LONG = (1, 255, 2079)
STEM_SIZES = ((1, 7, 9), (2, 9, 13), (1, 70, 100), (2, 64, 96), MULTI)
FAKE = 0x7000000


def stem_args(n, h, w, pool=False, **over):
    a = _lib.MssConvArgs()
    a.x = ctypes.c_void_p(FAKE)
    a.N, a.H, a.W, a.C, a.ldx = n, h, w, 4, 4
    a.OH, a.OW, a.K, a.Kpad = (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64, 64
    a.R, a.S, a.stride, a.dil, a.pad = 7, 7, 2, 1, 3
    if pool:
        a.res, a.ldres, a.res_mask = ctypes.c_void_p(FAKE + 0x100000), 64, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def ask(a, lddy=64, Cp=4, ws_bytes=0):
    out = _lib.MssWgradPlan()
    rc = _lib.value("mss_conv2d_wgrad_plan", ctypes.byref(a), ctypes.c_void_p(FAKE + 0x200000), lddy, ctypes.c_void_p(FAKE + 0x300000), Cp, ws_bytes, 0,
                    ctypes.byref(out))
    return rc, out


def expected_plan(n, h, w):
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    tiles = n * -(-oh // TH) * -(-ow // TW)
    per = max(2, -(-tiles // MAX_SPLITS))
    splits = -(-tiles // per)
    return tiles, per, splits


@pytest.mark.parametrize("size", STEM_SIZES + (LONG, (1, 1024, 2048)), ids=str)
@pytest.mark.parametrize("pool", [False, True], ids=["plain", "pool"])
def test_plan_of_the_stem_form(size, pool):
    a = stem_args(*size, pool=pool)
    rc, out = ask(a)
    tiles, per, splits = expected_plan(*size)
    print(f"{size}: {tiles} tiles, {per} per split, {splits} splits, scratch {out.ws_bytes} B, reduce group {out.reduce_group}")
    assert rc == 0 and out.kernel == _lib.MSS_WG_STEM7 == 11 and out.positions == 49 and out.ktiles == out.ctiles == 1
    assert (out.splits, out.rows_per_split, out.total, out.full, out.wide_K) == (splits, per * TH * TW, splits, -1, 0)
    assert out.ws_bytes == (splits * 49 * 64 * 4 * 4 if splits > 1 else 0)
    assert out.ws_bytes == _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a), 4)
    assert (out.reduce_group == 0) == (splits == 1) and out.reduce_group in (0, 1, 2, 4, 8, 16, 32)
    assert _lib.value("mss_conv2d_wgrad_route", ctypes.byref(a), 64) == 0
    a.route = 1                                      # ignored
    assert ask(a)[0] == 0 and ask(a)[1].kernel == 11


def test_the_named_sizes_reach_one_split_several_and_a_partial_last_one():
    assert expected_plan(*STEM_SIZES[0])[2] == 1
    tiles, per, splits = expected_plan(*MULTI)
    assert splits > 1 and tiles % per != 0                     # the last split holds fewer tiles than the others
    tiles, per, splits = expected_plan(*LONG)
    assert per == 3 and splits > 1 and tiles % per != 0
    assert any(((h - 1) // 2 + 1) % 2 for _, h, _ in STEM_SIZES) and any(((h - 1) // 2 + 1) % 2 == 0 for _, h, _ in STEM_SIZES)
    assert any(((w - 1) // 2 + 1) % 2 for _, _, w in STEM_SIZES) and any(((w - 1) // 2 + 1) % 2 == 0 for _, _, w in STEM_SIZES)


NEAR_MISSES = [
    ("stride=1", dict(stride=1), "MSS_ERR_UNSUPPORTED"),
    ("pad=2", dict(pad=2), "MSS_ERR_UNSUPPORTED"),
    ("C=16", dict(C=16), "MSS_ERR_UNSUPPORTED"),
    ("K=128", dict(K=128), "MSS_ERR_UNSUPPORTED"),
    ("in_relu=1", dict(in_relu=1), "MSS_ERR_UNSUPPORTED"),
    ("R=S=5", dict(R=5, S=5), "MSS_ERR_UNSUPPORTED"),
    ("wrong OH", dict(OH=36), "MSS_ERR_BAD_ARG"),
    ("res with res_mask=0", dict(res=ctypes.c_void_p(FAKE + 0x100000), ldres=64, res_mask=0), "MSS_ERR_BAD_ARG"),
    # beyond the issue's table: the other fields of the form
    ("dil=2", dict(dil=2), "MSS_ERR_UNSUPPORTED"),
    ("ldx=8", dict(ldx=8), "MSS_ERR_UNSUPPORTED"),
    ("Kpad=128", dict(Kpad=128), "MSS_ERR_UNSUPPORTED"),
    ("batch=2", dict(batch=2), "MSS_ERR_UNSUPPORTED"),
    ("in_scale", dict(in_scale=ctypes.c_void_p(FAKE + 0x400000)), "MSS_ERR_UNSUPPORTED"),
    ("wrong OW", dict(OW=49), "MSS_ERR_BAD_ARG"),
    ("ldres=60", dict(res=ctypes.c_void_p(FAKE + 0x100000), ldres=60, res_mask=1), "MSS_ERR_BAD_ARG"),
]


@pytest.mark.parametrize("name,over,status", NEAR_MISSES, ids=[n for n, _, _ in NEAR_MISSES])
def test_near_misses_are_refused(name, over, status):
    assert ask(stem_args(1, 70, 100))[0] == 0
    assert ask(stem_args(1, 70, 100, **over))[0] == getattr(_lib, status)


def test_other_arguments_of_the_call():
    a = stem_args(1, 70, 100)
    assert ask(a, Cp=8)[0] == _lib.MSS_ERR_UNSUPPORTED          # the caller passes Cp == 4
    assert ask(a, lddy=60)[0] == _lib.MSS_ERR_BAD_ARG
    assert ask(a, lddy=72)[0] == 0
    rc, out = ask(stem_args(0, 70, 100))                        # no pixels: nothing is launched
    assert rc == 0 and out.kernel == -1 and out.ws_bytes == 0


def test_kernels_use_no_scratch():
    src = os.path.join(ROOT, "multishiftseg_amd", "csrc", "stem7_wgrad.hip")
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    assert len(blocks) == 2 and all("stem7_wgrad_kernel" in b for b in blocks), [b[:80] for b in blocks]      # the plain and the pool form
    for b in blocks:
        usage = {}
        for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            m = re.search(r" " + re.escape(key) + r": (\d+)", b)
            assert m, key
            usage[key] = int(m.group(1))
        print(b.split()[0], usage)
        assert usage["ScratchSize [bytes/lane]"] == 0 and usage["VGPRs Spill"] == 0 and usage["SGPRs Spill"] == 0, usage
        assert usage["VGPRs"] + usage["AGPRs"] <= 128 and usage["Occupancy [waves/SIMD]"] >= 4, usage      # four workgroups per CU
        assert usage["LDS Size [bytes/block]"] <= 40 * 1024, usage


# ---- ResNet bookkeeping
def _backbone():
    from multishiftseg_amd import build_resnet_backbone
    return build_resnet_backbone().eval()


def test_stem_opt_in_puts_the_stem_weight_first():
    m = _backbone().freeze(0, norms=True)
    assert m.set_trainable(stem=True) is m and m._trainable and m._train_stem
    x = torch.zeros(1, 3, 32, 32)
    params = m._check_mode(x)
    assert len(params) == 53 and params[0] is m.stem.conv1.weight
    names = {id(p): n for n, p in m.named_parameters()}
    assert all(names[id(p)].endswith(".weight") and ".norm." not in names[id(p)] for p in params)
    assert len({id(p) for p in params}) == 53
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x)                                                   # past every refusal
    m.freeze(1, norms=True)                                    # the stem frozen: the opt-in changes nothing
    assert len(m._check_mode(x)) == 52
    assert not m.set_trainable(False)._train_stem and not m.set_trainable(False, stem=True)._train_stem


@pytest.mark.parametrize("which", ["weight", "bias"])
def test_a_trainable_stem_norm_still_raises(which):
    x = torch.zeros(1, 3, 32, 32)
    for stem in (True, False):
        m = _backbone().freeze(0, norms=True).set_trainable(stem=stem)
        if not stem:
            m.freeze(1, norms=True)
        getattr(m.stem.conv1.norm, which).requires_grad_(True)
        with pytest.raises(NotImplementedError, match=f"trainable stem.*stem.conv1.norm.{which}"):
            m(x)
    assert "FrozenBatchNorm" in type(m).set_trainable.__doc__ and "dbeta" in type(m).set_trainable.__doc__


def test_the_default_switch_still_refuses_the_stem():
    m = _backbone().freeze(0, norms=True).set_trainable()
    with pytest.raises(NotImplementedError, match=r"trainable stem.*stem.conv1.weight.*set_trainable\(stem=True\)"):
        m(torch.zeros(1, 3, 32, 32))
    doc = type(m).freeze.__doc__
    assert "freeze(0, norms=True)" in doc and "set_trainable(stem=True)" in doc and "freeze(1, norms=True)" in doc


def test_maskformer_passes_the_switch_and_groups_the_stem_weight_with_the_backbone():
    from torch import nn
    from multishiftseg_amd import MaskFormer, build_m2f_param_groups

    class _Predictor(nn.Linear):
        def set_trainable(self, flag=True):
            return self

    shell = MaskFormer(_backbone().freeze(0, norms=True), nn.Sequential(nn.Linear(2, 2)), _Predictor(3, 3))
    assert not shell.set_trainable().backbone._train_stem
    assert shell.set_trainable(stem=True).backbone._train_stem and shell.backbone._trainable
    groups = build_m2f_param_groups(shell, 1e-4, 0.05)
    g = [g for g in groups if g["params"][0] is shell.backbone.stem.conv1.weight]
    assert len(g) == 1 and g[0]["lr"] == pytest.approx(1e-5) and g[0]["weight_decay"] == 0.05
    assert sum(1 for g in groups if g["lr"] == pytest.approx(1e-5)) == 53


def test_constants_and_documents():
    import multishiftseg_amd as pkg
    from multishiftseg_amd import kernels
    assert "stem7_wgrad" in pkg.__all__ and pkg.stem7_wgrad is kernels.stem7_wgrad
    assert len(_lib.MSS_WG_NAMES) == 11 and _lib.MSS_WG_STEM7 == 11
    hdr = open(os.path.join(ROOT, "include", "mss_hip.h")).read()
    assert "#define MSS_WG_STEM7 11" in hdr and f"#define MSS_ABI_VERSION {_lib.MSS_ABI_VERSION} " in hdr
    assert "stem7_wgrad.hip" in hdr and "stem7_wgrad.hip" in open(os.path.join(ROOT, "README.md")).read()
