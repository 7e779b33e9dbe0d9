"""What tests/test_gpu_wgrad_exact.py stands on, checked without a GPU, over the one case table (tests/wgrad_cases.py):

  reference     tests/ref_wgrad.py (index arithmetic + one matrix product per tap) equals torch.nn.grad.conv2d_weight in float64 on the
                prologue's output, on every geometry case;
  exactness     for every case max over (tap, k, c) of sum_m |dy| |act(x)| is below 2^24 in units of the data's grid (1, or 1/2 where
                a scale of 0.5 occurs) and every input, scale and shift lies on it: an fp32 evaluation is then exact in any order.
                A condition, not a tolerance. The geometry cases compute the maximum itself; the large 1x1 / batched cases the
                bound rows * max|dy| * max|act(x)|, which is above it;
  plans         the hand-derived plan of every row is what mss_conv2d_wgrad_plan answers (fake aligned addresses, no device), and
                the table reaches every WgradKernel and every reduce group 0, 1, 2, 4, 8, 16, 32;
  sensitivity   on the reference alone (nothing broken ever runs on a GPU): a dropped last pixel of the first split, a dropped first
                pixel of the second image, the centre tap read one pixel further, stride and dilation swapped, image 0's affine
                used for image 1 -- each gives a result different from the true one. A change that is the identity by construction
                is not applicable: one image, stride == dilation, no per-sample affine."""
import ctypes

import pytest
import torch

import ref_wgrad
import wgrad_cases as wc
from multishiftseg_amd import _lib

GEOMETRY = [c for c in wc.CASES if c.geometry]
BASE = 0x7f0000000000            # fake addresses: 4 KiB aligned regions, nothing is dereferenced


def _fake_call(c):
    a = wc.conv_args(c, BASE + 4 * c.x_c0, BASE + (1 << 30), BASE + (2 << 30), BASE + (3 << 30))
    return a, BASE + (4 << 30) + 4 * c.dy_c0, BASE + (5 << 30)


def _answer(c, monkeypatch):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    a, dy, dwp = _fake_call(c)
    ws_bytes = _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a), c.Cp)
    return wc.answered_plan(c, a, dy, dwp, ws_bytes) + (ws_bytes,)


@pytest.mark.parametrize("c", GEOMETRY, ids=lambda c: c.name)
def test_reference_is_conv2d_weight_in_float64(c):
    x, dy, scale, shift = wc.operands(c)
    got = ref_wgrad.wgrad(x, dy, c.R, c.R, c.stride, c.dil, c.pad, scale, shift, c.relu, c.Kpad, c.Cp)
    a = ref_wgrad.act(x, scale, shift, c.relu).permute(0, 3, 1, 2)
    want = torch.nn.grad.conv2d_weight(a, (c.K, c.C, c.R, c.R), dy.double().permute(0, 3, 1, 2), stride=c.stride, padding=c.pad, dilation=c.dil)
    assert torch.equal(ref_wgrad.unpack(got, c.K, c.C, c.R, c.R), want)              # (integers: float64 is exact in any order too)
    assert got.shape == (c.R * c.R, c.Kpad, c.Cp)
    assert float(got[:, c.K:].abs().max() if c.Kpad > c.K else 0.0) == 0.0 and float(got[:, :, c.C:].abs().max() if c.Cp > c.C else 0.0) == 0.0
    assert float(got.abs().max()) > 0.0


@pytest.mark.parametrize("c", wc.CASES, ids=lambda c: c.name)
def test_exactness_condition(c):
    x, dy, scale, shift = wc.operands(c)
    unit = 0.5 if scale is not None and bool((scale == 0.5).any()) else 1.0
    for t in (x, dy, shift):
        if t is not None:
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2.0
    if scale is not None:
        assert bool(((scale == 0.5) | (scale == 1.0) | (scale == 2.0)).all())
    if c.geometry:
        most = float(ref_wgrad.wgrad(x, dy, c.R, c.R, c.stride, c.dil, c.pad, scale, shift, c.relu, absolute=True).max())
        how = "max sum |dy||act|"
    else:
        a = x.double().view(-1, c.C)
        if scale is not None:
            a = a * scale.double() + shift.double()
        most = float(c.M * dy.abs().max().double() * a.abs().max())
        how = "rows * max|dy| * max|act|"
    print(f"{c.name}: {how} = {most:g} in units of {unit:g}: {most / unit / 2 ** 24:.2e} of 2^24")
    assert most / unit < 2 ** 24


@pytest.mark.parametrize("c", wc.CASES, ids=lambda c: c.name)
def test_expected_plan_is_the_librarys(c, monkeypatch):
    got, pl, ws_bytes = _answer(c, monkeypatch)
    print(f"{c.name}: expected {c.expect}, answered {got} (rows per split {pl.rows_per_split}, {pl.total} jobs, scratch {pl.ws_bytes} of {ws_bytes} B)")
    assert got == c.expect
    assert pl.ws_bytes <= ws_bytes
    a, dy, dwp = _fake_call(c)
    out = _lib.MssWgradPlan()
    if c.expect["kernel"] != "two_part":
        assert _lib.value("mss_conv2d_wgrad_plan", ctypes.byref(a), dy, c.lddy, dwp, c.Cp, ws_bytes, 1, ctypes.byref(out)) == _lib.MSS_ERR_BAD_ARG
    assert _lib.value("mss_conv2d_wgrad_plan", ctypes.byref(a), dy, c.lddy, dwp, c.Cp, ws_bytes, 3, ctypes.byref(out)) == _lib.MSS_ERR_BAD_ARG


def test_the_table_reaches_every_kernel_and_every_reduce_group(monkeypatch):
    kernels, groups = set(), set()
    for c in wc.CASES:
        got, pl, _ = _answer(c, monkeypatch)
        for k in c.env:
            monkeypatch.delenv(k)
        launches = got.get("parts") or [(got["kernel"], got["splits"], got["reduce_group"])]
        kernels |= {got["kernel"]} | {p[0] for p in launches}
        groups |= {p[2] for p in launches}
    print(f"kernels reached: {sorted(kernels)}; reduce groups reached: {sorted(groups)}")
    assert kernels == set(wc.KERNELS)
    assert groups == {0, 1, 2, 4, 8, 16, 32}
    assert len({c.seed for c in wc.CASES}) == len(wc.CASES)


def test_the_query_answers_the_launchs_argument_checks():
    """The statuses of mss_conv2d_wgrad_f32's argument checks, in their order, from the query; an empty product is MSS_OK without a kernel."""
    c = wc.BY_NAME["c3x3_k19"]
    out = _lib.MssWgradPlan()

    def ask(a, dy, dwp, lddy=c.lddy, Cp=c.Cp):
        return _lib.value("mss_conv2d_wgrad_plan", ctypes.byref(a), dy, lddy, dwp, Cp, 0, 0, ctypes.byref(out))
    a, dy, dwp = _fake_call(c)
    assert ask(a, dy, dwp) == 0 and out.kernel == _lib.MSS_WG_NAMES.index("conv32")
    assert ask(a, None, dwp) == ask(a, dy, None) == _lib.MSS_ERR_BAD_ARG
    a.x = None
    assert ask(a, dy, dwp) == _lib.MSS_ERR_BAD_ARG
    a, dy, dwp = _fake_call(c)
    assert ask(a, dy, dwp, lddy=46) == ask(a, dy, dwp, Cp=34) == _lib.MSS_ERR_UNSUPPORTED
    a.C = 30
    assert ask(a, dy, dwp) == _lib.MSS_ERR_UNSUPPORTED
    a, dy, dwp = _fake_call(c)
    a.batch = 3                                                     # positions are 1x1 products
    assert ask(a, dy, dwp) == _lib.MSS_ERR_BAD_ARG
    a, dy, dwp = _fake_call(c)
    a.N = 0
    assert ask(a, dy, dwp) == 0 and (out.kernel, out.splits, out.total, out.reduce_group) == (-1, 0, 0, 0)
    a, dy, dwp = _fake_call(wc.BY_NAME["tn_direct_perimg"])
    a.in_relu = 1                                                   # the per-image form has no prologue
    assert ask(a, dy, dwp, lddy=256, Cp=512) == _lib.MSS_ERR_UNSUPPORTED
    assert _lib.MSS_WG_NAMES == wc.KERNELS
    # dwp's padding must lie inside the last tile of the kernel that runs: its epilogue is the only thing that writes it
    c = wc.BY_NAME["c3x3_k19"]                                      # conv32: 32 rows, 128 columns
    a, dy, dwp = _fake_call(c)
    a.Kpad = 32
    assert ask(a, dy, dwp, Cp=128) == 0
    assert ask(a, dy, dwp, Cp=132) == _lib.MSS_ERR_UNSUPPORTED
    a.Kpad = 33
    assert ask(a, dy, dwp, Cp=128) == _lib.MSS_ERR_UNSUPPORTED
    for name, kpad_ok, kpad_bad, cp_bad in (("dil2", 64, 68, 132), ("s2_1x1", 256, 260, 132), ("tn_lds_k136", 256, 260, 132),
                                            ("narrow_k19", 32, 36, None), ("narrow_k48", 64, 68, None), ("tn_direct", 512, 516, 516),
                                            ("tn_direct_tail", 512, 516, 516), ("tn_wide", 256, 260, 2052)):
        c = wc.BY_NAME[name]
        a, dy, dwp = _fake_call(c)
        a.Kpad = kpad_ok
        assert ask(a, dy, dwp, lddy=c.lddy, Cp=c.Cp) == 0 and wc.KERNELS[out.kernel] == c.expect["kernel"], name
        a.Kpad = kpad_bad
        assert ask(a, dy, dwp, lddy=c.lddy, Cp=c.Cp) == _lib.MSS_ERR_UNSUPPORTED, name
        a.Kpad = kpad_ok
        if cp_bad:
            assert ask(a, dy, dwp, lddy=c.lddy, Cp=cp_bad) == _lib.MSS_ERR_UNSUPPORTED, name
    c = wc.BY_NAME["two_part"]                                      # the second part's 32 rows are the narrow kernel's whole tile
    a, dy, dwp = _fake_call(c)
    a.Kpad = 164
    assert ask(a, dy, dwp, lddy=c.lddy, Cp=c.Cp) == _lib.MSS_ERR_UNSUPPORTED
    # ws_bytes decides one thing: without the scratch for its two slabs the split-bf16 kernel is skipped and the native rule answers
    # (256 tiles, cap ceil(520 / 256) = 3 -> 768 one-wave jobs, 3 splits of 174 rows)
    c = wc.BY_NAME["tn_bf16x3"]
    a, dy, dwp = _fake_call(c)
    for ws_bytes, want in ((2 * 32 * 256 * 512 * 4, ("tn_bf16x3", 2, 272)), (2 * 32 * 256 * 512 * 4 - 1, ("tn_direct", 3, 174)), (0, ("tn_direct", 3, 174))):
        assert _lib.value("mss_conv2d_wgrad_plan", ctypes.byref(a), dy, c.lddy, dwp, c.Cp, ws_bytes, 0, ctypes.byref(out)) == 0
        assert (wc.KERNELS[out.kernel], out.splits, out.rows_per_split) == want


def _wrong_variants(c, rows_per_split):
    v = {"drop_split_end": ("drop", min(rows_per_split, c.M) - 1), "tap_shift": ("tap", (c.R * c.R) // 2, 0, 1)}
    if c.N > 1:
        v["drop_image_start"] = ("drop", c.OH * c.OW)
    if c.stride != c.dil:
        v["swap"] = ("swap",)
    if c.affine == "per_sample":
        v["affine"] = ("affine", [0, 0] + list(range(2, c.N)))
    return v


@pytest.mark.parametrize("c", GEOMETRY, ids=lambda c: c.name)
def test_reference_notices_each_wrong_variant(c, monkeypatch):
    _, pl, _ = _answer(c, monkeypatch)
    x, dy, scale, shift = wc.operands(c)

    def ref(wrong=None):
        return ref_wgrad.wgrad(x, dy, c.R, c.R, c.stride, c.dil, c.pad, scale, shift, c.relu, c.Kpad, c.Cp, wrong=wrong)
    true = ref()
    for name, wrong in _wrong_variants(c, pl.rows_per_split).items():
        assert not torch.equal(ref(wrong), true), (c.name, name)


def test_every_wrong_variant_is_applicable_somewhere():
    count = {}
    for c in GEOMETRY:
        for name in _wrong_variants(c, 16):
            count[name] = count.get(name, 0) + 1
    assert count["drop_split_end"] == count["tap_shift"] == len(GEOMETRY)
    assert count["drop_image_start"] >= 15 and count["swap"] >= 6 and count["affine"] >= 1, count
