"""What tests/test_gpu_fwd_exact.py stands on, checked without a GPU, over the one case table (tests/fwd_cases.py):

  plans         every row goes through the stand-alone checker of csrc/fwd_route.h (tests/fwd_route_check.cpp: its own main, host
                sanitizers on that program only) in the column format it already reads; the printed route equals the row's
                hand-derived plan, the library answers the same code, and the union of plans covers every class that
                tests/test_gpu_fwd_route.py names for the codes 0 to 4;
  exactness     for every row, (largest sum of |terms| of an output) / (smallest granule of a term) is below 2^24 on the integer
                lattice and at most 2^20 on the three-plane lattice (four spare bits for however the bf16 MFMA aligns its internal
                sum); the scalar epilogue, one rounding per operation, and every statistics sum stay below 2^24 of their granule.
                A condition, not a tolerance. Rows that are computed on the CPU take the maxima themselves; the large GEMM rows
                without statistics a bound above them (reduction length x largest magnitudes, or on the three-plane lattice the
                exact count of products whose factors are both non-zero);
  planes        the float64 emulation of the three-term split agrees with torch's bfloat16 rounding, its terms add up to the value
                exactly, and on the three-plane rows more than a quarter of the elements of x (as the kernel sees it, after the
                prologue) and of w have each plane non-zero; dropping the mid or the lo plane of either operand changes the result;
  reference     tests/ref_fwd.py (index arithmetic + one matrix product per tap) equals F.conv2d in float64 on every geometry row;
  sensitivity   on the reference alone (nothing broken ever runs on a GPU): dropping any one live tap, the first or the last chunk
                of 16 input channels, the last output row, or giving image 1 the affine of image 0 changes the result. A tap
                that reaches no pixel (a dilation larger than the map) is not applicable. The two rows of 1024 wide tiles check
                the same by the dropped piece alone being non-zero (the piece and the rest add up exactly)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fwd_cases as fc
import ref_fwd
import test_fwd_route_cpu as frc
import test_gpu_fwd_route as gpu_route
from multishiftseg_amd import _lib

GEOMETRY = [c for c in fc.CASES if c.geometry]
PLANES = [c for c in fc.CASES if c.data == "planes"]
SMALL = [c for c in GEOMETRY if c.M * c.K <= 1 << 21]        # all but the two rows of 1024 wide tiles: a dozen whole references each is affordable
BASE = 0x7f0000000000            # fake addresses, 16-byte aligned regions: nothing is dereferenced


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """The printed route of every row: the checker has then passed all its properties on all of them."""
    import subprocess
    exe = frc._compile(tmp_path_factory, "fwd_route_check")
    p = subprocess.run([exe], input="".join(c.checker_line() + "\n" for c in fc.CASES), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(fc.CASES)
    return {c.name: {k: (v if k == "kernel" else int(v)) for k, v in zip(frc.FIELDS, ln.split())} for c, ln in zip(fc.CASES, lines)}


@pytest.mark.parametrize("c", fc.CASES, ids=lambda c: c.name)
def test_expected_plan_is_the_headers(c, routes):
    f = routes[c.name]
    print(f"{c.name}: expected {c.expect}, printed {f}")
    assert f["status"] == 0 and f["M"] == c.M
    assert {k: f[k] for k in fc.PLAN_KEYS} == c.expect
    assert f["code"] == fc.CODES[c.expect["kernel"]]


@pytest.mark.parametrize("c", fc.CASES, ids=lambda c: c.name)
def test_the_library_answers_the_plans_code(c, monkeypatch):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    a = fc.conv_args(c, BASE + 4 * c.x_c0, BASE + (1 << 30), BASE + (2 << 30) + 4 * (fc.GUARD * c.ldy + c.y_c0), BASE + (3 << 30), BASE + (4 << 30),
                     BASE + (5 << 30), BASE + (6 << 30), BASE + (7 << 30), BASE + (8 << 30), BASE + (9 << 30), BASE + (10 << 30))
    assert _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) == fc.CODES[c.expect["kernel"]]


# test_gpu_fwd_route.CASES, codes 0 to 4: what a row's plan must show to stand for the class
CLASSES = {
    "igemm_256x64": lambda c, p: (p["kernel"], p["BM"], p["BN"], p["BK"]) == ("conv_igemm", 256, 64, 16) and c.R == 3,
    "igemm_128x128x16": lambda c, p: (p["kernel"], p["BM"], p["BN"], p["BK"], p["affine"]) == ("conv_igemm", 128, 128, 16, 1),
    "igemm_128x128x32": lambda c, p: (p["kernel"], p["BM"], p["BN"], p["BK"]) == ("conv_igemm", 128, 128, 32),
    "igemm_per_sample": lambda c, p: p["kernel"] == "conv_igemm" and p["per_sample"] == 1,
    "igemm_1x1_stride2": lambda c, p: p["kernel"] == "conv_igemm" and c.R == 1 and c.stride == 2,
    "igemm_bn64_below_16384_rows": lambda c, p: p["kernel"] == "conv_igemm" and c.gemm and c.M == 16383,
    "few_rows_8": lambda c, p: (p["kernel"], p["BM"]) == ("few_rows", 8),
    "few_rows_16": lambda c, p: (p["kernel"], p["BM"]) == ("few_rows", 16),
    "few_rows_32": lambda c, p: (p["kernel"], p["BM"]) == ("few_rows", 32),
    "gemm_nt_bn64_v3": lambda c, p: (p["kernel"], p["BN"], p["variant"]) == ("gemm_nt", 64, 3),
    "gemm_nt_bn128_v3": lambda c, p: (p["kernel"], p["BN"], p["variant"], p["affine"]) == ("gemm_nt", 128, 3, 1),
    "gemm_nt_bn128_v2": lambda c, p: (p["kernel"], p["BN"], p["variant"]) == ("gemm_nt", 128, 2) and not c.env,
    "gemm_nt_bn128_v3_batched": lambda c, p: (p["kernel"], p["BN"], p["variant"]) == ("gemm_nt", 128, 3) and c.batch > 1,
    "gemm_nt_bn256_wide_v3": lambda c, p: (p["kernel"], p["BN"], p["variant"], p["mode"]) == ("gemm_nt", 256, 3, fc.WIDE),
    "gemm_nt_bn256_hybrid_v3": lambda c, p: (p["kernel"], p["BN"], p["variant"], p["mode"]) == ("gemm_nt", 256, 3, fc.HYBRID) and not c.env,
    "gemm_nt_per_sample_whole_tiles": lambda c, p: p["kernel"] == "gemm_nt" and c.affine == "per_sample",
    "perimg_bn128": lambda c, p: (p["kernel"], p["BN"]) == ("gemm_nt_perimg", 128) and not c.k_imgs,
    "perimg_bn256": lambda c, p: (p["kernel"], p["BN"]) == ("gemm_nt_perimg", 256) and not c.k_imgs,
    "k_imgs_bn128": lambda c, p: (p["kernel"], p["BN"]) == ("gemm_nt_perimg", 128) and c.k_imgs,
    "k_imgs_bn256": lambda c, p: (p["kernel"], p["BN"]) == ("gemm_nt_perimg", 256) and c.k_imgs,
    "split_bn128_mfma16": lambda c, p: (p["kernel"], p["BN"], p["mfma"]) == ("gemm_nt_bf16x3", 128, 16),
    "split_bn128_mfma32": lambda c, p: (p["kernel"], p["BN"], p["mfma"]) == ("gemm_nt_bf16x3", 128, 32),
    "split_bn256_mfma16": lambda c, p: (p["kernel"], p["BN"], p["mfma"]) == ("gemm_nt_bf16x3", 256, 16),
    "split_bn256_mfma32": lambda c, p: (p["kernel"], p["BN"], p["mfma"]) == ("gemm_nt_bf16x3", 256, 32),
    "split_conv_bn128": lambda c, p: (p["kernel"], p["BN"]) == ("conv_bf16x3", 128),
    "split_conv_bn256": lambda c, p: (p["kernel"], p["BN"]) == ("conv_bf16x3", 256),
    "split_rowaff": lambda c, p: p["kernel"] == "rowaff_bf16x3",
}
SPLIT_CLASSES = [n for n in CLASSES if n.startswith("split_")]


def test_the_plans_cover_every_class_of_the_route_test(routes):
    assert set(CLASSES) == {n for n, (code, _, _) in gpu_route.CASES.items() if code <= 4}
    for name, shows in CLASSES.items():
        rows = [c for c in fc.CASES if shows(c, routes[c.name])]
        print(f"{name}: {[c.name for c in rows]}")
        assert rows, name
        if name in SPLIT_CLASSES:
            assert {c.data for c in rows} == {"int", "planes"}, name
    assert {routes[c.name]["code"] for c in fc.CASES} == {0, 1, 2, 3, 4}


def test_the_table_reaches_the_edges_the_kernels_have(routes):
    """The edges the rows were chosen for, counted from the table itself."""
    ig = [c for c in fc.CASES if c.expect["kernel"] == "conv_igemm"]
    assert {c.C for c in ig} >= {16, 32, 2048} and {c.K for c in ig} >= {1, 63, 64, 65, 129, 200}
    assert {c.M % c.expect["BM"] for c in ig} >= {0, 1} and any(c.M % c.expect["BM"] == c.expect["BM"] - 1 for c in ig)
    assert {(c.R, c.stride) for c in ig} >= {(3, 1), (3, 2), (1, 2)} and any(c.dil > max(c.H, c.W) for c in ig)
    few = [c for c in fc.CASES if c.expect["kernel"] == "few_rows"]
    assert {c.M for c in few} == {1, 8, 9, 16, 17, 32} and {c.K for c in few} == {1, 19, 100} and all(c.ldx > c.C for c in few)
    nt = [c for c in fc.CASES if c.expect["kernel"] == "gemm_nt"]
    assert {c.M for c in nt} >= {16384, 16385} and {c.K for c in nt} >= {65, 128, 129, 200} and {c.M % 128 for c in nt} >= {1, 127}
    assert {(k, v) for c in nt for k, v in c.env.items()} >= {("MSS_GEMM_VARIANT", "2"), ("MSS_GEMM_TAIL", "0"), ("MSS_GEMM_TAIL", "1"), ("MSS_GEMM_GROUP_M", "4")}
    assert {c.expect["mode"] for c in nt} == {fc.NARROW, fc.WIDE, fc.HYBRID}
    per = [c for c in fc.CASES if c.expect["kernel"] == "gemm_nt_perimg"]
    assert min(min(c.k_steps) for c in per) == 3 and any(c.k_base > 0 for c in per)
    for kernel in ("conv_igemm", "gemm_nt", "gemm_nt_bf16x3", "conv_bf16x3", "rowaff_bf16x3"):
        rows = [c for c in fc.CASES if c.expect["kernel"] == kernel]
        assert any(c.out_affine for c in rows) and any(c.out_relu for c in rows) and any(c.res == "add" for c in rows) and any(c.stats for c in rows), kernel
        assert any(c.ldy > c.K and c.y_c0 > 0 for c in rows) and any(c.ldx > c.C and c.x_c0 > 0 for c in rows) or kernel == "rowaff_bf16x3", kernel
        assert any(c.stats and c.M % 64 for c in rows), kernel                     # a last statistics group of fewer than 64 rows
    assert sum(c.res == "mask" for c in fc.CASES) >= 4


# ---- exactness -----------------------------------------------------------------------------------------------------------------------

granule = ref_fwd.granule


def _kept_pairs(c, a, w):
    """(plane of act(x), plane of w) of every product the route keeps."""
    if not c.split:
        return [(a, w)]
    ah, am, al = ref_fwd.split3(a)
    wh, wm, wl = ref_fwd.split3(w)
    return [(ah, wh), (ah, wm), (am, wh), (ah, wl), (al, wh), (am, wm)]


@pytest.mark.parametrize("c", fc.CASES, ids=lambda c: c.name)
def test_exactness_condition(c):
    ops = fc.operands(c)
    a, w = fc.activated(c, ops), ops["w"].double()
    unit = min(granule(p) * granule(q) for p, q in _kept_pairs(c, a, w) if bool(p.any()) and bool(q.any()))
    limit = 2.0 ** 20 if c.data == "planes" else 2.0 ** 24
    if c.ref == "cpu" or c.stats:
        most, how = float(fc.accumulators(c, ops, absolute=True).max()), "max sum |terms|"
    elif c.data == "planes":
        nz_a, nz_w = (a != 0).float().view(c.nb, c.N, c.M // c.N, c.C), (w != 0).float().view(c.nw, c.K, c.C)
        count = max(float((nz_a[b, n] @ nz_w[b if c.batch > 1 else 0].t()).max()) for b in range(c.nb) for n in range(c.N))
        # a full product is |a| |w| (1 + ...) of its kept terms, below (|hi| + |mid| + |lo|)^2 of the largest values
        most, how = count * float(a.abs().max() * w.abs().max()) * 1.01, f"{count:g} products with two non-zero factors x largest magnitudes"
    else:
        most, how = c.R * c.R * c.C * float(a.abs().max() * w.abs().max()), "reduction length x largest magnitudes"
    print(f"{c.name}: {how} = {most:g} in units of {unit:g}: 2^{torch.log2(torch.tensor(most / unit)):.2f} of 2^{torch.log2(torch.tensor(limit)):.0f}")
    assert most / unit <= limit if c.data == "planes" else most / unit < limit
    # the epilogue: acc * out_scale + out_shift (+ res), one rounding each
    osc = ops["out_scale"].double() if c.out_affine else torch.ones(1, dtype=torch.float64)
    unit_y = unit * granule(osc)
    top = most * float(osc.max()) + (2.0 if c.out_affine else 0.0) + (2.0 if c.res == "add" else 0.0)
    for name in ("out_shift", "res"):
        if ops[name] is not None:
            assert granule(ops[name]) == 1.0 and float(ops[name].abs().max()) <= 2.0
    assert top / unit_y < 2.0 ** 24
    if c.stats:
        y, st = fc.reference(c, ops)
        grouped = ref_fwd.stats(y[0].abs())
        assert float(grouped[:, 0].max()) / unit_y < 2.0 ** 24 and float(grouped[:, 1].max()) / unit_y ** 2 < 2.0 ** 24
        print(f"{c.name}: statistics: max sum |y| = {float(grouped[:, 0].max()):g}, max sum y^2 = {float(grouped[:, 1].max()):g} in units of {unit_y:g} and its square:"
              f" 2^{torch.log2(grouped[:, 1].max() / unit_y ** 2):.2f} of 2^24")
        assert granule(st) >= unit_y ** 2


def test_raising_the_magnitudes_breaks_the_condition():
    """The condition is a real one: the three-plane lattice at twice the products per output no longer holds it."""
    c = fc.BY_NAME["sp128_mf16_planes"]
    ops = fc.operands(c)
    a, w = fc.activated(c, ops), ops["w"].double()
    most = float(fc.accumulators(c, ops, absolute=True).max())
    unit = min(granule(p) * granule(q) for p, q in _kept_pairs(c, a, w))
    assert unit == 2.0 ** -18 and 2.0 < most <= 4.0 and 2 * most / unit > 2.0 ** 20


# ---- the split -------------------------------------------------------------------------------------------------------------------------

def test_split_emulation_is_bf16_rounding():
    g = torch.Generator().manual_seed(7)
    v = torch.cat([torch.randn(4096, generator=g), torch.tensor([fc.V3, -fc.V3, fc.V2, 1.0, 0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 - 2.0 ** -9, 3.0 + 2.0 ** -9])]).float()
    hi, mid, lo = ref_fwd.split3(v)
    assert torch.equal(hi, v.bfloat16().double())                                    # ties included (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6)
    r1 = v - hi.float()
    assert torch.equal(mid, r1.bfloat16().double()) and torch.equal(lo, (r1 - mid.float()).bfloat16().double())
    assert torch.equal(hi + mid + lo, v.double())
    assert [float(t) for t in ref_fwd.split3(torch.tensor([fc.V3]))] == [1.0, 2.0 ** -9, 2.0 ** -18]


@pytest.mark.parametrize("c", PLANES, ids=lambda c: c.name)
def test_plane_shares_and_that_every_plane_matters(c):
    ops = fc.operands(c)
    a, w = fc.activated(c, ops), ops["w"].double()
    shares = {}
    for name, t in (("x", a), ("w", w)):
        planes = ref_fwd.split3(t)
        assert torch.equal(sum(planes), t)
        shares[name] = [float((p != 0).double().mean()) for p in planes]
        assert min(shares[name]) > 0.25, (c.name, name, shares[name])
    print(f"{c.name}: share of elements with a non-zero hi / mid / lo plane: x {shares['x']}, w {shares['w']}")
    if c.ref == "cpu" and c.M * c.K <= 1 << 21:
        true = fc.accumulators(c, ops)
        assert float(true.abs().max()) > 0.0
        for which in ("x", "w"):
            for plane in (1, 2):
                cut = dict(ops)
                hi, mid, lo = ref_fwd.split3(a if which == "x" else w)
                less = (hi + (lo if plane == 1 else mid))
                if which == "w":
                    cut["w"] = less.float()
                    assert torch.equal(cut["w"].double(), less)
                    assert not torch.equal(fc.accumulators(c, cut), true), (c.name, which, plane)
                else:                                                                    # (x goes through the prologue: cut the activated values)
                    got = torch.stack([ref_fwd.product(less[b], w[b if c.batch > 1 else 0], True, c.stride, c.dil, c.pad).view(c.M, c.K) for b in range(c.nb)])
                    assert not torch.equal(got, true), (c.name, which, plane)


# ---- reference and sensitivity -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in GEOMETRY if not c.split], ids=lambda c: c.name)
def test_reference_is_conv2d_in_float64(c):
    ops = fc.operands(c)
    a = fc.activated(c, ops)[0]
    want = F.conv2d(a.permute(0, 3, 1, 2), ops["w"][0].double(), stride=c.stride, padding=c.pad, dilation=c.dil).permute(0, 2, 3, 1)
    got = fc.accumulators(c, ops)[0].view(want.shape)
    assert torch.equal(got, want) and float(got.abs().max()) > 0.0                  # (integers: float64 is exact in any order too)


@pytest.mark.parametrize("c", [c for c in GEOMETRY if c.split], ids=lambda c: c.name)
def test_split_reference_is_conv2d_of_the_kept_products(c):
    ops = fc.operands(c)
    a = fc.activated(c, ops)[0]
    ap, wp = ref_fwd.split3(a), ref_fwd.split3(ops["w"][0])
    want = sum(F.conv2d(ap[i].permute(0, 3, 1, 2), wp[j], stride=c.stride, padding=c.pad, dilation=c.dil) for i, j in ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)))
    got = fc.accumulators(c, ops)[0].view(c.N, c.OH, c.OW, c.K)
    assert torch.equal(got, want.permute(0, 2, 3, 1))                                # (multiples of 2^-18 below 4: exact in any order)
    if c.data == "planes":                                                           # ... and not the true product
        true = F.conv2d(a.permute(0, 3, 1, 2), ops["w"][0].double(), stride=c.stride, padding=c.pad, dilation=c.dil).permute(0, 2, 3, 1)
        assert not torch.equal(got, true) and float((got - true).abs().max()) < 2.0 ** -24


def _wrong_variants(c):
    v = {f"tap{t}": ("tap", t) for t in ref_fwd.live_taps(c.H, c.W, c.R, c.stride, c.dil, c.pad)}
    v["first_chunk"], v["last_chunk"], v["last_row"] = ("chunk", 0), ("chunk", c.C - 16), ("row", c.M - 1)
    if c.affine == "per_sample":
        v["affine"] = ("affine", [0, 0] + list(range(2, c.N)))
    return v


@pytest.mark.parametrize("c", GEOMETRY, ids=lambda c: c.name)
def test_reference_notices_each_wrong_variant(c):
    ops = fc.operands(c)
    if c in SMALL:
        true = fc.accumulators(c, ops)
        for name, wrong in _wrong_variants(c).items():
            assert not torch.equal(fc.accumulators(c, ops, wrong=wrong), true), (c.name, name)
        return
    # the 1024-wide-tile rows: the piece alone is not all zero, which is the same statement (every sum here is exact) at a ninth of the cost
    assert not c.affine
    for wrong in sorted(set(_wrong_variants(c).values())):              # (C = 16: the first chunk is the last)
        assert bool(fc.accumulators(c, ops, only=wrong).any()), (c.name, wrong)


def test_a_piece_and_the_rest_add_up():
    """What the large rows' form of the sensitivity check stands on."""
    c = fc.BY_NAME["spc128_3x3_s2_planes"]
    ops = fc.operands(c)
    true = fc.accumulators(c, ops)
    for wrong in (("tap", 0), ("tap", 4), ("chunk", 0), ("row", c.M - 1)):
        assert torch.equal(fc.accumulators(c, ops, wrong=wrong) + fc.accumulators(c, ops, only=wrong), true), wrong


def test_every_wrong_variant_is_applicable_somewhere():
    count = {}
    assert {c.name for c in GEOMETRY} - {c.name for c in SMALL} == {"spc256_3x3_int", "spc256_3x3_planes"}
    for c in GEOMETRY:
        for name in _wrong_variants(c):
            count[name] = count.get(name, 0) + 1
    assert all(count[f"tap{t}"] >= 10 for t in range(9)) and count["affine"] >= 3, count
    dead = fc.BY_NAME["ig_dil20"]
    assert ref_fwd.live_taps(dead.H, dead.W, 3, 1, dead.dil, dead.pad) == [4]
