"""The forward routing (csrc/fwd_route.h: kernel, tile, variant, rounds) without a GPU.

tests/golden/fwd_route_parent.json pins what mss_conv2d_forward_route answered before the routing became one header
(tools/gen_fwd_route_golden.py): the library must answer the same code on every row, except the rows named in gen.OVER_SPAN_BN64,
where the old query disagreed with the launch and the launch is the authority. A stand-alone program (tests/fwd_route_check.cpp, its
own main, built with the host compiler's address and undefined-behaviour sanitizers) checks every row's route against what the
kernels assume and prints it; the printed routes are compared with the rules written down again here: the order of the routes, the
three width rules and the variant rule."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from multishiftseg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multishiftseg_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fwd_route_golden as gen  # noqa: E402
import test_gemm_rounds_cpu as rounds  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fwd_route_parent.json")))
ROWS = [dict(zip(GOLDEN["columns"], r)) for r in GOLDEN["rows"]]
FIELDS = ["code", "status", "kernel", "M", "BM", "BN", "BK", "variant", "affine", "per_sample", "mfma", "mode", "tiles256", "full", "rem",
          "mtiles", "ntiles", "rows_per_group"]
CODES = {"conv_igemm": 0, "gemm_nt": 1, "gemm_nt_perimg": 1, "few_rows": 2, "gemm_nt_bf16x3": 3, "conv_bf16x3": 4, "rowaff_bf16x3": 4,
         "stem7": 5, "dgrad_s2": 6}
U32, S31 = 0xffffffff, 0x7fffffff


def test_the_case_table_is_the_generators():
    assert GOLDEN["envs"] == gen.ENVS
    assert [{k: r[k] for k in ["name"] + gen.COLUMNS} for r in ROWS] == gen.cases()
    assert set(gen.OVER_SPAN_BN64) <= {r["name"] for r in ROWS}


def test_the_library_answers_the_parents_code_on_every_row():
    got = gen.answers(_lib, ROWS)
    for r, g in zip(ROWS, got):
        if r["name"] in gen.OVER_SPAN_BN64:
            assert (r["code"], g) == (1, 0), r["name"]          # the launch always ran conv_igemm_kernel there; now the label says so
        else:
            assert g == r["code"], (r["name"], g)
    assert set(got) == {0, 1, 2, 3, 4, 5, 6}


def _compile(tmp_path_factory, name):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _compile(tmp_path_factory, "fwd_route_check")


def _switches(r):
    env = GOLDEN["envs"][r["env"]]
    return {k: int(env.get(k, d)) for k, d in gen.SWITCHES}


@pytest.fixture(scope="module")
def routes(checker):
    """(row, printed route) of every row: the checker has then passed all its properties on all of them."""
    text = "".join(" ".join(map(str, [r[k] for k in gen.COLUMNS[:-1]] + list(_switches(r).values()))) + "\n" for r in ROWS)
    p = subprocess.run([checker], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(ROWS)
    return [(r, {k: (v if k == "kernel" else int(v)) for k, v in zip(FIELDS, ln.split())}) for r, ln in zip(ROWS, lines)]


def test_the_header_agrees_with_the_library_and_accepts_every_row(routes):
    got = gen.answers(_lib, ROWS)
    for (r, f), g in zip(routes, got):
        assert f["status"] == 0 and f["code"] == g == CODES[f["kernel"]], (r["name"], f, g)


def test_a_refused_call_still_gets_its_kernels_code():
    """include/mss_hip.h: the query answers 0..6 for arguments the launch refuses (callers label a call before `y` is set)"""
    import ctypes
    lib = _lib.load()
    lib.mss_env_reset()
    keep = []
    for r in ROWS:
        if r["env"] == 0 and r["name"] not in gen.OVER_SPAN_BN64:
            a = gen.conv_args(_lib, r, keep)
            a.y = None
            assert lib.mss_conv2d_forward_route(ctypes.byref(a)) == r["code"], r["name"]
            a = gen.conv_args(_lib, r, keep)
            a.x = gen.FAKE + 4                                 # misaligned: MSS_ERR_BAD_ARG at launch
            if r["R"] != 7 and not (r["R"] == 1 and r["stride"] == 1 and r["N"] * r["H"] * r["W"] <= 32):      # (the stem and few-rows rules read x's alignment)
                assert lib.mss_conv2d_forward_route(ctypes.byref(a)) == r["code"], r["name"]


# ---- the rules once more, from the row's columns -------------------------------------------------------------------------------------

def wide_dense(mtiles, K, C, batch):
    """256-wide tiles: two rounds of the 512 slots, unless the last wide round fills below 0.8 and narrow tiles fill 0.15 better"""
    return rounds.parent_plan(mtiles, K, C, batch, 0)[0] == rounds.WIDE


def wide_perimg(mtiles, K, C):
    return K % 256 == 0 and C >= 256 and mtiles * (K // 256) >= 1024


def wide_split_conv(mtiles, K):
    return K % 256 == 0 and mtiles * (K // 256) >= 1024


def expected(c, sw):
    """(kernel, BN, variant, mode) by the documented order: dgrad_s2, stem7, few rows, k_steps, NT GEMM (128 x 64 tile, split, native),
    split implicit GEMM (per-sample rows first), implicit GEMM"""
    OH, OW, pad = gen.out_size(c)
    M, nb, K, C, taps = c["N"] * OH * OW, max(c["batch"], 1), c["K"], c["C"], c["R"] ** 2
    x_bs = c["x_bs"] or c["N"] * c["H"] * c["W"] * c["ldx"]
    w_bs = c["w_bs"] or c["Kpad"] * C
    mtiles = -(-M // 128)
    affine, split = c["affine"] == 1, c["w_split"] == 1                 # (a misaligned w_split: no split route)
    per_sample = affine and c["in_ss_stride"] != 0
    one_by_one = c["R"] == 1 and c["stride"] == 1
    if c["stride"] == -2:
        return "dgrad_s2", 64 if K <= 64 else 128, 0, rounds.NARROW
    if c["R"] == 7:
        return "stem7", 64, 0, rounds.NARROW
    plain = not (c["affine"] or c["epilogue"] or c["res"] or c["stats"])
    if one_by_one and M <= 32 and c["batch"] <= 1 and plain and (sw["MSS_GEMM"] or c["k_steps"]):
        return "few_rows", 0, 0, rounds.NARROW
    if c["k_steps"]:
        wide = wide_dense(mtiles, K, C, c["batch"]) if c["k_imgs"] else wide_perimg(mtiles, K, C)
        return "gemm_nt_perimg", 256 if wide else 128, 3, rounds.WIDE if wide else rounds.NARROW
    span_x, span_w = ((nb - 1) * x_bs + M * c["ldx"]) * 4, ((nb - 1) * w_bs + c["Kpad"] * C) * 4
    bn64 = 32 <= K <= 64 and C // 16 >= 3 and M >= 16384
    gemm_shape = (one_by_one and (K > 64 or bn64) and C % 16 == 0 and C >= 32 and c["affine"] != 2 and not (per_sample and (OH * OW) % 128))
    if sw["MSS_GEMM"] and gemm_shape and not (K <= 64 and (span_x >= U32 or span_w >= U32)):
        if K <= 64:
            return "gemm_nt", 64, 3, rounds.NARROW
        if (split and C // 16 >= 3 and c["Kpad"] % 128 == 0 and (c["batch"] <= 1 or w_bs == c["Kpad"] * C) and M * c["ldx"] * 4 < U32
                and nb * c["Kpad"] * C * 6 < U32):
            wide = wide_dense(mtiles, K, C, c["batch"])
            return "gemm_nt_bf16x3", 256 if wide else 128, 0, rounds.WIDE if wide else rounds.NARROW
        variant = 3 if sw["MSS_GEMM_VARIANT"] == 3 and C // 16 >= 3 and span_x < U32 and span_w < U32 else 2
        mode = rounds.expected_plan(mtiles, K, C, c["batch"], sw["MSS_GEMM_TAIL"])[0]
        return "gemm_nt", 128 if mode == rounds.NARROW else 256, variant, mode
    if split and K > 64 and c["Kpad"] % 128 == 0 and C % 16 == 0 and c["batch"] <= 1:
        if one_by_one and per_sample and (OH * OW) % 128 and C // 16 >= 3 and M * c["ldx"] * 4 < U32 and c["Kpad"] * C * 6 < U32:
            return "rowaff_bf16x3", 128, 0, rounds.NARROW
        if (not one_by_one and taps <= 9 and taps * (C // 16) >= 3 and not per_sample and c["affine"] != 2
                and c["N"] * c["H"] * c["W"] * c["ldx"] * 4 < S31 and taps * c["Kpad"] * C * 6 < U32):
            wide = wide_split_conv(mtiles, K)
            return "conv_bf16x3", 256 if wide else 128, 0, rounds.WIDE if wide else rounds.NARROW
    return "conv_igemm", 64 if K <= 64 else 128, 0, rounds.NARROW


def test_routes_are_the_rules(routes):
    for r, f in routes:
        assert (f["kernel"], f["BN"], f["variant"], f["mode"]) == expected(r, _switches(r)), (r["name"], f, expected(r, _switches(r)))


def test_every_kernel_tile_and_variant_is_among_the_rows(routes):
    fs = [f for _, f in routes]
    assert {f["kernel"] for f in fs} == set(CODES)
    for kernel, bns in (("gemm_nt", {64, 128, 256}), ("gemm_nt_perimg", {128, 256}), ("gemm_nt_bf16x3", {128, 256}), ("conv_bf16x3", {128, 256}),
                        ("conv_igemm", {64, 128}), ("dgrad_s2", {64, 128})):
        assert {f["BN"] for f in fs if f["kernel"] == kernel} == bns, kernel
    assert {(f["BN"], f["variant"], f["mode"]) for f in fs if f["kernel"] == "gemm_nt"} >= {
        (bn, v, m) for v in (2, 3) for bn, m in ((128, rounds.NARROW), (256, rounds.WIDE), (256, rounds.HYBRID))}
    assert {(f["BN"], f["mfma"]) for f in fs if f["kernel"] == "gemm_nt_bf16x3"} == {(bn, mf) for bn in (128, 256) for mf in (16, 32)}
    assert {f["BK"] for f in fs if f["kernel"] == "conv_igemm" and f["BN"] == 128} == {16, 32}
    assert {f["BM"] for f in fs if f["kernel"] == "few_rows"} == {8, 16, 32}
    assert {f["per_sample"] for f in fs if f["kernel"] == "conv_igemm" and f["affine"]} == {0, 1}


def test_named_rows_get_the_documented_kernels(routes):
    by = {r["name"]: f for r, f in routes}
    want = {"aspp_compose": ("gemm_nt", 256, rounds.HYBRID), "aspp_compose_tail0": ("gemm_nt", 128, rounds.NARROW), "aspp_project": ("gemm_nt", 256, rounds.HYBRID),
            "wino_f6_aspp": ("gemm_nt", 128, rounds.NARROW), "wino_f6_mod4": ("gemm_nt", 256, rounds.WIDE), "wino_f6_mod4_env4": ("gemm_nt", 256, rounds.HYBRID),
            "dec_16img_256to256": ("gemm_nt", 256, rounds.HYBRID), "dec_16img_256to32": ("gemm_nt", 64, rounds.NARROW),
            "wino_f6_final_dgrad_tail": ("gemm_nt", 64, rounds.NARROW), "dl_16x768x768_aspp_pool": ("few_rows", 0, rounds.NARROW),
            "dl_16x700x700_mod7_1x1_b": ("conv_igemm", 128, rounds.NARROW), "dl_16x700x700_mod7_1x1_b_split": ("rowaff_bf16x3", 128, rounds.NARROW),
            "dl_1x512x1024_aspp_3x3_d12": ("conv_igemm", 128, rounds.NARROW), "r50_stem": ("stem7", 64, rounds.NARROW),
            "bn64_x_span_under": ("gemm_nt", 64, rounds.NARROW), "bn64_x_span_over": ("conv_igemm", 64, rounds.NARROW),
            "v3_x_span_under": ("gemm_nt", 256, rounds.WIDE), "split_x_span_over": ("gemm_nt", 256, rounds.WIDE), "dropped_k_imgs_wide": ("gemm_nt_perimg", 256, rounds.WIDE)}
    for name, w in want.items():
        assert (by[name]["kernel"], by[name]["BN"], by[name]["mode"]) == w, (name, by[name])
    assert (by["aspp_compose"]["full"], by["aspp_compose"]["rem"]) == (512, 384)
    assert by["v3_x_span_under"]["variant"] == 3 and by["v3_x_span_over"]["variant"] == 2 and by["v3_w_span_over"]["variant"] == 2
    assert by["dl_1x512x1024_aspp_3x3_d12"]["BK"] == 32 and by["dl_1x512x1024_mod4_3x3"]["BK"] == 16


def test_the_replaced_width_rules_were_the_rounds_rule(tmp_path_factory):
    """The k_imgs branch of the NT dispatch and the split GEMM launch each wrote the wide-tile rule out by hand; both now ask
    mss_gemm_rounds(..., 0). On the whole grid of test_gemm_rounds_cpu.py the hand-written rule (here once more) and the header agree,
    so the replacement was an identity; the two rules that really differ are what their names say."""
    grid = sorted({c[:4] for c in rounds.GRID})

    def by_hand(mtiles, K, C, batch):
        t = mtiles * (K // 256) * max(batch, 1)
        wide = K % 256 == 0 and t >= 1024 and C >= 256
        if wide:
            ew, en = t / (-(-t // 512) * 512), 2 * t / (-(-2 * t // 768) * 768)
            if ew < 0.8 and en > ew + 0.15:
                wide = False
        return wide

    out = subprocess.run([_compile(tmp_path_factory, "gemm_rounds_check"), "width"], input="".join(" ".join(map(str, c)) + "\n" for c in grid), capture_output=True, text=True, check=True).stdout
    got = [tuple(int(v) for v in ln.split()) for ln in out.split("\n")[:-1]]
    assert len(got) == len(grid)
    for c, g in zip(grid, got):
        assert g == (by_hand(*c), wide_perimg(*c[:3]), wide_split_conv(*c[:2])), (c, g)
    assert len({g for g in got}) >= 4                          # the three rules really differ somewhere on the grid
