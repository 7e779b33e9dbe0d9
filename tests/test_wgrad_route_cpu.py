"""The weight gradient's routing (csrc/wgrad_route.h: kernel, splits, rows per split, scratch) without a GPU.

tests/golden/wgrad_route_parent.json pins what mss_conv2d_wgrad_workspace_bytes and mss_conv2d_wgrad_route answered before the routing
became one header (tools/gen_wgrad_route_golden.py): the route must be equal on every row and the scratch never larger. A stand-alone
program (tests/wgrad_route_check.cpp, its own main, built with the host compiler's address and undefined-behaviour sanitizers) checks
every row under every combination of the facts the query cannot know, prints the chosen kernel, and exposes split_search and
wg_reduce_group (which reducer adds the partial slabs), each compared with the rule written down again here."""
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
import gen_wgrad_route_golden as gen  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "wgrad_route_parent.json")))
ROWS = [dict(zip(GOLDEN["columns"], r)) for r in GOLDEN["rows"]]
TN_KERNELS = ("tn_lds", "tn_wide", "tn_direct", "tn_direct_tail")


def test_the_case_table_is_the_generators():
    assert GOLDEN["envs"] == gen.ENVS
    assert [{k: r[k] for k in gen.COLUMNS} for r in ROWS] == gen.cases()


@pytest.fixture(scope="module")
def answers():
    return gen.answers(_lib, ROWS)


def test_profiling_label_is_the_parents_on_every_row(answers):
    assert [a[1] for a in answers] == [r["route_answer"] for r in ROWS]
    assert sum(a[1] for a in answers) > 10                    # (the split-bf16 route is really among the rows)


def test_workspace_query_never_asks_for_more_than_the_parent(answers):
    larger = [(r, a[0]) for r, a in zip(ROWS, answers) if a[0] > r["ws"]]
    assert not larger, larger[:5]
    # where it asks for less (profiles/wgrad_route/README.md lists them): only under MSS_WGRAD_TN=7, where a channel slice of dy no
    # longer falls back to conv_wgrad_kernel
    assert all(GOLDEN["envs"][r["env"]] == {"MSS_WGRAD_TN": "7"} for r, a in zip(ROWS, answers) if a[0] < r["ws"])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("wgrad_route") / "wgrad_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "wgrad_route_check.cpp"), "-o", exe], check=True)
    return exe


def _switches(r):
    env = GOLDEN["envs"][r["env"]]
    return [int(env.get(k, d)) for k, d in (("MSS_WGRAD_TN", 5), ("MSS_WGRAD_NARROW", 1), ("MSS_WGRAD_TN_AFFINE", 1), ("MSS_WGRAD_TN_TAIL", 1))]


@pytest.fixture(scope="module")
def routes(checker):
    """(row, printed fields) of every row: the checker has then passed all its properties on all of them."""
    text = "".join(" ".join(map(str, [r[k] for k in gen.COLUMNS[:-1]] + _switches(r))) + "\n" for r in ROWS)
    p = subprocess.run([checker], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(ROWS)
    return [(r, ln.split()) for r, ln in zip(ROWS, lines)]


def test_every_kernel_is_reached_and_the_header_agrees_with_the_library(routes, answers):
    seen = {f[0] for _, f in routes}
    assert seen == {"conv32", "conv64", "conv128", "narrow", "tn_lds", "tn_wide", "tn_direct", "tn_direct_tail", "tn_direct_perimg", "two_part"}
    for (r, f), a in zip(routes, answers):
        if not r["route"]:                      # (the checker is not offered the split-bf16 route)
            assert int(f[7]) == a[0], (r, f, a)


def test_named_step_shapes_get_the_documented_kernels(routes):
    # DESIGN 3.18 / the comments of wgrad_route.h, default switches, native route
    want = {(2304, 4096, 256, 64): "tn_direct",          # ASPP F(6x6): 4096 tiles, four whole rounds
            (5184, 4096, 256, 36): "tn_direct_tail",     # ASPP F(4x4): 2304 tiles = 2048 whole + 256 x 4
            (29412, 256, 256, 64): "tn_direct",          # decoder F(6x6)
            (162624, 256, 256, 1): "tn_direct", (162624, 1024, 256, 1): "tn_direct", (162624, 256, 1024, 1): "tn_direct",
            (10164, 256, 256, 1): "tn_lds",              # one image: 156 one-wave jobs are too few
            (65536, 4096, 256, 1): "tn_direct", (32768, 1280, 256, 1): "tn_direct",
            (162624, 256, 288, 1): "two_part",
            (2592, 4096, 256, 72): "tn_direct_perimg", (1152, 4096, 256, 128): "tn_direct_perimg"}
    found = 0
    for r, f in routes:
        key = (r["M"], r["C"], r["K"], r["batch"])
        if r["env"] == 0 and not r["route"] and key in want and r["Kpad"] == gen.kpad(r["K"]):
            assert f[0] == want[key], (r, f)
            found += 1
            if f[0] == "two_part":               # 256 channels on the LDS-free kernel (it takes the row stride), 32 on the narrow one
                assert f[6] == "256" and f[8:] == ["tn_direct", "narrow"]
            if key == (5184, 4096, 256, 36):
                assert (f[1], f[3], f[4]) == ("4", "3072", "2048")
    assert found >= len(want)
    # the two-part GPU test's shapes (tests/test_gpu_ops.py): the same kernels for a channel slice of dy and for its contiguous copy
    parts = {(r["K"], r["lddy"]): f[8:] for r, f in routes if r["M"] == 16385 and not r["route"]}
    assert parts == {(Ko, ld): ["conv128", "narrow"] for Ko in (160, 192) for ld in (Ko, 256)}


def test_forcing_switches_give_the_kernel_they_document(routes):
    for r, f in routes:
        env = GOLDEN["envs"][r["env"]]
        kernels = [f[0]] if f[0] != "two_part" else f[8:]
        tn = env.get("MSS_WGRAD_TN")
        plain = r["R"] == 1 and r["ldx"] == r["C"] and r["lddy"] == r["K"] and not r["affine"] and not r["k_imgs"] and r["K"] % 4 == 0
        tn_shape = plain and (r["batch"] > 1 or (r["K"] >= 128 and r["C"] >= 128))
        if tn == "0":
            assert not set(kernels) & set(TN_KERNELS), (r, f)
        if tn == "1" and tn_shape and f[0] != "two_part":
            assert f[0] == "tn_lds", (r, f)
        if tn == "4" and tn_shape and f[0] != "two_part":
            assert f[0] == ("tn_wide" if r["C"] % 256 == 0 else "tn_lds"), (r, f)
        if tn == "7" and tn_shape and r["K"] % 128 == 0 and r["C"] % 128 == 0:
            assert f[0] in ("tn_direct", "tn_direct_tail"), (r, f)
        if env.get("MSS_WGRAD_NARROW") == "0":
            assert "narrow" not in kernels and f[0] != "two_part", (r, f)
        if env.get("MSS_WGRAD_TN_AFFINE") == "0" and r["affine"]:
            assert not set(kernels) & set(TN_KERNELS), (r, f)
        if env.get("MSS_WGRAD_TN_TAIL") == "0":
            assert "tn_direct_tail" not in kernels, (r, f)


def _split_search(base, slots, cap):
    splits, best = 1, 0.0
    for sp in range(1, cap + 1):
        total = base * sp
        eff = total / (-(-total // slots) * slots)
        if eff > best + 1e-9:
            best, splits = eff, sp
        if eff >= 0.95 and total >= slots:
            break
    return splits


@pytest.mark.parametrize("cap", [1, 16, 64, 256, 1024])
def test_split_search_is_the_rule(checker, cap):
    got = [int(v) for v in subprocess.run([checker, "split", str(cap)], capture_output=True, text=True, check=True).stdout.split()]
    want = [_split_search(base, slots, cap) for slots in (512, 768, 1024) for base in range(1, 5001)]
    assert got == want


REDUCE_SLAB4 = [1, 304, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, 65535, 65536, 65537,
                73728, 1048576, 1 << 33]


def reduce_group(slab4, splits):
    """The rule of wg_reduce_group: the largest power of two G <= 32 such that, for every doubling on the way to it, the threads so far
    (one per output float4 and lane: slab4 * G / 2) are fewer than 65536 and every lane keeps at least 4 splits (splits >= 4 G)."""
    g = 1
    while g < 32 and slab4 * g < 65536 and splits >= 8 * g:
        g *= 2
    return g


def test_reduce_group_is_the_rule(checker):
    got = [int(v) for v in subprocess.run([checker, "reduce"], capture_output=True, text=True, check=True).stdout.split()]
    want = [reduce_group(slab4, splits) for slab4 in REDUCE_SLAB4 for splits in range(1, 601)]
    assert got == want
    assert set(want) == {1, 2, 4, 8, 16, 32}
    # the shapes the header's comments name: 1536 splits of the 19 x 256 head slab (20 KB) on 32 lanes, 256 splits of a 256 x 256
    # Linear (256 KB) on 4, anything of 64 k float4s or more, or fewer than 8 splits, on the sequential kernel
    assert reduce_group(20 * 256 // 4, 1536) == 32 and reduce_group(256 * 256 // 4, 256) == 4
    assert reduce_group(65536, 1024) == 1 and reduce_group(16, 7) == 1
