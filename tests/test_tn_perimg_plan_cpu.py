"""The packed job plan of the per-image TN weight gradient (csrc/tn_perimg_plan.h) on the host: a stand-alone program
(tests/tn_perimg_plan_check.cpp, its own main, built with the host compiler's address and undefined-behaviour sanitizers) decodes
every job number of the worst-case grid and checks that the live tiles are covered exactly -- whole tiles once, tail tiles once per
row range, the ranges a partition of the rows -- and that every number at or behind the plan's total is rejected. The plan's figures
are compared with the rule written down again here."""
import os
import re
import shutil
import subprocess

import pytest

from multishiftseg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multishiftseg_amd", "csrc")


def _cdiv(a, b):
    return -(-a // b)


def expected_plan(P, k_imgs, ktiles, ctiles, k_base, slots, rows, want_tail, k_steps):
    """tn_plan_direct's tail rule on the live tiles: (S, live, full, tail, splits, tps, total, worst)."""
    L = [min(ctiles, max(0, _cdiv(16 * (k_base + k), 128))) for k in k_steps]
    S = ktiles * sum(L)
    live = P * S
    worst = P * k_imgs * ktiles * ctiles
    worst += slots if want_tail and worst > slots else 0
    none = (S, live, live, 0, 1, rows, live, worst)
    if not want_tail or live <= slots or live % slots == 0 or live / (_cdiv(live, slots) * slots) >= 0.95:
        return none
    tail = live % slots
    ts = min(slots // tail, _cdiv(rows, 256), 16)
    if ts < 2:
        return none
    tps = _cdiv(_cdiv(rows, ts), 2) * 2
    splits = _cdiv(rows, tps)
    return (S, live, live - tail, tail, splits, tps, live - tail + tail * splits, worst)


# (P, k_imgs, ktiles, ctiles, k_base, slots, rows, want_tail, k_steps)
CASES = [
    # the step's shapes: L = 24 / 25 of 32 c tiles
    (64, 2, 2, 32, 128, 1024, 1152, 1, [64, 64]),             # L equal, 6144 live = 6 whole rounds: no tail
    (64, 2, 2, 32, 128, 1024, 1152, 1, [64, 65]),             # extent a multiple of 128, and one 16-column step over: 6272 = 6 rounds + 128 x 5
    (64, 2, 2, 32, 128, 1024, 1152, 1, [65, 65]),
    (36, 2, 2, 32, 128, 1024, 2592, 1, [64, 65]),             # 3528 = 3 rounds + 456 x 2
    (36, 2, 2, 32, 128, 1024, 2592, 0, [64, 65]),             # the same without scratch: whole tiles only
    (64, 2, 2, 32, 128, 1024, 1152, 1, [128, 128]),           # everything kept: L = ctiles
    (64, 2, 2, 32, 128, 1024, 1152, 1, [128, 3]),             # L mixed: everything and the minimum
    (64, 2, 2, 32, 128, 1024, 1152, 1, [200, 3]),             # k_steps past the pitch: clamped to ctiles
    # small shapes (the GPU test's), k_imgs = 1, 2, 3 and 16
    (36, 1, 1, 2, 8, 32, 600, 1, [3]),
    (36, 2, 1, 2, 8, 64, 600, 1, [4, 8]),
    (36, 3, 2, 6, 8, 128, 600, 1, [3, 40, 21]),
    (36, 3, 2, 6, 8, 128, 200, 1, [3, 40, 21]),               # 200 rows: a single 256-row range, no split possible
    (4, 16, 1, 4, 8, 64, 700, 1, [3, 8, 9, 16, 17, 24, 3, 5, 11, 24, 24, 8, 7, 6, 23, 19]),
    # live below, equal to, just over the slots, and a multiple of them
    (5, 2, 1, 4, 0, 64, 600, 1, [24, 24]),                    # 40 < 64
    (8, 2, 1, 4, 0, 64, 600, 1, [32, 32]),                    # 64 == slots
    (13, 1, 1, 5, 0, 64, 600, 1, [40]),                       # 65: one tail tile, splits capped by ceil(rows / 256) = 3
    (16, 2, 1, 4, 0, 64, 600, 1, [32, 32]),                   # 128 = 2 x slots
    (31, 1, 2, 1, 0, 64, 600, 1, [8]),                        # 62: below
    (61, 1, 1, 2, 0, 64, 5000, 1, [9]),                       # 122 = 0.953 of two rounds: fill >= 0.95, no tail
    (35, 1, 1, 2, 0, 64, 5000, 1, [9]),                       # 70: tail 6, splits capped at 16 (10 by slots / tail)
    (33, 1, 1, 2, 0, 64, 5000, 1, [9]),                       # 66: tail 2, slots / tail = 32 -> 16 splits
    (36, 2, 1, 2, 8, 64, 601, 1, [4, 8]),                     # odd row count
]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tn_perimg_plan") / "tn_perimg_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "tn_perimg_plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_every_job_of_the_worst_case_grid_decodes_to_exactly_the_live_tiles(checker):
    text = "".join(" ".join(map(str, c[:8] + tuple(c[8]))) + "\n" for c in CASES)
    r = subprocess.run([checker], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(CASES)
    taken = 0
    for c, ln in zip(CASES, lines):
        got = tuple(int(v) for v in ln.split()[1:])
        assert got == expected_plan(*c), (c, got, expected_plan(*c))
        taken += got[3] > 0
    assert taken >= 8                                          # the tail plan is really among the cases


def test_the_step_shapes_give_the_estimated_rounds():
    # 6272 live jobs = 6 rounds + 128 tiles in 5 row ranges; d = 36: 3528 = 3 rounds + 456 tiles halved
    assert expected_plan(*CASES[1])[1:7] == (6272, 6144, 128, 5, 232, 6784)
    assert expected_plan(*CASES[3])[1:7] == (3528, 3072, 456, 2, 1296, 3984)


def test_workspace_constant_matches_the_header_and_the_plan():
    hdr = open(os.path.join(ROOT, "include", "mss_hip.h")).read()
    m = re.search(r"#define MSS_WGRAD_PERIMG_TAIL_BYTES \(1024ll \* 128 \* 128 \* 4\)", hdr)
    assert m and _lib.MSS_WGRAD_PERIMG_TAIL_BYTES == 1024 * 128 * 128 * 4
    plan = open(os.path.join(CSRC, "tn_perimg_plan.h")).read()
    assert int(re.search(r"#define TN_PERIMG_MAX_SLOTS (\d+)", plan).group(1)) * 128 * 128 * 4 == _lib.MSS_WGRAD_PERIMG_TAIL_BYTES
