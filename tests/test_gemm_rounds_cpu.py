"""The round arithmetic of gemm_nt_kernel's dense launches (csrc/gemm_rounds.h) on the host: a stand-alone program
(tests/gemm_rounds_check.cpp, its own main, built with the host compiler's address and undefined-behaviour sanitizers) walks the tile
ranges of every plan as gemm.hip launches them and checks that the wide and narrow ranges cover every output tile exactly once. The
plans are compared with the rule written down again here: the hybrid of one wide round plus at most one narrow round fires only for
single-position products between one and two wide rounds, and MSS_GEMM_TAIL=0 gives the plan from before that rule."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multishiftseg_amd", "csrc")

NARROW, WIDE, HYBRID = 0, 1, 2


def _fill(total, slots):
    return total / (-(-total // slots) * slots)


def parent_plan(mtiles, K, C, batch, tail):
    """(mode, full, rem) of the launch rule before the mid-rounds class: wide from two rounds of 512 slots up unless the narrow
    tiles fill their rounds much better, its last round on narrow tiles by MSS_GEMM_TAIL."""
    if K % 256 or C < 256:
        return NARROW, 0, 0
    t = mtiles * (K // 256) * max(batch, 1)
    if t < 1024:
        return NARROW, 0, 0
    ew, en = _fill(t, 512), _fill(2 * t, 768)
    if ew < 0.8 and en > ew + 0.15:
        return NARROW, 0, 0
    full = t // 512 * 512
    rem = t - full
    rem_max = 384 if tail == 1 or (tail == -1 and batch <= 1 and full <= 2048) else 0
    if 0 < rem <= rem_max:
        return HYBRID, full, rem
    return WIDE, 0, 0


def in_mid_class(mtiles, K, C, batch):
    t = mtiles * (K // 256) * max(batch, 1)
    return K % 256 == 0 and C >= 256 and batch <= 1 and 512 < t < 1024 and t - 512 <= 384


def expected_plan(mtiles, K, C, batch, tail):
    if tail != 0 and in_mid_class(mtiles, K, C, batch):
        return HYBRID, 512, mtiles * (K // 256) - 512
    return parent_plan(mtiles, K, C, batch, tail)


MTILES = [1, 31, 32, 33, 36, 55, 56, 57, 63, 64, 65, 87, 128, 129, 224, 225, 256, 257, 347, 448, 449, 512, 513, 896, 897, 1024, 1271, 2304]
GRID = [c for c in itertools.product(MTILES, [128, 256, 304, 512, 1024, 2048, 4096], [128, 256, 4096], [0, 1, 2, 64], [-1, 0, 1])
        if c[0] * -(-c[1] // 128) * max(c[3], 1) <= 120000]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("gemm_rounds") / "gemm_rounds_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "gemm_rounds_check.cpp"), "-o", exe], check=True)
    text = "".join(" ".join(map(str, c)) + "\n" for c in GRID)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr                       # every tile of every case covered exactly once
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(GRID)
    return {c: tuple(int(v) for v in ln.split()[1:]) for c, ln in zip(GRID, lines)}


def test_plans_are_the_rule_and_the_new_class_fires_only_inside_it(plans):
    fired = 0
    for c, (mode, t256, full, rem, g1, g2) in plans.items():
        assert (mode, full, rem) == expected_plan(*c), (c, (mode, full, rem), expected_plan(*c))
        new = (mode, full, rem) != parent_plan(*c)
        assert new == (c[4] != 0 and in_mid_class(*c[:4])), c
        if new:
            assert mode == HYBRID and full == 512 and 0 < rem <= 384 and (g1, g2) == (512, min(2 * rem, 768)), (c, g1, g2)
        fired += new
    assert fired >= 20                                         # the class is really among the cases


def test_tail_mode_0_is_the_plan_from_before_the_rule(plans):
    for c, (mode, t256, full, rem, g1, g2) in plans.items():
        if c[4] == 0:
            assert (mode, full, rem) == parent_plan(*c) and mode != HYBRID, c


def test_the_composed_aspp_products_run_one_wide_and_one_narrow_round(plans):
    # 7168 x 4096 -> 4096: 56 x 16 = 896 wide tiles = 512 + 384 -> 768 narrow tiles, every slot of both launches filled once
    assert plans[(56, 4096, 4096, 0, -1)] == (HYBRID, 896, 512, 384, 512, 768)
    assert plans[(56, 4096, 4096, 0, 0)][0] == NARROW
    # 4603 rows: 36 x 16 = 576 wide tiles, a short tail
    assert plans[(36, 4096, 256, 1, -1)] == (HYBRID, 576, 512, 64, 512, 128)
    # exactly one round, two rounds and the first shape over 512 + 384 stay what they were
    for c in [(32, 4096, 4096, 0, -1), (64, 4096, 4096, 0, -1), (57, 4096, 4096, 0, -1), (56, 4096, 4096, 2, -1), (56, 4096, 128, 0, -1)]:
        assert (plans[c][0], plans[c][2], plans[c][3]) == parent_plan(*c), c
