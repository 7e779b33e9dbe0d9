"""CPU: the object bank's arithmetic and its host side.
  * the numpy restatement (tests/ref_object_bank.py) returns the source at scale 1.0 and the exact 2 x 2 mean at scale 0.5 on even
    sizes, and stays within 8 * 2^-24 * 255 of its own float64 form on the sizes the GPU test uses;
  * the nearest mapping at scale 0.5 keeps even source rows and columns only: a single valid pixel at an odd row or column of a
    12 x 12 mask gives the empty box, the one at (4, 6) gives (2, 3, 3, 4);
  * csrc/mss_cv_resize.h, the one definition the kernels use, compiled with g++ into a stand-alone program -- once plain, once with
    -fsanitize=address,undefined -- reproduces the restatement's index and fraction for every destination index, bit for bit;
  * with a bank (anything with __len__ and bbox) both draw functions make the draws of the host-object path: the same p, top, left,
    h0, w0 and box size, and the generator is left in the same state.
"""
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import ref_object_bank as R
from conftest import ROOT

SCALES = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
SIZES = [(10, 10), (13, 17), (37, 64), (64, 37), (100, 130), (480, 640)]


def _image(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("H,W", SIZES[:5])
def test_scale_one_returns_the_source(H, W):
    img = _image(H, W)
    assert np.array_equal(R.linear(img, H, W), img.astype(np.float32))
    assert np.array_equal(R.nearest(img[..., 0], H, W), img[..., 0])


@pytest.mark.parametrize("H,W", [(10, 10), (38, 64), (100, 130)])
def test_scale_half_on_even_sizes_is_the_exact_2x2_mean(H, W):
    img = _image(H, W, 1)
    want = img.astype(np.float64).reshape(H // 2, 2, W // 2, 2, 3).mean(axis=(1, 3))
    got = R.linear(img, H // 2, W // 2)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


def test_float32_sequence_stays_near_its_float64_form():
    worst = 0.0
    for k, (H, W) in enumerate(SIZES):
        img = _image(H, W, 10 + k)
        for s in SCALES:
            sh, sw = R.scaled_size(H, W, s)
            worst = max(worst, float(np.abs(R.linear(img, sh, sw).astype(np.float64) - R.linear_f64(img, sh, sw)).max()))
    # two rounded products and one rounded sum per pass, two passes, plus the two rounded 1 - f: eight roundings, each at most
    # 2^-24 relative, on values <= 255. These images give 3.4e-5, about a quarter of the bound.
    print(f"max |float32 - float64| = {worst:.3e}")
    assert worst <= 8 * 2.0 ** -24 * 255


def test_single_pixel_masks_at_scale_half():
    def box(y, x):
        m = np.zeros((12, 12), dtype=np.uint8)
        m[y, x] = 7
        return R.bbox(R.nearest(m, *R.scaled_size(12, 12, 0.5)))
    assert box(4, 6) == (2, 3, 3, 4)
    assert box(5, 6) == box(4, 7) == box(5, 7) == (0, 0, 0, 0)
    m = np.full((12, 12), 255, dtype=np.uint8)
    m[0, 0] = 0
    assert R.bbox(m) == (0, 0, 0, 0)                      # 0 and 255 are both invalid


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mss_cv_resize.h"

int main(int argc, char** argv) {
  for (int k = 1; k + 1 < argc; k += 2) {
    const int src = atoi(argv[k]), dst = atoi(argv[k + 1]);
    const double scale = cv_scale(src, dst);
    for (int d = 0; d < dst; ++d) {
      const CvTap t = cv_linear(d, scale, src);
      unsigned bits;
      memcpy(&bits, &t.f, 4);
      printf("%d %d %d %d %d %d %u\n", src, dst, d, cv_nearest(d, scale, src), t.i0, t.i1, bits);
    }
  }
  return 0;
}
"""


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_coordinate_header_reproduces_the_restatement_in_a_stand_alone_program(tmp_path, flags):
    pairs = sorted({(n, R.scaled_size(n, n, s)[0]) for hw in SIZES for n in hw for s in SCALES} | {(1, 1), (2, 1), (3, 2), (7, 3)})
    src, exe = tmp_path / "cv_resize.cpp", tmp_path / "cv_resize"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", os.path.join(ROOT, "multishiftseg_amd", "csrc"), str(src), "-o",
                    str(exe)], check=True)
    run = subprocess.run([str(exe)] + [str(v) for p in pairs for v in p], capture_output=True, text=True, check=True)
    got = np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()], dtype=np.int64)
    want = []
    for s, d in pairs:
        i0, i1, f = R.linear_taps(s, d)
        want.append(np.stack([np.full(d, s), np.full(d, d), np.arange(d), R.nearest_index(s, d), i0, i1, f.view(np.uint32).astype(np.int64)], axis=1))
    want = np.concatenate(want)
    assert got.shape == want.shape and len(pairs) > 80
    bad = np.where((got != want).any(axis=1))[0]
    assert bad.size == 0, (got[bad[:5]], want[bad[:5]])
    assert (want[:, 4] >= 0).all() and (want[:, 5] < want[:, 0]).all() and (want[:, 3] < want[:, 0]).all()      # every tap in range


def _objects(seed=3):
    """Small host objects: masks with valid bytes inside, one object without any valid byte."""
    rng = np.random.default_rng(seed)
    objs = []
    for k, (H, W) in enumerate([(10, 10), (13, 17), (20, 30), (12, 12)]):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        mask = np.zeros((H, W), dtype=np.uint8)
        if k != 3:
            mask[H // 4: H - 1, 1: W - W // 4] = rng.choice(np.array([0, 7, 254, 255], dtype=np.uint8), (H - 1 - H // 4, W - W // 4 - 1))
        objs.append((img, mask))
    return objs


def _same_draws(draw):
    objs = _objects()
    for seed in range(40):
        r_host, r_bank = random.Random(seed), random.Random(seed)
        torch.manual_seed(seed)
        host = draw(objs, R.scaled_object, r_host)
        torch.manual_seed(seed)
        bank = draw(R.StubBank(objs), None, r_bank)
        assert r_host.getstate() == r_bank.getstate(), seed
        for key in ("p", "top", "left"):
            assert host[key] == bank[key], (seed, key)
        assert "obj_img" not in bank and "obj_mask" not in bank
        index, scale = bank["pick"]
        assert host["obj_mask"].shape == R.scaled_size(*objs[index][1].shape, scale)
        assert bank["geom"][:2] == (0, 0) and bank["geom"][2:] == host["geom"][2:], (seed, host["geom"], bank["geom"])
        if "entries" in host:
            assert host["entries"] == bank["entries"] and host["size"] == bank["size"]


def test_bank_draws_match_the_host_object_draws_deeplab():
    from multishiftseg_amd import datapath as D
    _same_draws(lambda objs, cb, rng: D.draw_sample_params(96, 128, (64, 64), True, objs, cb, rng=rng))


@pytest.mark.parametrize("chain", ["default", "three"])
def test_bank_draws_match_the_host_object_draws_m2f(chain):
    from multishiftseg_amd import m2f_datapath as M
    ch = M.M2F_CHAIN if chain == "default" else (("ToTensor", 1.0), ("RandCrop", 1.0), ("Normalize", 1.0))
    _same_draws(lambda objs, cb, rng: M.draw_m2f_sample_params(96, 128, (48, 48), True, objs, cb, rng=rng, chain=ch))


def test_a_pick_without_a_bank_and_a_mixed_batch_raise():
    from multishiftseg_amd import datapath as D
    objs = _objects()
    picked = D.draw_sample_params(96, 128, (64, 64), True, R.StubBank(objs), rng=random.Random(0))
    hosted = D.draw_sample_params(96, 128, (64, 64), True, objs, R.scaled_object, rng=random.Random(0))
    with pytest.raises(ValueError, match="bank"):
        D.bank_objects([picked, picked], None)
    with pytest.raises(ValueError, match="either"):
        D.bank_objects([picked, hosted], object())
    assert D.bank_objects([hosted, hosted], None) is None


def test_the_bank_has_no_cpu_path():
    from multishiftseg_amd.object_bank import ObjectBank, scaled_size
    with pytest.raises(RuntimeError, match="no CPU path"):
        ObjectBank(_objects(), device="cpu")
    with pytest.raises(ValueError):
        scaled_size(5, 20, 0.1)                           # int(5 * 0.1) = 0 rows: cv2 raises there too
