"""CPU: the align_corners=True coordinate function and its inverse (csrc/mss_bilinear_ac.h), the one definition that the kernels
of csrc/m2f_ood_loss.hip use, compiled into a stand-alone host program with g++ -- once plain, once with
-fsanitize=address,undefined -- and run. For every (in, out) in 1..9 x 1..33, and a few sizes a user runs:
  * the taps of every output index lie in 0..in-1, i1 is i0 or i0 + 1, 0 <= l < 1 (at the last output the rounded coordinate may
    exceed in - 1 by an ulp: then i1 == i0 and both weights fall on that tap, as in ATen);
  * i0 + l is within in * 2^-23 of the exact rational dst (in - 1) / (out - 1) (0 for out == 1): one rounding of the scale and one
    of the product, each at most 2^-24 relative, of a value below in;
  * every output index that has source index i as a tap lies inside ac_candidates(i), the range the backward kernel walks.
"""
import os
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "mss_bilinear_ac.h"

static int failures = 0;
static void fail(const char* what, int in, int out, int dst, int i) {
  if (++failures <= 20) printf("FAIL %s: in %d out %d dst %d i %d\n", what, in, out, dst, i);
}

static void check(int in, int out) {
  const float scale = ac_scale(in, out);
  AcCoord* c = (AcCoord*)malloc(sizeof(AcCoord) * out);         // exactly `out` entries: the sanitizer sees an index outside
  for (int dst = 0; dst < out; ++dst) {
    c[dst] = ac_coord(dst, scale, in);
    const AcCoord k = c[dst];
    if (k.i0 < 0 || k.i0 > in - 1 || k.i1 < k.i0 || k.i1 > k.i0 + 1 || k.i1 > in - 1) fail("taps", in, out, dst, k.i0);
    if (!(k.l >= 0.f && k.l < 1.f)) fail("weight", in, out, dst, k.i0);
    const double exact = out > 1 ? (double)dst * (double)(in - 1) / (double)(out - 1) : 0.0;
    const double got = (double)k.i0 + (double)k.l, bound = (double)in / 8388608.0;
    if (!(got - exact <= bound && exact - got <= bound)) fail("coordinate", in, out, dst, k.i0);
  }
  int* seen = (int*)calloc(in, sizeof(int));
  for (int i = 0; i < in; ++i) {
    int lo, hi;
    ac_candidates(i, scale, out, &lo, &hi);
    if (lo < 0 || hi > out - 1) fail("range outside the output", in, out, lo, i);
    for (int dst = 0; dst < out; ++dst) {
      float wgt;
      if (!ac_tap_weight(c[dst], i, &wgt)) continue;
      seen[i] = 1;
      if (dst < lo || dst > hi) fail("a tap outside the candidate range", in, out, dst, i);
      if (!(wgt >= 0.f && wgt <= 1.f)) fail("tap weight", in, out, dst, i);
    }
  }
  if (out >= in)                                                 // growing or identity: every source index is somebody's tap
    for (int i = 0; i < in; ++i)
      if (!seen[i]) fail("a source index without any output", in, out, -1, i);
  free(seen);
  free(c);
}

int main() {
  long pairs = 0;
  for (int in = 1; in <= 9; ++in)
    for (int out = 1; out <= 33; ++out, ++pairs) check(in, out);
  const int extra[][2] = {{176, 704}, {704, 176}, {177, 701}, {1, 2048}, {2048, 1}, {2, 100000}, {100000, 2}, {1024, 2048}, {3, 1000003}};
  for (unsigned k = 0; k < sizeof(extra) / sizeof(extra[0]); ++k, ++pairs) check(extra[k][0], extra[k][1]);
  printf("%ld size pairs, %d failures\n", pairs, failures);
  return failures ? 1 : 0;
}
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]], ids=["plain", "asan_ubsan"])
def test_coordinates_and_candidate_ranges_in_a_stand_alone_program(tmp_path, flags):
    src, exe = tmp_path / "bilinear_ac.cpp", tmp_path / "bilinear_ac"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "multishiftseg_amd", "csrc"), str(src), "-o",
                    str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"{9 * 33 + 9} size pairs, 0 failures")
