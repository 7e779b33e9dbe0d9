// Bilinear interpolation with align_corners=True as ATen's upsample_bilinear2d computes it in float, and its inverse: which
// output indices can have a given source index among their two taps. One definition for the kernels of csrc/m2f_ood_loss.hip and
// for the stand-alone host program of tests/test_bilinear_ac_cpu.py: this header needs no HIP and compiles with a plain C++ compiler.
// (align_corners=False lives in mss_bilinear.h: src_coord.)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MSS_AC_HD __host__ __device__ __forceinline__
#else
#define MSS_AC_HD static inline
#endif

struct AcCoord { int i0, i1; float l; };

// ATen's area_pixel_compute_scale with align_corners: (in - 1) / (out - 1), rounded to float once; 0 for a single output
MSS_AC_HD float ac_scale(int in_size, int out_size) { return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f; }

// src = scale * dst rounded to float BEFORE the subtraction (area_pixel_compute_source_index); i0 = (int)src, i1 = i0 + (i0 < in - 1),
// l = src - i0. The clamp of i0 never acts for a scale made by ac_scale and 0 <= dst < out; it keeps the taps in range for any caller.
MSS_AC_HD AcCoord ac_coord(int dst, float scale, int in_size) {
  float src = scale * (float)dst;
  // -ffp-contract=fast would fuse the product into `src - i0` below (fma(scale, dst, -i0)): pin the rounded product
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(src));
#else
  volatile float pinned = src;
  src = pinned;
#endif
  AcCoord c;
  c.i0 = (int)src;
  if (c.i0 > in_size - 1) c.i0 = in_size - 1;
  c.i1 = c.i0 + (c.i0 < in_size - 1 ? 1 : 0);
  c.l = src - (float)c.i0;
  return c;
}

// The output indices lo..hi (inclusive, inside 0..out-1) among which every dst with ac_coord(dst).i0 == i or .i1 == i lies. A tap
// means fl(scale dst) in [i - 1, i + 1), so scale dst lies within a factor 1 +- 2^-24 of that interval; the quotients are taken in
// double, widened by 2^-22 of themselves and by one index on either side. Only a superset is promised: the caller checks every
// candidate against ac_coord itself. scale == 0 (one output, or one input): every output is a candidate.
MSS_AC_HD void ac_candidates(int i, float scale, int out_size, int* lo, int* hi) {
  *lo = 0;
  *hi = out_size - 1;
  if (!(scale > 0.f)) return;
  const double a = ((double)i - 1.0) / (double)scale, z = ((double)i + 1.0) / (double)scale;
  const double lo_d = floor(a - fabs(a) * (1.0 / 4194304.0)) - 1.0, hi_d = ceil(z + z * (1.0 / 4194304.0)) + 1.0;
  if (lo_d > 0.0) *lo = lo_d < (double)out_size ? (int)lo_d : out_size;       // lo > hi: no candidate
  if (hi_d < (double)(out_size - 1)) *hi = (int)hi_d;
}

// the weight of source index i in an output with coordinate c, and whether i is one of its taps at all
MSS_AC_HD bool ac_tap_weight(const AcCoord& c, int i, float* wgt) {
  *wgt = (c.i0 == i ? 1.f - c.l : 0.f) + (c.i1 == i ? c.l : 0.f);
  return c.i0 == i || c.i1 == i;
}
