// Bilinear interpolation with align_corners=False, shared by every kernel that restates F.interpolate(mode="bilinear") of the
// Mask2Former chain (csrc/m2f.hip, csrc/m2f_attn.hip, csrc/m2f_mix.hip): one definition of the source coordinate, so that all
// of them pick the same taps and the same weight for an output pixel.
#pragma once
#include "mss_common.h"

struct SrcCoord { int i0, i1; float l; };
// F.interpolate(mode="bilinear", align_corners=False): src = (dst + 0.5) * in/out - 0.5, clamped at 0
__device__ __forceinline__ SrcCoord src_coord(int dst, float scale, int in_size) {
  float s = ((float)dst + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  SrcCoord c;
  c.i0 = (int)s;
  if (c.i0 > in_size - 1) c.i0 = in_size - 1;
  c.i1 = c.i0 + (c.i0 < in_size - 1 ? 1 : 0);
  c.l = s - (float)c.i0;
  return c;
}

// ATen's scale of upsample_bilinear2d when no scale_factor is given: in / out, rounded to float once
static inline float mss_bilinear_scale(int in, int out) { return (float)in / (float)out; }
