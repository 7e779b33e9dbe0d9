// point_sample of detectron2 (F.grid_sample(2u - 1, bilinear, align_corners=False, zero padding)) as the Mask2Former matcher and
// criterion use it: shared by m2f_match.hip and m2f_loss.hip, so that both sample a point with the same arithmetic.
#pragma once
#include "mss_common.h"

struct PointTap { int x0, y0; float fx, fy; };

// pixel coordinate of F.grid_sample(2u - 1, align_corners=False): u n - 0.5. Clamped to [-2, n + 1] (every tap of a clamped
// coordinate lies outside the map, as it did before the clamp), which also turns a NaN into -2: the integer taps stay defined.
__device__ __forceinline__ void point_tap(float u, int n, int& i0, float& f) {
  float c = __builtin_fmaf(u, (float)n, -0.5f);
  c = fminf(fmaxf(c, -2.f), (float)n + 1.f);
  const float fl = floorf(c);
  i0 = (int)fl;
  f = c - fl;
}

template <typename T>
__device__ __forceinline__ float bilinear_zero(const T* base, long long ps, int h, int w, const PointTap& t) {
  const bool xa = t.x0 >= 0 && t.x0 < w, xb = t.x0 + 1 >= 0 && t.x0 + 1 < w;
  const bool ya = t.y0 >= 0 && t.y0 < h, yb = t.y0 + 1 >= 0 && t.y0 + 1 < h;
  const long long o = ((long long)t.y0 * w + t.x0) * ps;
  const float v00 = xa && ya ? (float)base[o] : 0.f;
  const float v01 = xb && ya ? (float)base[o + ps] : 0.f;
  const float v10 = xa && yb ? (float)base[o + (long long)w * ps] : 0.f;
  const float v11 = xb && yb ? (float)base[o + (long long)w * ps + ps] : 0.f;
  const float gx = 1.f - t.fx, gy = 1.f - t.fy;
  return v00 * (gx * gy) + v01 * (t.fx * gy) + v10 * (gx * t.fy) + v11 * (t.fx * t.fy);
}
