// The destination-to-source coordinates of cv2.resize as the reference's random_scale calls it (lib/utils/img_utils.py:345-352):
// INTER_NEAREST for the object mask, INTER_LINEAR for the object image. One definition for the kernels of csrc/obj_bank.hip and
// for the stand-alone host program of tests/test_object_bank_cpu.py: this header needs no HIP and compiles with a plain C++
// compiler. The rules, for a source extent `src` resized to `dst`, all in double unless a cast is written:
//   inv = (double)dst / src, scale = 1.0 / inv
//   nearest:  s = min((int)floor(d * scale), src - 1)
//   linear:   f = (float)((d + 0.5) * scale - 0.5); s = (int)floor(f); f = f - (float)s;
//             s < 0 -> s = 0, f = 0;  s >= src - 1 -> s = src - 1, f = 0 (the second tap is then the same pixel)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MSS_CV_HD __host__ __device__ __forceinline__
#else
#define MSS_CV_HD static inline
#endif

struct CvTap { int i0, i1; float f; };          // taps i0 <= i1 <= i0 + 1, weight 1 - f on i0 and f on i1

// a rounded double that the compiler may not fuse into the operation that follows (-ffp-contract=fast is hipcc's default)
MSS_CV_HD double cv_pin(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
  return v;
#else
  volatile double pinned = v;
  return pinned;
#endif
}

MSS_CV_HD double cv_scale(int src, int dst) {
  const double inv = (double)dst / (double)src;
  return 1.0 / inv;
}

MSS_CV_HD int cv_nearest(int d, double scale, int src) {
  const int s = (int)floor((double)d * scale);
  return s < src - 1 ? s : src - 1;
}

MSS_CV_HD CvTap cv_linear(int d, double scale, int src) {
  const double prod = cv_pin(((double)d + 0.5) * scale);
  float f = (float)(prod - 0.5);
  int s = (int)floorf(f);
  f = f - (float)s;
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= src - 1) {
    s = src - 1;
    f = 0.f;
  }
  CvTap t;
  t.i0 = s;
  t.i1 = s + 1 < src ? s + 1 : src - 1;
  t.f = f;
  return t;
}
