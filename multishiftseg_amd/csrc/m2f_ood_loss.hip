// The pixel losses of SetCriterion.loss_ood, branches "margin" and "bce" (lib/network/mask2former/modeling/criterion.py:140-161),
// between the class mix M [B,C,h,w] (csrc/m2f_mix.hip) and its backward. The reference computes
//   t = -max_c M                                                  :141 / :152      at the LOW resolution
//   s = interpolate(t, (H, W), bilinear, align_corners=True)      :142 / :153      the padded size of ood_mask, no crop
//   loss = 0.5 (mean_{ood == 0} l_id(s) + [n_ood > 0] mean_{ood == 1} l_ood(s))    :144-149 / :155-161
// and leaves the backward to autograd: two boolean-index gathers that synchronise with the host, an index_put and an
// upsample_bilinear2d_backward with float atomics, several [B,H,W] passes. Here:
//   ood_negmax_kernel               t [B,h,w]
//   ood_pixel_loss_kernel           a thread owns output pixels of its workgroup's fixed range: four taps of t, one mask byte; the
//                                   workgroup leaves (S_id, S_ood, n_id, n_ood) as doubles, reduced in one fixed order
//   ood_pixel_loss_fold_kernel      adds the partial sums in index order -> stats [4] (double), loss (float)
//   ood_pixel_loss_backward_kernel  dM [B,C,h,w] whole, in gather form as mix_upsample_backward_kernel: a thread owns a low-resolution
//                                   pixel, walks the output pixels whose taps contain it (rows then columns ascending), recomputes s,
//                                   and gives -sum wy wx g to the arg-max channel of ITS pixel, recomputed from M (strict >: a tie
//                                   stays with the lowest class index), 0 to the others
// No float atomics, no memset, no integer buffer, no device-to-host copy: two runs give the same bits. DESIGN.md 3.32.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mss_bilinear_ac.h"
#include "../../include/mss_ood_hip.h"

namespace {

constexpr int OD_T = 256;                          // threads of every workgroup here
constexpr int OD_PX = 16;                          // output pixels of one thread in the forward
constexpr int OD_WG_PIXELS = OD_T * OD_PX;         // the fixed range of one workgroup = pixels of one partial sum

inline int od_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

inline int od_launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MSS_OK : (int)e;
}

__device__ __forceinline__ double od_wave_sum(double v) {          // a fixed tree: the same bits on every run
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float od_sigmoid(float x) {
  const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
  return x >= 0.f ? r : e * r;
}

// max(x, 0) + log1p(exp(-|x|))
__device__ __forceinline__ float od_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// The low-resolution arg-max: strictly larger wins, so a tie stays with the lowest class index. m points at channel 0 of the pixel.
__device__ __forceinline__ float od_first_max(const float* __restrict__ m, int C, size_t hw, int& arg) {
  float best = m[0];
  arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = m[(size_t)c * hw];
    if (v > best) {
      best = v;
      arg = c;
    }
  }
  return best;
}

// One interpolated value in ATen's association h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) with the contraction fixed (as mix_interp
// of m2f_mix.hip), so that the forward and the backward's recomputation give the same bits.
__device__ __forceinline__ float od_interp(const float* __restrict__ t, int w, const AcCoord& cy, const AcCoord& cx) {
  const float w0 = 1.f - cx.l, w1 = cx.l, h0 = 1.f - cy.l, h1 = cy.l;
  const float* r0 = t + (size_t)cy.i0 * w;
  const float* r1 = t + (size_t)cy.i1 * w;
  const float top = __builtin_fmaf(w0, r0[cx.i0], w1 * r0[cx.i1]);
  const float bot = __builtin_fmaf(w0, r1[cx.i0], w1 * r1[cx.i1]);
  return __builtin_fmaf(h0, top, h1 * bot);
}

// grid ceil(B h w / 256)
__global__ __launch_bounds__(OD_T) void ood_negmax_kernel(const float* __restrict__ mix, unsigned n_low, int C, unsigned hw, float* __restrict__ t) {
  const unsigned i = blockIdx.x * OD_T + threadIdx.x;
  if (i >= n_low) return;
  const unsigned b = i / hw, pix = i - b * hw;
  int arg;
  t[i] = -od_first_max(mix + (size_t)b * C * hw + pix, C, hw, arg);
}

// grid ceil(B H W / OD_WG_PIXELS): workgroup g owns the pixels [g OD_WG_PIXELS, (g + 1) OD_WG_PIXELS) of the flat [B,H,W] index; a
// thread walks its OD_PX pixels ascending (stride OD_T: neighbouring lanes on neighbouring bytes), then lanes, waves: one order.
template <int KIND, bool SCORE>
__global__ __launch_bounds__(OD_T) void ood_pixel_loss_kernel(const float* __restrict__ t, const uint8_t* __restrict__ ood, unsigned n_out, int h,
                                                               int w, int H, int W, float sy, float sx, float margin,
                                                               double* __restrict__ partial, float* __restrict__ score) {
  __shared__ double red[OD_T / 64][4];
  const unsigned HW = (unsigned)H * W, hw = (unsigned)h * w;
  const unsigned first = blockIdx.x * (unsigned)OD_WG_PIXELS + threadIdx.x;        // n_out < 2^31: first + k OD_T < 2^32
  double s_id = 0., s_ood = 0., n_id = 0., n_ood = 0.;
  for (int k = 0; k < OD_PX; ++k) {
    const unsigned i = first + k * OD_T;
    if (i >= n_out) break;
    const unsigned b = i / HW, r = i - b * HW;
    const int oy = (int)(r / W), ox = (int)(r - (unsigned)oy * W);
    const float s = od_interp(t + (size_t)b * hw, w, ac_coord(oy, sy, h), ac_coord(ox, sx, w));
    if (SCORE) score[i] = s;
    const int m = ood[i];
    if (m > 1) continue;                                  // neither set
    double term;
    if (KIND == MSS_OOD_MARGIN) {
      const double d = m ? fmax((double)margin - (double)s, 0.) : (double)s;
      term = d * d;
    } else {
      term = (double)od_softplus(m ? -s : s);
    }
    if (m) {
      s_ood += term;
      n_ood += 1.;
    } else {
      s_id += term;
      n_id += 1.;
    }
  }
  s_id = od_wave_sum(s_id);
  s_ood = od_wave_sum(s_ood);
  n_id = od_wave_sum(n_id);
  n_ood = od_wave_sum(n_ood);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[wv][0] = s_id;
    red[wv][1] = s_ood;
    red[wv][2] = n_id;
    red[wv][3] = n_ood;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double v = red[0][threadIdx.x];
    for (int j = 1; j < OD_T / 64; ++j) v += red[j][threadIdx.x];
    partial[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
  }
}

// one workgroup of 64: thread q < 4 adds quantity q of the partials in index order, 0 + p_0 + p_1 + ...
__global__ __launch_bounds__(64) void ood_pixel_loss_fold_kernel(const double* __restrict__ partial, int rows, double* __restrict__ stats,
                                                                  float* __restrict__ loss) {
  __shared__ double tot[4];
  if (threadIdx.x < 4) {
    double v = 0.;
#pragma unroll 16
    for (int k = 0; k < rows; ++k) v += partial[(size_t)k * 4 + threadIdx.x];
    tot[threadIdx.x] = v;
    stats[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double ood_term = tot[3] > 0. ? tot[1] / tot[3] : 0.;
    loss[0] = (float)(0.5 * (tot[0] / tot[2] + ood_term));          // n_id == 0: 0 / 0 = NaN, the mean of an empty tensor
  }
}

// grid ceil(B h w / 256): a thread owns one low-resolution pixel and all C channels of it
template <int KIND>
__global__ __launch_bounds__(OD_T) void ood_pixel_loss_backward_kernel(const float* __restrict__ mix, const float* __restrict__ t,
                                                                        const uint8_t* __restrict__ ood, const double* __restrict__ stats,
                                                                        const float* __restrict__ gloss, unsigned n_low, int C, int h, int w,
                                                                        int H, int W, float sy, float sx, float margin,
                                                                        float* __restrict__ dmix) {
  const unsigned i = blockIdx.x * OD_T + threadIdx.x;
  if (i >= n_low) return;
  const unsigned hw = (unsigned)h * w;
  const unsigned b = i / hw, pix = i - b * hw;
  const int iy = (int)(pix / w), ix = (int)(pix - (unsigned)iy * w);
  const double n_id = stats[2], n_ood = stats[3], half_g = 0.5 * (double)gloss[0];
  const float k_id = n_id > 0. ? (float)(half_g / n_id) : 0.f, k_ood = n_ood > 0. ? (float)(half_g / n_ood) : 0.f;
  int oy_lo, oy_hi, ox_lo, ox_hi;
  ac_candidates(iy, sy, H, &oy_lo, &oy_hi);
  ac_candidates(ix, sx, W, &ox_lo, &ox_hi);
  const float* tb = t + (size_t)b * hw;
  const uint8_t* ob = ood + (size_t)b * H * W;
  float acc = 0.f;
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {                 // rows, then columns, ascending: one order
    const AcCoord cy = ac_coord(oy, sy, h);
    float wy;
    if (!ac_tap_weight(cy, iy, &wy)) continue;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const AcCoord cx = ac_coord(ox, sx, w);
      float wx;
      if (!ac_tap_weight(cx, ix, &wx)) continue;
      const int m = ob[(size_t)oy * W + ox];
      if (m > 1) continue;
      const float s = od_interp(tb, w, cy, cx);
      float g;
      if (KIND == MSS_OOD_MARGIN)
        g = m ? k_ood * (-2.f * fmaxf(margin - s, 0.f)) : k_id * (2.f * s);
      else
        g = m ? k_ood * (od_sigmoid(s) - 1.f) : k_id * od_sigmoid(s);
      acc = __builtin_fmaf(wy * wx, g, acc);
    }
  }
  const float* mb = mix + (size_t)b * C * hw + pix;
  int arg;
  od_first_max(mb, C, hw, arg);
  float* o = dmix + (size_t)b * C * hw + pix;
  for (int c = 0; c < C; ++c) o[(size_t)c * hw] = c == arg ? 0.f - acc : 0.f;        // dt/dM = -1 in the arg-max channel
}

// the common checks 2-4 of include/mss_ood_hip.h, after the caller's NULL checks
int od_check(int B, int C, int h, int w, int H, int W, int kind, float margin) {
  if (B < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return MSS_ERR_BAD_ARG;
  if ((kind != MSS_OOD_MARGIN && kind != MSS_OOD_BCE) || !isfinite(margin)) return MSS_ERR_BAD_ARG;
  if (C > MSS_OOD_MAX_CLASSES) return MSS_ERR_UNSUPPORTED;
  if ((long long)B * h > MSS_OOD_MAX_PIXELS || (long long)B * h * w > MSS_OOD_MAX_PIXELS) return MSS_ERR_UNSUPPORTED;
  if ((long long)B * H > MSS_OOD_MAX_PIXELS || (long long)B * H * W > MSS_OOD_MAX_PIXELS) return MSS_ERR_UNSUPPORTED;
  return MSS_OK;
}

}  // namespace

extern "C" int mss_ood_abi_version(void) { return MSS_OOD_ABI_VERSION; }

extern "C" int mss_ood_loss_partials(long long pixels) {
  return pixels < 1 || pixels > MSS_OOD_MAX_PIXELS ? 0 : od_cdiv(pixels, OD_WG_PIXELS);
}

extern "C" int mss_ood_negmax_f32(const float* mix, int B, int C, int h, int w, float* t, void* stream) {
  if (!mix || !t) return MSS_ERR_BAD_ARG;
  const int rc = od_check(B, C, h, w, 1, 1, MSS_OOD_MARGIN, 0.f);
  if (rc != MSS_OK) return rc;
  const unsigned n_low = (unsigned)B * h * w;
  ood_negmax_kernel<<<od_cdiv(n_low, OD_T), OD_T, 0, (hipStream_t)stream>>>(mix, n_low, C, (unsigned)h * w, t);
  return od_launch_status();
}

extern "C" int mss_ood_pixel_loss_f32(const float* t, const uint8_t* ood, int B, int h, int w, int H, int W, int kind, float margin,
                                      double* partial, double* stats, float* loss, float* score, void* stream) {
  if (!t || !ood || !partial || !stats || !loss) return MSS_ERR_BAD_ARG;
  const int rc = od_check(B, 1, h, w, H, W, kind, margin);
  if (rc != MSS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned n_out = (unsigned)B * H * W;
  const int rows = mss_ood_loss_partials(n_out);
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
#define OD_FWD(KIND, SCORE) \
  ood_pixel_loss_kernel<KIND, SCORE><<<rows, OD_T, 0, st>>>(t, ood, n_out, h, w, H, W, sy, sx, margin, partial, score)
  if (kind == MSS_OOD_MARGIN) {
    if (score) OD_FWD(MSS_OOD_MARGIN, true);
    else OD_FWD(MSS_OOD_MARGIN, false);
  } else {
    if (score) OD_FWD(MSS_OOD_BCE, true);
    else OD_FWD(MSS_OOD_BCE, false);
  }
#undef OD_FWD
  ood_pixel_loss_fold_kernel<<<1, 64, 0, st>>>(partial, rows, stats, loss);
  return od_launch_status();
}

extern "C" int mss_ood_pixel_loss_backward_f32(const float* mix, const float* t, const uint8_t* ood, const double* stats, const float* gloss,
                                               int B, int C, int h, int w, int H, int W, int kind, float margin, float* dmix, void* stream) {
  if (!mix || !t || !ood || !stats || !gloss || !dmix) return MSS_ERR_BAD_ARG;
  const int rc = od_check(B, C, h, w, H, W, kind, margin);
  if (rc != MSS_OK) return rc;
  const unsigned n_low = (unsigned)B * h * w;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int grid = od_cdiv(n_low, OD_T);
  if (kind == MSS_OOD_MARGIN)
    ood_pixel_loss_backward_kernel<MSS_OOD_MARGIN><<<grid, OD_T, 0, (hipStream_t)stream>>>(mix, t, ood, stats, gloss, n_low, C, h, w, H, W, sy,
                                                                                           sx, margin, dmix);
  else
    ood_pixel_loss_backward_kernel<MSS_OOD_BCE><<<grid, OD_T, 0, (hipStream_t)stream>>>(mix, t, ood, stats, gloss, n_low, C, h, w, H, W, sy, sx,
                                                                                        margin, dmix);
  return od_launch_status();
}
