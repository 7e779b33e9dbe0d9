// SetCriterion of Mask2Former (lib/network/mask2former/modeling/criterion.py): loss_labels (:189-205), loss_masks (:312-363) and
// loss_masks_aug (:244-310) for all S prediction steps x B images x matched masks of a train step, forward and backward, in five
// launches that do not depend on S, B or T_b. No float atomics, no host round trip; every loop is bounded.
//
// A row is one matched (step s, target g): r = s * total_t + g. Its source map is the mask logits of query match[s,b,m] of image b
// (g = tstart[b] + m), its target map tmask[g]. One workgroup per row:
//   loss_select_kernel        the K candidates' keys go to a per-row workspace (L2-resident while its workgroup works on it), the
//                             exact k-th largest comes from 4 x 8-bit radix passes on the order-preserving bit pattern, ties are
//                             resolved by an in-order prefix count, the chosen points are written in ascending candidate index
//   loss_mask_forward_kernel  sum bce, sum sigmoid t, sum sigmoid, sum t over the row's P points in float64, one tree order
//   loss_finalize_kernel      one workgroup per step: target classes from the match table, the weighted cross entropy, and the
//                             row table folded in row order
//   loss_mask_backward_kernel the per-point gradient, scattered through the four bilinear taps into an int64 fixed-point window in
//                             LDS (integer addition is associative: any arrival order gives the same bits), converted once
//   loss_label_backward_kernel
// DESIGN.md 3.13 holds the reasoning.
#include "mss_common.h"
#include "mss_point_sample.h"
#include "mss_m2f_maps.h"

namespace {

constexpr int ML_T = 256;          // threads of every workgroup here
constexpr int ML_BAND = 7680;      // int64 cells of the backward's LDS window: 60 KiB

struct LossRow { int s, b, g, q; };      // q < 0: the row has no map (an unsolved problem)

// image of target g: the number of images that end at or before g (tstart is non-decreasing), clamped into the batch
__device__ __forceinline__ int image_of(const int* __restrict__ tstart, int B, int g) {
  int b = 0;
  for (int i = 1; i < B; ++i) b += tstart[i] <= g ? 1 : 0;
  return b;
}

__device__ __forceinline__ LossRow loss_row(long long r, int total_t, const int* __restrict__ tstart, const int* __restrict__ match, int B,
                                            int Q, int Tmax) {
  LossRow o;
  o.s = (int)(r / total_t);
  o.g = (int)(r - (long long)o.s * total_t);
  o.b = image_of(tstart, B, o.g);
  const int m = o.g - tstart[o.b];
  int q = -1;
  if (m >= 0 && m < Tmax && o.g < tstart[o.b + 1]) q = match[((long long)o.s * B + o.b) * Tmax + m];
  o.q = q >= 0 && q < Q ? q : -1;
  return o;
}

// order-preserving bit pattern of a key: larger float <=> larger unsigned. -0.0 counts as +0.0, a NaN ranks below every number.
__device__ __forceinline__ unsigned key_bits(float key) {
  if (key != key) return 0u;
  if (key == 0.f) key = 0.f;
  const unsigned u = __float_as_uint(key);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float bce_with_logits(float x, float t) { return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))); }

// grid R, 256 threads
__global__ __launch_bounds__(ML_T) void loss_select_kernel(MssM2fMaps maps, MssM2fTargets tg, const int* __restrict__ match,
                                                            const float* __restrict__ cand, const float* __restrict__ rnd, int Tmax, int K, int k,
                                                            int P, int Pr, int mode, int sel_start, unsigned* __restrict__ ws,
                                                            float* __restrict__ points) {
  const long long bs = maps.img_stride, qs = maps.query_stride, ps = maps.pixel_stride;
  const int B = maps.B, Q = maps.Q, h = maps.h, w = maps.w, total_t = tg.total_t, H = tg.H, W = tg.W;
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_need;
  __shared__ unsigned wcnt[ML_T / 64][2];
  const int tid = threadIdx.x;
  const long long r = blockIdx.x;
  const LossRow row = loss_row(r, total_t, tg.tstart, match, B, Q, Tmax);
  float* out = points + r * P * 2;
  if (row.q < 0) {
    for (int i = tid; i < 2 * P; i += ML_T) out[i] = 0.f;
    return;
  }
  const int ksel = row.g >= sel_start ? k : 0;
  const float* rr = rnd + r * Pr * 2;
  for (int i = tid; i < 2 * (P - ksel); i += ML_T) out[2 * ksel + i] = rr[i];
  if (ksel == 0) return;

  const float* cp = cand + ((long long)row.s * (total_t - sel_start) + (row.g - sel_start)) * K * 2;
  unsigned* keys = ws + r * K;
  const float* src = maps.step[row.s] + (long long)row.b * bs + (long long)row.q * qs;
  const uint8_t* tgt = tg.tmask + (long long)row.g * H * W;
  for (int i = tid; i < K; i += ML_T) {
    const float u = cp[2 * i], v = cp[2 * i + 1];
    PointTap a;
    point_tap(u, w, a.x0, a.fx);
    point_tap(v, h, a.y0, a.fy);
    const float x = bilinear_zero(src, ps, h, w, a);
    float key;
    if (mode == 2) {
      PointTap t;
      point_tap(u, W, t.x0, t.fx);
      point_tap(v, H, t.y0, t.fy);
      key = -bce_with_logits(x, bilinear_zero(tgt, 1, H, W, t));
    } else {
      key = -fabsf(x);
    }
    keys[i] = key_bits(key);
  }

  // the exact ksel-th largest key: after pass j, `prefix` holds its top 8 (j + 1) bits and `need` its rank among the keys that share them
  unsigned prefix = 0, need = (unsigned)ksel;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();                                  // also makes the keys visible to the whole workgroup
    for (int i = tid; i < K; i += ML_T) {
      const unsigned key = keys[i];
      if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned n = need;
      int bin = 255;
      for (; bin > 0; --bin) {
        const unsigned c = hist[bin];
        if (c >= n) break;
        n -= c;
      }
      sh_prefix = (prefix << 8) | (unsigned)bin;
      sh_need = n;
    }
    __syncthreads();
    prefix = sh_prefix;
    need = sh_need;
  }
  const unsigned tau = prefix;                        // every key > tau is taken, and the first `need` keys == tau in index order

  // in-order compaction: wave wv owns the candidates [beg, end); counts first, then positions from ballots
  const int lane = tid & 63, wv = tid >> 6;
  const int chunk = mss_cdiv(mss_cdiv(K, ML_T / 64), 64) * 64;
  const int beg = wv * chunk < K ? wv * chunk : K, end = beg + chunk < K ? beg + chunk : K;
  unsigned n_gt = 0, n_eq = 0;
  for (int base = beg; base < end; base += 64) {
    const int i = base + lane;
    const unsigned key = i < end ? keys[i] : 0u;
    n_gt += __popcll(__ballot(i < end && key > tau));
    n_eq += __popcll(__ballot(i < end && key == tau));
  }
  if (lane == 0) {
    wcnt[wv][0] = n_gt;
    wcnt[wv][1] = n_eq;
  }
  __syncthreads();
  unsigned run_eq = 0, gt_before = 0;
  for (int v = 0; v < wv; ++v) {
    gt_before += wcnt[v][0];
    run_eq += wcnt[v][1];
  }
  unsigned run_sel = gt_before + (run_eq < need ? run_eq : need);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = beg; base < end; base += 64) {
    const int i = base + lane;
    const unsigned key = i < end ? keys[i] : 0u;
    const bool gt = i < end && key > tau, eq = i < end && key == tau;
    const unsigned long long beq = __ballot(eq);
    const bool sel = gt || (eq && run_eq + (unsigned)__popcll(beq & below) < need);
    const unsigned long long bsel = __ballot(sel);
    const unsigned pos = run_sel + (unsigned)__popcll(bsel & below);
    if (sel && pos < (unsigned)ksel) {
      out[2 * pos] = cp[2 * i];
      out[2 * pos + 1] = cp[2 * i + 1];
    }
    run_eq += (unsigned)__popcll(beq);
    run_sel += (unsigned)__popcll(bsel);
  }
}

// sum of v over the workgroup in one fixed tree order; every thread gets it
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = ML_T / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

struct PointVal { double x, t, sg, bce; };

// the row's source and target samples at (u, v) and what both losses need of them, in float64 from the fp32 samples
__device__ __forceinline__ PointVal point_val(const float* src, long long ps, int h, int w, const uint8_t* tgt, int H, int W, float u,
                                              float v, PointTap& a) {
  PointTap t;
  point_tap(u, w, a.x0, a.fx);
  point_tap(v, h, a.y0, a.fy);
  point_tap(u, W, t.x0, t.fx);
  point_tap(v, H, t.y0, t.fy);
  PointVal o;
  o.x = (double)bilinear_zero(src, ps, h, w, a);
  o.t = (double)bilinear_zero(tgt, 1, H, W, t);
  const double e = exp(-fabs(o.x)), rcp = 1. / (1. + e);
  o.sg = o.x >= 0. ? rcp : e * rcp;
  o.bce = fmax(o.x, 0.) - o.x * o.t + log1p(e);
  return o;
}

// grid R, 256 threads
__global__ __launch_bounds__(ML_T) void loss_mask_forward_kernel(MssM2fMaps maps, MssM2fTargets tg, const int* __restrict__ match,
                                                                  const float* __restrict__ points, int Tmax, int P, double* __restrict__ rows) {
  const long long bs = maps.img_stride, qs = maps.query_stride, ps = maps.pixel_stride;
  const int B = maps.B, Q = maps.Q, h = maps.h, w = maps.w, total_t = tg.total_t, H = tg.H, W = tg.W;
  __shared__ double red[ML_T];
  const int tid = threadIdx.x;
  const long long r = blockIdx.x;
  const LossRow row = loss_row(r, total_t, tg.tstart, match, B, Q, Tmax);
  if (row.q < 0) {
    if (tid < 4) rows[r * 4 + tid] = __builtin_nan("");
    return;
  }
  const float* src = maps.step[row.s] + (long long)row.b * bs + (long long)row.q * qs;
  const uint8_t* tgt = tg.tmask + (long long)row.g * H * W;
  const float* pts = points + r * P * 2;
  double a_bce = 0., a_st = 0., a_sg = 0., a_t = 0.;
  for (int p = tid; p < P; p += ML_T) {
    PointTap a;
    const PointVal v = point_val(src, ps, h, w, tgt, H, W, pts[2 * p], pts[2 * p + 1], a);
    a_bce += v.bce;
    a_st += v.sg * v.t;
    a_sg += v.sg;
    a_t += v.t;
  }
  a_bce = block_sum(a_bce, red, tid);
  a_st = block_sum(a_st, red, tid);
  a_sg = block_sum(a_sg, red, tid);
  a_t = block_sum(a_t, red, tid);
  if (tid == 0) {
    rows[r * 4] = a_bce;
    rows[r * 4 + 1] = a_st;
    rows[r * 4 + 2] = a_sg;
    rows[r * 4 + 3] = a_t;
  }
}

// grid S, 256 threads
__global__ __launch_bounds__(ML_T) void loss_finalize_kernel(MssM2fSteps cls, MssM2fTargets tg, const int* __restrict__ match,
                                                              const float* __restrict__ weight, const double* __restrict__ rows, int B, int Q,
                                                              int C1, int Tmax, int P, int split, double scale0, double scale1, int ncols,
                                                              int* __restrict__ tclass, int* __restrict__ bad, double* __restrict__ wsum,
                                                              float* __restrict__ loss) {
  const int total_t = tg.total_t;
  __shared__ double red[ML_T];
  __shared__ int sbad;
  const int tid = threadIdx.x, s = blockIdx.x;
  int* tc = tclass + (long long)s * B * Q;
  if (tid == 0) sbad = 0;
  for (int i = tid; i < B * Q; i += ML_T) tc[i] = C1 - 1;
  __syncthreads();
  for (int g = tid; g < total_t; g += ML_T) {
    const LossRow row = loss_row((long long)s * total_t + g, total_t, tg.tstart, match, B, Q, Tmax);
    const int lab = tg.labels[g];
    if (row.q < 0 || lab < 0 || lab >= C1 - 1) atomicOr(&sbad, 1);
    else tc[row.b * Q + row.q] = lab;
  }
  __syncthreads();
  const float* lg = cls.step[s];
  double num = 0., den = 0.;
  for (int i = tid; i < B * Q; i += ML_T) {
    const float* x = lg + (long long)i * C1;
    float mx = x[0];
    for (int c = 1; c < C1; ++c) mx = fmaxf(mx, x[c]);
    double se = 0.;
    for (int c = 0; c < C1; ++c) se += exp((double)x[c] - (double)mx);
    const int c = tc[i];
    const double wc = (double)weight[c];
    num += wc * ((double)mx + log(se) - (double)x[c]);
    den += wc;
  }
  num = block_sum(num, red, tid);
  den = block_sum(den, red, tid);
  if (tid != 0) return;
  double acc[2][2] = {{0., 0.}, {0., 0.}};
  for (int g = 0; g < total_t; ++g) {                 // in row order
    const double* rw = rows + ((long long)s * total_t + g) * 4;
    const int G = g >= split ? 1 : 0;
    acc[G][0] += rw[0] / (double)P;
    acc[G][1] += 1. - (2. * rw[1] + 1.) / (rw[2] + rw[3] + 1.);
  }
  const float nanf_ = __builtin_nanf("");
  float* o = loss + (long long)s * ncols;
  o[0] = sbad ? nanf_ : (float)(num / den);
  for (int G = 0; 1 + 2 * G < ncols; ++G) {
    const double sc = G ? scale1 : scale0;
    o[1 + 2 * G] = sbad ? nanf_ : (float)(acc[G][0] * sc);
    o[2 + 2 * G] = sbad ? nanf_ : (float)(acc[G][1] * sc);
  }
  bad[s] = sbad;
  wsum[s] = den;
}

// grid R, 256 threads
__global__ __launch_bounds__(ML_T) void loss_mask_backward_kernel(MssM2fMaps maps, MssM2fTargets tg, const int* __restrict__ match,
                                                                   const int* __restrict__ bad, const float* __restrict__ points,
                                                                   const double* __restrict__ rows, const float* __restrict__ gloss, int Tmax,
                                                                   int P, int split, double scale0, double scale1, int ncols,
                                                                   float* __restrict__ ws, MssM2fGrads grads) {
  const long long bs = maps.img_stride, qs = maps.query_stride, ps = maps.pixel_stride;
  const int B = maps.B, Q = maps.Q, h = maps.h, w = maps.w, total_t = tg.total_t, H = tg.H, W = tg.W;
  __shared__ unsigned long long win[ML_BAND];
  const int tid = threadIdx.x;
  const long long r = blockIdx.x;
  const LossRow row = loss_row(r, total_t, tg.tstart, match, B, Q, Tmax);
  if (row.q < 0 || bad[row.s]) return;
  const long long map = (long long)row.b * bs + (long long)row.q * qs;
  const float* src = maps.step[row.s] + map;
  float* dst = grads.step[row.s] + map;
  const uint8_t* tgt = tg.tmask + (long long)row.g * H * W;
  const float* pts = points + r * P * 2;
  float* gc = ws + r * P;
  const int G = row.g >= split ? 1 : 0;
  const double sc = G ? scale1 : scale0;
  const double a = (double)gloss[(long long)row.s * ncols + 1 + 2 * G] * sc, d = (double)gloss[(long long)row.s * ncols + 2 + 2 * G] * sc;
  const double N = 2. * rows[r * 4 + 1] + 1., D = rows[r * 4 + 2] + rows[r * 4 + 3] + 1.;
  // |per-point gradient| <= |a| / P + |d| / 2 (|2 t D - N| <= 2 D, D >= 1, sigmoid' <= 1/4) and a tap's weights are <= 1, so every
  // cell's sum stays below P (|a| / P + 2 |d|) < 2^e: in units of 2^(e - 60) it fits an int64 with room for the roundings
  const double bound = fabs(a) + 2. * (double)P * fabs(d);
  const long long cells = (long long)h * w;
  if (!(bound > 0.) || !(bound < __builtin_huge_val())) {      // no gradient at all, or a non-finite one
    const float fill = bound == 0. ? 0.f : __builtin_nanf("");
    for (long long c = tid; c < cells; c += ML_T) dst[c * ps] = fill;
    return;
  }
  int e;
  frexp(bound, &e);
  const double to_fixed = ldexp(1., 60 - e), to_float = ldexp(1., e - 60);

  for (int p = tid; p < P; p += ML_T) {
    PointTap t;
    const PointVal v = point_val(src, ps, h, w, tgt, H, W, pts[2 * p], pts[2 * p + 1], t);
    gc[p] = (float)((v.sg - v.t) * (a / (double)P) - ((2. * v.t * D - N) / (D * D)) * v.sg * (1. - v.sg) * d);
  }
  const int band_rows = ML_BAND / w;                  // w <= ML_BAND is the launcher's condition
  for (int y_lo = 0; y_lo < h; y_lo += band_rows) {
    const int y_hi = y_lo + band_rows < h ? y_lo + band_rows : h;
    const int n = (y_hi - y_lo) * w;
    for (int c = tid; c < n; c += ML_T) win[c] = 0ull;
    __syncthreads();
    for (int p = tid; p < P; p += ML_T) {             // the same thread wrote gc[p]
      PointTap t;
      point_tap(pts[2 * p], w, t.x0, t.fx);
      point_tap(pts[2 * p + 1], h, t.y0, t.fy);
      const double g = (double)gc[p];
      const float gx = 1.f - t.fx, gy = 1.f - t.fy;
      const float wt[4] = {gx * gy, t.fx * gy, gx * t.fy, t.fx * t.fy};      // the forward's weights
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = t.x0 + (j & 1), y = t.y0 + (j >> 1);
        if (x >= 0 && x < w && y >= y_lo && y < y_hi)
          atomicAdd(&win[(y - y_lo) * w + x], (unsigned long long)__double2ll_rn(g * (double)wt[j] * to_fixed));
      }
    }
    __syncthreads();
    for (int c = tid; c < n; c += ML_T) dst[((long long)y_lo * w + c) * ps] = (float)((double)(long long)win[c] * to_float);
    __syncthreads();
  }
}

// grid (ceil(B Q / 256), S), 256 threads: one query per thread
__global__ __launch_bounds__(ML_T) void loss_label_backward_kernel(MssM2fSteps cls, const int* __restrict__ tclass, const int* __restrict__ bad,
                                                                    const float* __restrict__ weight, const double* __restrict__ wsum,
                                                                    const float* __restrict__ gloss, int B, int Q, int C1, int ncols,
                                                                    MssM2fGrads grads) {
  const int s = blockIdx.y;
  const long long i = (long long)blockIdx.x * ML_T + threadIdx.x;
  if (i >= (long long)B * Q) return;
  const float* x = cls.step[s] + i * C1;
  float* o = grads.step[s] + i * C1;
  if (bad[s]) {
    for (int c = 0; c < C1; ++c) o[c] = 0.f;
    return;
  }
  const int tc = tclass[(long long)s * B * Q + i];
  const double f = (double)weight[tc] / wsum[s] * (double)gloss[(long long)s * ncols];
  float mx = x[0];
  for (int c = 1; c < C1; ++c) mx = fmaxf(mx, x[c]);
  double se = 0.;
  for (int c = 0; c < C1; ++c) se += exp((double)x[c] - (double)mx);
  for (int c = 0; c < C1; ++c) o[c] = (float)(f * (exp((double)x[c] - (double)mx) / se - (c == tc ? 1. : 0.)));
}

bool loss_shape_ok(int S, int B, int Q, int Tmax, int total_t) {
  return m2f_steps_ok(S) && B >= 1 && Q >= 1 && Tmax >= 1 && total_t >= 0 && (long long)S * total_t <= 0x7fffffffll;
}

}  // namespace

extern "C" long long mss_m2f_loss_workspace_bytes(long long R, int K, int P) {
  if (R < 0 || K < 0 || P < 1) return 0;
  return 4ll * R * (K > P ? K : P);
}

extern "C" int mss_m2f_loss_select_f32(const MssM2fMaps* maps, const MssM2fTargets* targets, const int* match, const float* cand,
                                       const float* rnd, int Tmax, int K, int k, int P, int Pr, int mode, int sel_start, float* ws, float* points,
                                       void* stream) {
  if (!maps || !targets) return MSS_ERR_BAD_ARG;
  MssM2fMaps m = *maps;
  const MssM2fTargets tg = *targets;
  const int S = m.S, total_t = tg.total_t;
  if (!tg.tstart || !match || m.h < 1 || m.w < 1 || tg.H < 1 || tg.W < 1 || P < 1 || K < 0 || k < 0 || k > K || k > P || Pr < 0) return MSS_ERR_BAD_ARG;
  if (!loss_shape_ok(S, m.B, m.Q, Tmax, total_t)) return MSS_ERR_UNSUPPORTED;
  if (m.img_stride < 0 || m.query_stride < 0 || m.pixel_stride < 0 || sel_start < 0 || sel_start > total_t || (mode != 1 && mode != 2)) return MSS_ERR_BAD_ARG;
  if (total_t == 0) return MSS_OK;
  const bool selects = k > 0 && sel_start < total_t;
  if (!tg.tmask || !points || (selects && (!cand || !ws))) return MSS_ERR_BAD_ARG;
  const int most_random = (sel_start > 0 || k == 0) ? P : P - k;      // the most points a row takes from rnd
  if (Pr < most_random || (most_random > 0 && !rnd)) return MSS_ERR_BAD_ARG;
  if (!m2f_fill(m.step, maps->step, S)) return MSS_ERR_BAD_ARG;
  loss_select_kernel<<<S * total_t, ML_T, 0, (hipStream_t)stream>>>(m, tg, match, cand, rnd, Tmax, K, k, P, Pr, mode, sel_start, (unsigned*)ws, points);
  return mss_launch_status();
}

extern "C" int mss_m2f_loss_mask_forward_f32(const MssM2fMaps* maps, const MssM2fTargets* targets, const int* match, const float* points, int Tmax,
                                             int P, double* rows, void* stream) {
  if (!maps || !targets) return MSS_ERR_BAD_ARG;
  MssM2fMaps m = *maps;
  const MssM2fTargets tg = *targets;
  const int S = m.S, total_t = tg.total_t;
  if (!tg.tstart || !match || m.h < 1 || m.w < 1 || tg.H < 1 || tg.W < 1 || P < 1) return MSS_ERR_BAD_ARG;
  if (!loss_shape_ok(S, m.B, m.Q, Tmax, total_t)) return MSS_ERR_UNSUPPORTED;
  if (m.img_stride < 0 || m.query_stride < 0 || m.pixel_stride < 0) return MSS_ERR_BAD_ARG;
  if (total_t == 0) return MSS_OK;
  if (!tg.tmask || !points || !rows) return MSS_ERR_BAD_ARG;
  if (!m2f_fill(m.step, maps->step, S)) return MSS_ERR_BAD_ARG;
  loss_mask_forward_kernel<<<S * total_t, ML_T, 0, (hipStream_t)stream>>>(m, tg, match, points, Tmax, P, rows);
  return mss_launch_status();
}

extern "C" int mss_m2f_loss_finalize_f32(const MssM2fSteps* cls, const MssM2fTargets* targets, const int* match, const float* weight,
                                         const double* rows, int S, int B, int Q, int C1, int Tmax, int P, int split, double scale0, double scale1,
                                         int ncols, int* tclass, int* bad, double* wsum, float* loss, void* stream) {
  if (!targets) return MSS_ERR_BAD_ARG;
  const MssM2fTargets tg = *targets;
  const int total_t = tg.total_t;
  if (!tg.tstart || !match || !weight || !tclass || !bad || !wsum || !loss || C1 < 2 || P < 1 || (ncols != 3 && ncols != 5)) return MSS_ERR_BAD_ARG;
  if (!loss_shape_ok(S, B, Q, Tmax, total_t) || (long long)B * Q > 0x7fffffffll) return MSS_ERR_UNSUPPORTED;
  if (split < 0 || split > total_t || (ncols == 3 && split != total_t) || (total_t > 0 && (!tg.labels || !rows))) return MSS_ERR_BAD_ARG;
  MssM2fSteps cp;
  if (!cls || !m2f_fill(cp.step, cls->step, S)) return MSS_ERR_BAD_ARG;
  loss_finalize_kernel<<<S, ML_T, 0, (hipStream_t)stream>>>(cp, tg, match, weight, rows, B, Q, C1, Tmax, P, split, scale0, scale1, ncols, tclass, bad,
                                                            wsum, loss);
  return mss_launch_status();
}

extern "C" int mss_m2f_loss_mask_backward_f32(const MssM2fMaps* maps, const MssM2fTargets* targets, const int* match, const int* bad,
                                              const float* points, const double* rows, const float* gloss, int Tmax, int P, int split,
                                              double scale0, double scale1, int ncols, float* ws, const MssM2fGrads* grads, void* stream) {
  if (!maps || !targets) return MSS_ERR_BAD_ARG;
  MssM2fMaps m = *maps;
  const MssM2fTargets tg = *targets;
  const int S = m.S, total_t = tg.total_t;
  if (!tg.tstart || !match || !bad || !gloss || m.h < 1 || m.w < 1 || tg.H < 1 || tg.W < 1 || P < 1 || (ncols != 3 && ncols != 5)) return MSS_ERR_BAD_ARG;
  if (!loss_shape_ok(S, m.B, m.Q, Tmax, total_t) || m.w > ML_BAND) return MSS_ERR_UNSUPPORTED;
  if (m.img_stride < 0 || m.query_stride < 0 || m.pixel_stride < 0 || split < 0 || split > total_t || (ncols == 3 && split != total_t)) return MSS_ERR_BAD_ARG;
  if (total_t == 0) return MSS_OK;
  if (!tg.tmask || !points || !rows || !ws || !grads) return MSS_ERR_BAD_ARG;
  MssM2fGrads gp;
  if (!m2f_fill(m.step, maps->step, S) || !m2f_fill(gp.step, grads->step, S)) return MSS_ERR_BAD_ARG;
  loss_mask_backward_kernel<<<S * total_t, ML_T, 0, (hipStream_t)stream>>>(m, tg, match, bad, points, rows, gloss, Tmax, P, split, scale0, scale1, ncols,
                                                                           ws, gp);
  return mss_launch_status();
}

extern "C" int mss_m2f_loss_label_backward_f32(const MssM2fSteps* cls, const int* tclass, const int* bad, const float* weight, const double* wsum,
                                               const float* gloss, int S, int B, int Q, int C1, int ncols, const MssM2fGrads* grads, void* stream) {
  if (!tclass || !bad || !weight || !wsum || !gloss || !grads || C1 < 2 || (ncols != 3 && ncols != 5)) return MSS_ERR_BAD_ARG;
  if (!m2f_steps_ok(S) || B < 1 || Q < 1 || (long long)B * Q > 0x7fffffffll) return MSS_ERR_UNSUPPORTED;
  MssM2fSteps cp;
  MssM2fGrads gp;
  if (!cls || !m2f_fill(cp.step, cls->step, S) || !m2f_fill(gp.step, grads->step, S)) return MSS_ERR_BAD_ARG;
  loss_label_backward_kernel<<<dim3(mss_cdiv((long long)B * Q, ML_T), S), ML_T, 0, (hipStream_t)stream>>>(cp, tclass, bad, weight, wsum, gloss, B, Q, C1,
                                                                                                         ncols, gp);
  return mss_launch_status();
}
