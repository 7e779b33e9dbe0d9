// The class mix of SetCriterion.loss_ood, RCL branch (lib/network/mask2former/modeling/criterion.py:128-138, 162-187), forward and
// backward. Per prediction step the reference computes
//   P = softmax(pred_logits, -1)[..., :-1]                          :135 / :172
//   M = einsum("bqc,bqhw->bchw", P, sigmoid(pred_masks))            :136-138 / :173-175      at the LOW resolution h x w
//   L = interpolate(M[:, :19], size, bilinear)[:, :, :Ht, :Wt]      :166-168
//   s = -max_c interpolate(M', size, bilinear)[:, :, :Ht, :Wt]      :177-181
// and leaves the backward to autograd: an index_put with float atomics for the maximum, upsample_bilinear2d_backward with float
// atomics, two bmm and the sigmoid / softmax backward, each a pass over [B,Q,h,w] or [B,C,H,W]. Here:
//   mix_prob_kernel              P [B,Q,C]
//   mix_forward_kernel           M [B,C,h,w]: a thread owns a pixel, walks the Q queries in index order, P of the image in LDS
//   mix_upsample_kernel          L (the first min(C,19) channels, NCHW) or s = -max_c over all C channels, never the C full-size maps
//   mix_upsample_backward_kernel dM [B,C,h,w] in gather form: a thread owns a low-resolution pixel and walks, in one fixed order, the
//                                output pixels of the crop whose taps contain it; for ds it recomputes the C interpolated values of
//                                the output pixel and gives -ds to the largest (a tie: the lowest class index)
//   mix_backward_kernel          dx in the layout of x, and per-workgroup partial sums of dP[b,q,c] = sum_p dM[b,c,p] sigmoid(x[b,q,p]);
//                                without dx (dmasks == NULL: Mask2Former stage 1, frozen masks) the partial sums alone, same bits
//   mix_backward_fold_kernel     folds the partial sums in index order, one thread per (b, q, c)
//   mix_backward_cls_kernel      applies the softmax backward with the dropped column to the folded sums
// No float atomics, no memset, no integer buffer: two runs give the same bits. DESIGN.md 3.14 holds the reasoning.
#include "mss_common.h"
#include "mss_bilinear.h"
#include "../../include/mss_hip.h"

namespace {

constexpr int MX_T = 256;                      // threads of every workgroup here
constexpr int MX_MAXQ = 128, MX_MAXC = 32;     // most queries / classes
constexpr int MX_CL = 19;                      // channels of L (criterion.py:166)
constexpr int MX_TP = 64;                      // pixels of one tile of the mix backward: one per lane
constexpr int MX_TILES = 8;                    // tiles of one workgroup = pixels of one partial sum / MX_TP
constexpr int MX_LD = MX_TP + 1;               // LDS row stride of the tile tables: rows fall into different banks
constexpr int MX_PAIRS = MX_MAXQ * MX_MAXC / MX_T;      // (q, c) pairs of one thread in the partial sums

__device__ __forceinline__ float mix_sigmoid(float x) {
  const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
  return x >= 0.f ? r : e * r;
}

// grid ceil(B Q / 256)
__global__ __launch_bounds__(MX_T) void mix_prob_kernel(const float* __restrict__ cls, long long BQ, int C, float* __restrict__ prob) {
  const long long i = (long long)blockIdx.x * MX_T + threadIdx.x;
  if (i >= BQ) return;
  const float* row = cls + i * (C + 1);
  float m = row[0];
  for (int c = 1; c <= C; ++c) m = fmaxf(m, row[c]);
  float s = 0.f;
  for (int c = 0; c <= C; ++c) s += expf(row[c] - m);
  for (int c = 0; c < C; ++c) prob[i * C + c] = expf(row[c] - m) / s;
}

// the image's probability table into LDS as [Q][CP], the classes C..CP-1 zero
template <int CP>
__device__ __forceinline__ void mix_stage_prob(const float* __restrict__ prob, int b, int Q, int C, float* sp) {
  for (int i = threadIdx.x; i < Q * CP; i += MX_T) {
    const int q = i / CP, c = i - q * CP;
    sp[i] = c < C ? prob[((long long)b * Q + q) * C + c] : 0.f;
  }
}

// grid (ceil(hw / 256), B). PM: pixel-major logits [B,h,w,ldq] (qs == 1, ps == ldq, ldq % 4 == 0), else NCHW (ps == 1).
template <int CP, bool PM>
__global__ __launch_bounds__(MX_T) void mix_forward_kernel(const float* __restrict__ x, long long bs, long long qs, long long ps, int Q, int C,
                                                            long long hw, const float* __restrict__ prob, float* __restrict__ mix) {
  __shared__ __attribute__((aligned(16))) float sp[MX_MAXQ * CP];
  const int b = blockIdx.y;
  mix_stage_prob<CP>(prob, b, Q, C, sp);
  __syncthreads();
  const long long p = (long long)blockIdx.x * MX_T + threadIdx.x;
  if (p >= hw) return;
  const float* xp = x + (long long)b * bs + p * ps;
  float acc[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = 0.f;
  for (int q0 = 0; q0 < Q; q0 += 4) {
    float xv[4];
    if (PM) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xp + q0);       // the columns Q..ldq-1 may hold anything: never used below
      xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[j] = q0 + j < Q ? xp[(long long)(q0 + j) * qs] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (q0 + j >= Q) break;
      const float sg = mix_sigmoid(xv[j]);
      const float* pr = sp + (q0 + j) * CP;
#pragma unroll
      for (int c = 0; c < CP; ++c) acc[c] = __builtin_fmaf(sg, pr[c], acc[c]);      // in query order, in both layouts
    }
  }
  float* o = mix + (long long)b * C * hw + p;
#pragma unroll
  for (int c = 0; c < CP; ++c)
    if (c < C) o[(long long)c * hw] = acc[c];
}

// One interpolated value, in ATen's association h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) with the contraction fixed, so that the
// forward and the backward's recomputation give the same bits.
__device__ __forceinline__ float mix_interp(const float* __restrict__ m, int w, const SrcCoord& cy, const SrcCoord& cx) {
  const float w0 = 1.f - cx.l, w1 = cx.l, h0 = 1.f - cy.l, h1 = cy.l;
  const float* r0 = m + (long long)cy.i0 * w;
  const float* r1 = m + (long long)cy.i1 * w;
  const float top = __builtin_fmaf(w0, r0[cx.i0], w1 * r0[cx.i1]);
  const float bot = __builtin_fmaf(w0, r1[cx.i0], w1 * r1[cx.i1]);
  return __builtin_fmaf(h0, top, h1 * bot);
}

// grid (ceil(Wt / 64), ceil(Ht / 4), B): a thread owns one output pixel of the crop
template <bool NEGMAX>
__global__ __launch_bounds__(MX_T) void mix_upsample_kernel(const float* __restrict__ mix, int C, int Cl, int h, int w, int Ht, int Wt, float sy,
                                                             float sx, float* __restrict__ out) {
  const int b = blockIdx.z;
  const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (ox >= Wt || oy >= Ht) return;
  const SrcCoord cy = src_coord(oy, sy, h), cx = src_coord(ox, sx, w);
  const long long hw = (long long)h * w;
  const float* mb = mix + (long long)b * C * hw;
  if (NEGMAX) {
    float best = -__builtin_huge_valf();
    for (int c = 0; c < C; ++c) best = fmaxf(best, mix_interp(mb + c * hw, w, cy, cx));
    out[((long long)b * Ht + oy) * Wt + ox] = -best;
  } else {
    for (int c = 0; c < Cl; ++c) out[(((long long)b * Cl + c) * Ht + oy) * Wt + ox] = mix_interp(mb + c * hw, w, cy, cx);
  }
}

// the output rows (columns) that can have source pixel i among their taps: |src(o) - i| < 1, widened by one on either side; every
// candidate is checked against src_coord itself below, so the range only has to be a superset
__device__ __forceinline__ void mix_candidates(int i, float scale, int out_size, int& lo, int& hi) {
  const float a = floorf(((float)i - 0.5f) / scale - 0.5f) - 1.f, z = ceilf(((float)i + 1.5f) / scale - 0.5f) + 1.f;
  lo = a > 0.f ? (int)a : 0;
  hi = z < (float)(out_size - 1) ? (int)z : out_size - 1;
}

// the weight of source pixel i in an output pixel with coordinate c, and whether it is a tap at all
__device__ __forceinline__ bool mix_tap_weight(const SrcCoord& c, int i, float& wgt) {
  wgt = (c.i0 == i ? 1.f - c.l : 0.f) + (c.i1 == i ? c.l : 0.f);
  return c.i0 == i || c.i1 == i;
}

// grid (ceil(hw / 256), B): a thread owns one low-resolution pixel and all C channels of it
template <int CP>
__global__ __launch_bounds__(MX_T) void mix_upsample_backward_kernel(const float* __restrict__ dL, const float* __restrict__ ds,
                                                                      const float* __restrict__ mix, int C, int Cl, int h, int w, int Ht,
                                                                      int Wt, float sy, float sx, float* __restrict__ dmix) {
  const int b = blockIdx.y;
  const long long hw = (long long)h * w;
  const long long pix = (long long)blockIdx.x * MX_T + threadIdx.x;
  if (pix >= hw) return;
  const int iy = (int)(pix / w), ix = (int)(pix - (long long)iy * w);
  int oy_lo, oy_hi, ox_lo, ox_hi;
  mix_candidates(iy, sy, Ht, oy_lo, oy_hi);
  mix_candidates(ix, sx, Wt, ox_lo, ox_hi);
  const float* mb = mix + (long long)b * C * hw;
  float acc[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = 0.f;
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {                 // rows, then columns, ascending: one order
    const SrcCoord cy = src_coord(oy, sy, h);
    float wy;
    if (!mix_tap_weight(cy, iy, wy)) continue;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const SrcCoord cx = src_coord(ox, sx, w);
      float wx;
      if (!mix_tap_weight(cx, ix, wx)) continue;
      const float wgt = wy * wx;
      if (dL) {
        const float* g = dL + (((long long)b * Cl) * Ht + oy) * Wt + ox;
#pragma unroll
        for (int c = 0; c < CP; ++c)
          if (c < Cl) acc[c] = __builtin_fmaf(wgt, g[(long long)c * Ht * Wt], acc[c]);
      }
      if (ds) {
        float best = -__builtin_huge_valf();
        int arg = 0;
        for (int c = 0; c < C; ++c) {
          const float v = mix_interp(mb + c * hw, w, cy, cx);
          if (v > best) {                                   // strictly larger: a tie stays with the lowest class index
            best = v;
            arg = c;
          }
        }
        const float g = -ds[((long long)b * Ht + oy) * Wt + ox] * wgt;
#pragma unroll
        for (int c = 0; c < CP; ++c) acc[c] += c == arg ? g : 0.f;
      }
    }
  }
  float* o = dmix + (long long)b * C * hw + pix;
#pragma unroll
  for (int c = 0; c < CP; ++c)
    if (c < C) o[(long long)c * hw] = acc[c];
}

// grid (chunks, B), chunks = ceil(hw / (MX_TP MX_TILES)). Lane = pixel of the tile, wave = every fourth group of 4 queries.
// DX false (frozen masks, stage 1): no dx is formed or stored, so the probability table is not staged, only wave 0 reads dM and the
// pad columns of a pixel-major layout are not walked; sgs / sdm, the sums over them and their order are those of DX true.
template <int CP, bool PM, bool DX>
__global__ __launch_bounds__(MX_T) void mix_backward_kernel(const float* __restrict__ dmix, const float* __restrict__ prob,
                                                             const float* __restrict__ x, long long bs, long long qs, long long ps, int Q,
                                                             int C, long long hw, double* __restrict__ partial, float* __restrict__ dx) {
  __shared__ __attribute__((aligned(16))) float sp[MX_MAXQ * CP];
  __shared__ float sgs[MX_MAXQ * MX_LD];                    // sigmoid(x[q, p]) of the tile, 0 beyond the image
  __shared__ float sdm[CP * MX_LD];                         // dM[c, p] of the tile, 0 beyond the image
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (DX) mix_stage_prob<CP>(prob, b, Q, C, sp);
  double pacc[MX_PAIRS];
#pragma unroll
  for (int k = 0; k < MX_PAIRS; ++k) pacc[k] = 0.;
  const int nq4 = (PM && DX) ? (int)(ps >> 2) : (Q + 3) >> 2;       // pixel-major dx: every column up to ldq is written
  for (int t = 0; t < MX_TILES; ++t) {
    const long long p0 = ((long long)blockIdx.x * MX_TILES + t) * MX_TP;
    if (p0 >= hw) break;
    __syncthreads();                                        // sp is staged; the previous tile's sums are done with sgs / sdm
    const long long p = p0 + lane;
    const bool live = p < hw;
    float dm[CP];
    if (DX || wv == 0) {
#pragma unroll
      for (int c = 0; c < CP; ++c) dm[c] = (live && c < C) ? dmix[((long long)b * C + c) * hw + p] : 0.f;
    }
    if (wv == 0) {
#pragma unroll
      for (int c = 0; c < CP; ++c) sdm[c * MX_LD + lane] = dm[c];
    }
    const long long off = (long long)b * bs + p * ps;
    for (int q4 = wv; q4 < nq4; q4 += MX_T / 64) {
      float xv[4], o[4];
      if (PM) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (live) v = *reinterpret_cast<const f32x4*>(x + off + 4 * q4);
        xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = (live && 4 * q4 + j < Q) ? x[off + (long long)(4 * q4 + j) * qs] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = 4 * q4 + j;
        o[j] = 0.f;                                         // the pad columns Q..ldq-1 of a pixel-major gradient
        if (q >= Q) continue;
        const float sg = mix_sigmoid(xv[j]);
        if (DX) {
          const float* pr = sp + q * CP;
          float dot = 0.f;
#pragma unroll
          for (int c = 0; c < CP; ++c) dot = __builtin_fmaf(pr[c], dm[c], dot);
          o[j] = sg * (1.f - sg) * dot;
        }
        sgs[q * MX_LD + lane] = live ? sg : 0.f;
      }
      if (!DX || !live) continue;
      if (PM) {
        *reinterpret_cast<f32x4*>(dx + off + 4 * q4) = f32x4{o[0], o[1], o[2], o[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * q4 + j < Q) dx[off + (long long)(4 * q4 + j) * qs] = o[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MX_PAIRS; ++k) {
      const int pair = tid + k * MX_T;
      if (pair >= Q * C) break;
      const int q = pair / C, c = pair - q * C;
      float s = 0.f;
      for (int i = 0; i < MX_TP; ++i) s = __builtin_fmaf(sgs[q * MX_LD + i], sdm[c * MX_LD + i], s);     // pixels in index order
      pacc[k] += (double)s;                                 // tiles in index order
    }
  }
  double* o = partial + ((long long)b * gridDim.x + blockIdx.x) * Q * C;
#pragma unroll
  for (int k = 0; k < MX_PAIRS; ++k) {
    const int pair = tid + k * MX_T;
    if (pair < Q * C) o[pair] = pacc[k];
  }
}

// grid ceil(B Q C / 256): one (image, query, class) per thread, neighbouring threads on neighbouring doubles. Folds the image's
// partial sums in chunk order, 0 + p_0 + p_1 + ..., and leaves dP[b, q, c] in the slot of chunk 0. A launch of its own because
// mix_backward_cls_kernel has only one thread per query: folding there meant chunks x C loads, twice, one at a time (a mix at the
// image's resolution has 968 chunks at 704 x 704: 13 ms of latency for five such images).
__global__ __launch_bounds__(MX_T) void mix_backward_fold_kernel(double* __restrict__ partial, long long BQC, int QC, int chunks) {
  const long long i = (long long)blockIdx.x * MX_T + threadIdx.x;
  if (i >= BQC) return;
  const long long b = i / QC;
  double* p = partial + b * chunks * QC + (i - b * QC);
  double g = 0.;
#pragma unroll 8
  for (int k = 0; k < chunks; ++k) g += p[(long long)k * QC];
  p[0] = g;
}

// grid ceil(B Q / 256): one query per thread. dP[q, c] = what mix_backward_fold_kernel left in the slot of chunk 0; the softmax over
// C + 1 with the dropped column: dcls_j = p_j (g_j - sum_{c<C} p_c g_c), g_C = 0.
__global__ __launch_bounds__(MX_T) void mix_backward_cls_kernel(const float* __restrict__ cls, const double* __restrict__ partial, int B, int Q,
                                                                 int C, int chunks, float* __restrict__ dcls) {
  const long long i = (long long)blockIdx.x * MX_T + threadIdx.x;
  if (i >= (long long)B * Q) return;
  const int b = (int)(i / Q), q = (int)(i - (long long)b * Q);
  const float* row = cls + i * (C + 1);
  float m = row[0];
  for (int c = 1; c <= C; ++c) m = fmaxf(m, row[c]);
  double se = 0.;
  for (int c = 0; c <= C; ++c) se += exp((double)row[c] - (double)m);
  const double* pq = partial + (long long)b * chunks * Q * C + (long long)q * C;
  double dot = 0.;
  for (int c = 0; c < C; ++c) dot += exp((double)row[c] - (double)m) / se * pq[c];
  float* o = dcls + i * (C + 1);
  for (int c = 0; c < C; ++c) o[c] = (float)(exp((double)row[c] - (double)m) / se * (pq[c] - dot));
  o[C] = (float)(exp((double)row[C] - (double)m) / se * -dot);
}

// (image, query, pixel) strides of the mask logits -> 0 NCHW, 1 pixel-major, -1 neither
int mix_layout(long long bs, long long qs, long long ps, int Q, long long hw) {
  if (ps == 1 && qs >= hw && bs >= qs * Q) return 0;
  if (qs == 1 && ps >= Q && ps % 4 == 0 && bs >= ps * hw) return 1;
  return -1;
}

bool mix_shape_ok(int B, int Q, int C, int h, int w) {
  return B >= 1 && B <= 65535 && Q >= 1 && Q <= MX_MAXQ && C >= 1 && C <= MX_MAXC && h >= 1 && w >= 1 && (long long)h * w <= 0x3fffffffll;
}

bool mix_size_ok(int H, int W, int Ht, int Wt) { return H >= 1 && W >= 1 && Ht >= 1 && Wt >= 1 && Ht <= H && Wt <= W && Ht <= 4 * 65535; }

}  // namespace

#define MIX_BY_CP(C, CALL) \
  do {                      \
    if ((C) <= 8) {         \
      constexpr int CP = 8; \
      CALL;                 \
    } else if ((C) <= 20) { \
      constexpr int CP = 20; \
      CALL;                 \
    } else {                \
      constexpr int CP = 32; \
      CALL;                 \
    }                       \
  } while (0)

extern "C" int mss_m2f_mix_backward_chunks(long long hw) { return hw < 1 ? 0 : mss_cdiv(hw, (long long)MX_TP * MX_TILES); }

extern "C" int mss_m2f_mix_forward_f32(const float* cls, const float* masks, long long img_stride, long long query_stride, long long pixel_stride,
                                       int B, int Q, int C, int h, int w, float* prob, float* mix, void* stream) {
  if (!cls || !masks || !prob || !mix) return MSS_ERR_BAD_ARG;
  if (!mix_shape_ok(B, Q, C, h, w)) return MSS_ERR_UNSUPPORTED;
  const long long hw = (long long)h * w;
  const int layout = mix_layout(img_stride, query_stride, pixel_stride, Q, hw);
  if (layout < 0) return MSS_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  mix_prob_kernel<<<mss_cdiv((long long)B * Q, MX_T), MX_T, 0, st>>>(cls, (long long)B * Q, C, prob);
  const dim3 grid(mss_cdiv(hw, MX_T), B);
  if (layout)
    MIX_BY_CP(C, (mix_forward_kernel<CP, true><<<grid, MX_T, 0, st>>>(masks, img_stride, query_stride, pixel_stride, Q, C, hw, prob, mix)));
  else
    MIX_BY_CP(C, (mix_forward_kernel<CP, false><<<grid, MX_T, 0, st>>>(masks, img_stride, query_stride, pixel_stride, Q, C, hw, prob, mix)));
  return mss_launch_status();
}

extern "C" int mss_m2f_mix_upsample_f32(const float* mix, int B, int C, int h, int w, int H, int W, int Ht, int Wt, int neg_max, float* out,
                                        void* stream) {
  if (!mix || !out || !mix_size_ok(H, W, Ht, Wt)) return MSS_ERR_BAD_ARG;
  if (!mix_shape_ok(B, 1, C, h, w)) return MSS_ERR_UNSUPPORTED;
  const float sy = mss_bilinear_scale(h, H), sx = mss_bilinear_scale(w, W);      // the scale of the whole size, not of the crop
  const dim3 grid(mss_cdiv(Wt, 64), mss_cdiv(Ht, 4), B);
  const int Cl = C < MX_CL ? C : MX_CL;
  if (neg_max)
    mix_upsample_kernel<true><<<grid, MX_T, 0, (hipStream_t)stream>>>(mix, C, Cl, h, w, Ht, Wt, sy, sx, out);
  else
    mix_upsample_kernel<false><<<grid, MX_T, 0, (hipStream_t)stream>>>(mix, C, Cl, h, w, Ht, Wt, sy, sx, out);
  return mss_launch_status();
}

extern "C" int mss_m2f_mix_upsample_backward_f32(const float* dlogits, const float* dscore, const float* mix, int B, int C, int h, int w, int H,
                                                 int W, int Ht, int Wt, float* dmix, void* stream) {
  if ((!dlogits && !dscore) || (dscore && !mix) || !dmix || !mix_size_ok(H, W, Ht, Wt)) return MSS_ERR_BAD_ARG;
  if (!mix_shape_ok(B, 1, C, h, w)) return MSS_ERR_UNSUPPORTED;
  const float sy = mss_bilinear_scale(h, H), sx = mss_bilinear_scale(w, W);
  const dim3 grid(mss_cdiv((long long)h * w, MX_T), B);
  const int Cl = C < MX_CL ? C : MX_CL;
  MIX_BY_CP(C, (mix_upsample_backward_kernel<CP><<<grid, MX_T, 0, (hipStream_t)stream>>>(dlogits, dscore, mix, C, Cl, h, w, Ht, Wt, sy, sx, dmix)));
  return mss_launch_status();
}

extern "C" int mss_m2f_mix_backward_f32(const float* dmix, const float* prob, const float* cls, const float* masks, long long img_stride,
                                        long long query_stride, long long pixel_stride, int B, int Q, int C, int h, int w, double* partial,
                                        float* dmasks, float* dcls, void* stream) {
  if (!dmix || !prob || !cls || !masks || !partial || !dcls) return MSS_ERR_BAD_ARG;
  if (!mix_shape_ok(B, Q, C, h, w)) return MSS_ERR_UNSUPPORTED;
  const long long hw = (long long)h * w;
  const int layout = mix_layout(img_stride, query_stride, pixel_stride, Q, hw);
  if (layout < 0) return MSS_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = mss_m2f_mix_backward_chunks(hw);
  const dim3 grid(chunks, B);
#define MIX_BWD(PM, DX)                                                                                                                        \
  MIX_BY_CP(C, (mix_backward_kernel<CP, PM, DX><<<grid, MX_T, 0, st>>>(dmix, prob, masks, img_stride, query_stride, pixel_stride, Q, C, hw, \
                                                                       partial, dmasks)))
  if (layout && dmasks)
    MIX_BWD(true, true);
  else if (layout)
    MIX_BWD(true, false);               // dmasks == NULL: the masks are frozen, dcls alone
  else if (dmasks)
    MIX_BWD(false, true);
  else
    MIX_BWD(false, false);
#undef MIX_BWD
  const long long BQC = (long long)B * Q * C;
  mix_backward_fold_kernel<<<mss_cdiv(BQC, MX_T), MX_T, 0, st>>>(partial, BQC, Q * C, chunks);
  mix_backward_cls_kernel<<<mss_cdiv((long long)B * Q, MX_T), MX_T, 0, st>>>(cls, partial, B, Q, C, chunks, dcls);
  return mss_launch_status();
}
