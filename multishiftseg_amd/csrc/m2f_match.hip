// Hungarian matching of Mask2Former (lib/network/mask2former/modeling/matcher.py:70-179) for all S prediction steps x B images
// of a train step at once: two launches, no float atomics, no host round trip per image.
//
// A problem is one (step s, image b). Launch 1 (match_partial_kernel) cuts the P sampled points of every problem into NC chunks;
// a workgroup samples its chunk's mask logits x[q][p] and target masks t[m][p] bilinearly (F.grid_sample, align_corners=False,
// zero padding), evaluates softplus / sigmoid once per (q, p) and leaves in the float workspace
//     sum_p x t, sum_p sigmoid(x) t   [Q][T]      (neg - pos = x, so cost_mask = (sum_p neg - sum_p x t) / P)
//     sum_p neg, sum_p sigmoid(x)     [Q]         sum_p t   [T]
// Launch 2 (match_solve_kernel) adds the chunks in index order in float64, forms C = w_mask cost_mask + w_class cost_class +
// w_dice cost_dice, rounds it to fp32 once, and one wave solves the rectangular assignment on it by shortest augmenting paths in
// float64 (Crouse 2016, the algorithm of scipy.optimize.linear_sum_assignment, which the reference hands its fp32 C to).
// The contraction runs on the vector ALUs: DESIGN.md 3.12 holds the measurement behind that.
#include "mss_common.h"
#include "mss_point_sample.h"
#include "mss_m2f_maps.h"

namespace {

constexpr int MT_Q = 128;        // most queries (and targets) of a problem
constexpr int MT_PT = 32;        // points staged in LDS at a time
constexpr int MT_COLS = 16;      // target columns of a workgroup of launch 1: two halves of the workgroup x 8 accumulators
constexpr int MT_MAXCHUNKS = 16;

struct MatchPlan { int TP, NC, PC; long long stride; };

// TP: T padded to the column tile; NC chunks of PC points (a multiple of the staged tile; trailing chunks may be empty and then
// hold zeros); stride: floats of one (problem, chunk)
inline MatchPlan match_plan(int Q, int Tmax, int P) {
  MatchPlan p;
  p.TP = mss_cdiv(Tmax, MT_COLS) * MT_COLS;
  p.NC = mss_cdiv(P, 2 * MT_PT) < MT_MAXCHUNKS ? mss_cdiv(P, 2 * MT_PT) : MT_MAXCHUNKS;
  p.PC = mss_cdiv(mss_cdiv(P, p.NC), MT_PT) * MT_PT;
  p.stride = 2ll * Q * p.TP + 2ll * Q + p.TP;
  return p;
}

// Launch 1. grid (NC, S*B, TP / 16), 256 threads. Thread (q = tid & 127, half = tid >> 7): samples x[q][p] for the points p of its
// parity, then accumulates its 8 target columns over all 32 staged points.
__global__ __launch_bounds__(256) void match_partial_kernel(MssM2fMaps maps, MssM2fTargets tg, const float* __restrict__ points, int P, int Tmax,
                                                             int TP, int NC, int PC, long long stride, float* __restrict__ ws) {
  const long long bs = maps.img_stride, qs = maps.query_stride, ps = maps.pixel_stride;
  const int B = maps.B, Q = maps.Q, h = maps.h, w = maps.w, total_t = tg.total_t, H = tg.H, W = tg.W;
  __shared__ float xs[MT_PT][MT_Q];
  __shared__ float sg[MT_PT][MT_Q];
  __shared__ __attribute__((aligned(16))) float ts[MT_PT][MT_COLS];
  __shared__ PointTap mtap[MT_PT], ttap[MT_PT];
  __shared__ int valid[MT_PT];
  __shared__ float red[2][256];
  const int tid = threadIdx.x, c = blockIdx.x, prob = blockIdx.y, m0 = blockIdx.z * MT_COLS;
  const int s = prob / B, b = prob - s * B;
  const int t0 = tg.tstart[b], t1 = tg.tstart[b + 1], Tb = t1 - t0;
  if (t0 < 0 || Tb < 0 || t1 > total_t || Tb > Tmax || m0 >= Tb) return;      // a bad range is reported by launch 2 (status 1)
  const int q = tid & (MT_Q - 1), half = tid >> 7;
  const float* mq = maps.step[s] + (long long)b * bs + (long long)q * qs;
  const int pbeg = c * PC < P ? c * PC : P, pend = pbeg + PC < P ? pbeg + PC : P;
  float ax[8], ag[8], neg_acc = 0.f, sig_acc = 0.f, t_acc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) ax[k] = ag[k] = 0.f;

  for (int p0 = pbeg; p0 < pend; p0 += MT_PT) {
    if (tid < MT_PT) {
      const int p = p0 + tid;
      valid[tid] = p < pend;
      if (p < pend) {
        const float u = points[((long long)prob * P + p) * 2], v = points[((long long)prob * P + p) * 2 + 1];
        PointTap a, t;
        point_tap(u, w, a.x0, a.fx);
        point_tap(v, h, a.y0, a.fy);
        point_tap(u, W, t.x0, t.fx);
        point_tap(v, H, t.y0, t.fy);
        mtap[tid] = a;
        ttap[tid] = t;
      }
    }
    __syncthreads();
    for (int k = 0; k < MT_PT / 2; ++k) {
      const int p = half + 2 * k;
      float x = 0.f, g = 0.f;
      if (q < Q && valid[p]) {
        x = bilinear_zero(mq, ps, h, w, mtap[p]);
        const float e = expf(-fabsf(x)), l = log1pf(e), r = 1.f / (1.f + e);
        g = x >= 0.f ? r : e * r;
        neg_acc += fmaxf(x, 0.f) + l;              // neg = x + pos, pos = max(-x, 0) + log1p(exp(-|x|))
        sig_acc += g;
      }
      xs[p][q] = x;
      sg[p][q] = g;
    }
    for (int i = tid; i < MT_PT * MT_COLS; i += 256) {
      const int m = i & (MT_COLS - 1), p = i >> 4;
      float t = 0.f;
      if (m0 + m < Tb && valid[p]) t = bilinear_zero(tg.tmask + (long long)(t0 + m0 + m) * H * W, 1, H, W, ttap[p]);
      ts[p][m] = t;
    }
    __syncthreads();
#pragma unroll 4
    for (int p = 0; p < MT_PT; ++p) {
      const float x = xs[p][q], g = sg[p][q];
      const f32x4 ta = *(const f32x4*)&ts[p][half * 8], tb = *(const f32x4*)&ts[p][half * 8 + 4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ax[k] = __builtin_fmaf(x, ta[k], ax[k]);
        ag[k] = __builtin_fmaf(g, ta[k], ag[k]);
        ax[4 + k] = __builtin_fmaf(x, tb[k], ax[4 + k]);
        ag[4 + k] = __builtin_fmaf(g, tb[k], ag[4 + k]);
      }
    }
    if (tid < MT_COLS)
      for (int p = 0; p < MT_PT; ++p) t_acc += ts[p][tid];
    __syncthreads();
  }

  float* out = ws + ((long long)prob * NC + c) * stride;
  const long long QT = (long long)Q * TP;
  if (q < Q) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int m = m0 + half * 8 + k;                // < TP: TP is a multiple of the column tile
      out[(long long)q * TP + m] = ax[k];
      out[QT + (long long)q * TP + m] = ag[k];
    }
  }
  if (tid < MT_COLS) out[2 * QT + 2 * Q + m0 + tid] = t_acc;
  if (blockIdx.z == 0) {
    red[0][tid] = neg_acc;
    red[1][tid] = sig_acc;
    __syncthreads();
    if (tid < MT_Q && tid < Q) {
      out[2 * QT + tid] = red[0][tid] + red[0][tid + MT_Q];
      out[2 * QT + Q + tid] = red[1][tid] + red[1][tid + MT_Q];
    }
  }
}

__device__ __forceinline__ double bcast_d(double a0, double a1, int idx) { return __shfl(idx >> 6 ? a1 : a0, idx & 63); }
__device__ __forceinline__ int bcast_i(int a0, int a1, int idx) { return __shfl(idx >> 6 ? a1 : a0, idx & 63); }
// element idx of a two-per-lane register array, set by its owner lane (no dynamic register index)
#define MT_SET2(arr, idx, val)           \
  do {                                   \
    if (lane == ((idx) & 63)) {          \
      if ((idx) >> 6) arr[1] = (val);    \
      else arr[0] = (val);               \
    }                                    \
  } while (0)

// Launch 2: one workgroup per problem. MERGE: all 256 threads add the chunks and write C (global + LDS); else C is read.
// Then wave 0 solves T_b rows (targets) x Q columns (queries); lane l owns columns l, l + 64 and rows l, l + 64 in registers.
// Every loop is bounded by T_b or Q; a cost that is NaN or -inf, or a row without a finite column, ends the problem with status 1.
template <bool MERGE>
__global__ __launch_bounds__(256) void match_solve_kernel(const float* __restrict__ ws, MssM2fSteps cls, MssM2fTargets tg, const int* __restrict__ tcount,
                                                           int B, int Q, int C1, int P, int Tmax, int TP, int NC, long long stride, float w_class,
                                                           float w_mask, float w_dice, float* __restrict__ cost, int* __restrict__ match,
                                                           int* __restrict__ status) {
  __shared__ float cs[MT_Q * MT_Q];        // C transposed: [T_b][Q]
  const int tid = threadIdx.x, prob = blockIdx.x;
  const int s = prob / B, b = prob - s * B;
  int t0 = 0, Tb;
  bool bad;
  if (MERGE) {
    t0 = tg.tstart[b];
    const int t1 = tg.tstart[b + 1];
    Tb = t1 - t0;
    bad = t0 < 0 || Tb < 0 || t1 > tg.total_t;
  } else {
    Tb = tcount[b];
    bad = Tb < 0;
  }
  bad = bad || Tb > Tmax || Tb > Q;
  if (bad) Tb = 0;
  float* cp = cost + (long long)prob * Q * Tmax;
  if (MERGE) {
    const float* wp = ws + (long long)prob * NC * stride;
    const float* lg = cls.step[s] + (long long)b * Q * C1;
    const long long QT = (long long)Q * TP;
    for (int idx = tid; idx < Q * Tmax; idx += 256) {
      const int q = idx / Tmax, m = idx - q * Tmax;
      float o = 0.f;                                   // padding columns are written as 0
      if (m < Tb) {
        double xt = 0., st = 0., ng = 0., sm = 0., tm = 0.;
        for (int c = 0; c < NC; ++c) {
          const float* p = wp + c * stride;
          xt += (double)p[(long long)q * TP + m];
          st += (double)p[QT + (long long)q * TP + m];
          ng += (double)p[2 * QT + q];
          sm += (double)p[2 * QT + Q + q];
          tm += (double)p[2 * QT + 2 * Q + m];
        }
        const double cmask = (ng - xt) / (double)P;
        const double cdice = 1. - (2. * st + 1.) / (sm + tm + 1.);
        const int lab = tg.labels[t0 + m];
        double cclass = __builtin_nan("");             // a label outside the class range ends the problem with status 1
        if (lab >= 0 && lab < C1) {
          float mx = lg[q * C1];
          for (int k = 1; k < C1; ++k) mx = fmaxf(mx, lg[q * C1 + k]);
          double se = 0.;
          for (int k = 0; k < C1; ++k) se += exp((double)lg[q * C1 + k] - (double)mx);
          cclass = -exp((double)lg[q * C1 + lab] - (double)mx) / se;
        }
        o = (float)((double)w_mask * cmask + (double)w_class * cclass + (double)w_dice * cdice);
        cs[m * Q + q] = o;
      }
      cp[idx] = o;
    }
  } else {
    for (int idx = tid; idx < Q * Tmax; idx += 256) {
      const int q = idx / Tmax, m = idx - q * Tmax;
      if (m < Tb) cs[m * Q + q] = cp[idx];
    }
  }
  if (match == nullptr) return;
  __syncthreads();
  if (tid >= 64) return;

  const int lane = tid;
  const double INF = __builtin_huge_val();
  int fail = bad ? 1 : 0;
  {
    int nonfinite = 0;
    for (int i = lane; i < Tb * Q; i += 64) nonfinite |= !(cs[i] > -__builtin_huge_valf());      // NaN or -inf
    fail |= __any(nonfinite) ? 1 : 0;
  }
  double u[2] = {0., 0.}, v[2] = {0., 0.}, sp[2];
  int c4r[2] = {-1, -1}, r4c[2] = {-1, -1}, path[2] = {-1, -1};
  for (int cur = 0; cur < Tb && !fail; ++cur) {
    bool sr[2] = {false, false}, sc[2] = {false, false};
    sp[0] = sp[1] = INF;
    double minval = 0.;
    int i = cur, sink = -1;
    for (int it = 0; it < Q && sink < 0; ++it) {
      MT_SET2(sr, i, true);
      const double ui = bcast_d(u[0], u[1], i);
      const float* row = cs + i * Q;
      double best = INF;
      int bj = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        if (j < Q && !sc[k]) {
          const double r = minval + (double)row[j] - ui - v[k];
          if (r < sp[k]) {
            sp[k] = r;
            path[k] = i;
          }
          if (sp[k] < best) {                          // strict: the lower column wins a tie
            best = sp[k];
            bj = j;
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        if (ob < best || (ob == best && oj < bj)) {
          best = ob;
          bj = oj;
        }
      }
      if (!(best < INF)) {                             // no finite column left for this row: infeasible
        fail = 1;
        break;
      }
      minval = best;
      MT_SET2(sc, bj, true);
      const int r = bcast_i(r4c[0], r4c[1], bj);
      if (r < 0) sink = bj;
      else i = r;
    }
    if (sink < 0) fail = 1;
    if (fail) break;
#pragma unroll
    for (int k = 0; k < 2; ++k) {                      // duals of the rows and columns the search visited
      const int cj = c4r[k] < 0 ? 0 : c4r[k];
      const double s0 = __shfl(sp[0], cj & 63), s1 = __shfl(sp[1], cj & 63);
      if (lane + 64 * k == cur) u[k] += minval;
      else if (sr[k]) u[k] += minval - (cj >> 6 ? s1 : s0);
      if (sc[k]) v[k] -= minval - sp[k];
    }
    int j = sink;
    for (int step = 0; step <= Tb && j >= 0; ++step) { // augment along the path back to row cur
      const int pi = bcast_i(path[0], path[1], j);
      if (pi < 0 || pi >= Tb) {
        fail = 1;
        break;
      }
      MT_SET2(r4c, j, pi);
      const int old = bcast_i(c4r[0], c4r[1], pi);
      MT_SET2(c4r, pi, j);
      j = old;
      if (pi == cur) break;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int m = lane + 64 * k;
    if (m < Tmax) match[(long long)prob * Tmax + m] = (m < Tb && !fail) ? c4r[k] : -1;
  }
  if (lane == 0) status[prob] = fail;
}

bool match_shape_ok(int S, int B, int Q, int Tmax) { return m2f_steps_ok(S) && B >= 1 && Q >= 1 && Q <= MT_Q && Tmax >= 1 && Tmax <= MT_Q; }

}  // namespace

extern "C" long long mss_m2f_match_workspace_bytes(int S, int B, int Q, int Tmax, int P) {
  if (!match_shape_ok(S, B, Q, Tmax) || P < 1) return 0;
  const MatchPlan pl = match_plan(Q, Tmax, P);
  return 4ll * S * B * pl.NC * pl.stride;
}

extern "C" int mss_m2f_match_cost_f32(const MssM2fMaps* maps, const MssM2fSteps* cls, const MssM2fTargets* targets, const float* points, int C1,
                                      int P, int Tmax, float w_class, float w_mask, float w_dice, float* ws, float* cost, int* match, int* status,
                                      void* stream) {
  if (!maps || !cls || !targets || !targets->tstart || !points || !ws || !cost || (match == nullptr) != (status == nullptr)) return MSS_ERR_BAD_ARG;
  MssM2fMaps m = *maps;
  const MssM2fTargets tg = *targets;
  const int S = m.S, B = m.B, Q = m.Q;
  if (S < 1 || B < 1 || Q < 1 || Tmax < 1 || P < 1 || C1 < 1 || m.h < 1 || m.w < 1 || tg.H < 1 || tg.W < 1 || tg.total_t < 0) return MSS_ERR_BAD_ARG;
  if (m.img_stride < 0 || m.query_stride < 0 || m.pixel_stride < 0 || (tg.total_t > 0 && (!tg.tmask || !tg.labels))) return MSS_ERR_BAD_ARG;
  if (!match_shape_ok(S, B, Q, Tmax) || (long long)S * B > 65535) return MSS_ERR_UNSUPPORTED;
  MssM2fSteps cp;
  if (!m2f_fill(m.step, maps->step, S) || !m2f_fill(cp.step, cls->step, S)) return MSS_ERR_BAD_ARG;
  const MatchPlan pl = match_plan(Q, Tmax, P);
  hipStream_t st = (hipStream_t)stream;
  if (tg.total_t > 0)
    match_partial_kernel<<<dim3(pl.NC, S * B, pl.TP / MT_COLS), 256, 0, st>>>(m, tg, points, P, Tmax, pl.TP, pl.NC, pl.PC, pl.stride, ws);
  match_solve_kernel<true><<<S * B, 256, 0, st>>>(ws, cp, tg, nullptr, B, Q, C1, P, Tmax, pl.TP, pl.NC, pl.stride, w_class, w_mask, w_dice, cost, match,
                                                   status);
  return mss_launch_status();
}

extern "C" int mss_m2f_match_assign_f32(const float* cost, const int* tcount, int S, int B, int Q, int Tmax, int* match, int* status,
                                        void* stream) {
  if (!cost || !tcount || !match || !status || S < 1 || B < 1 || Q < 1 || Tmax < 1) return MSS_ERR_BAD_ARG;
  if (Q > MT_Q || Tmax > MT_Q) return MSS_ERR_UNSUPPORTED;
  match_solve_kernel<false><<<S * B, 256, 0, (hipStream_t)stream>>>(nullptr, MssM2fSteps{}, MssM2fTargets{}, tcount, B, Q, 1, 1, Tmax, 0, 0, 0, 0.f, 0.f, 0.f,
                                                                    const_cast<float*>(cost), match, status);
  return mss_launch_status();
}
