// Per-sample channel compaction in front of a 1x1 product whose prologue is a Dropout2d-folded affine (deepv3.py:_dropout_affine):
// the dropped channels of sample n are exact zeros after the prologue, so the product only has to run over the K_n kept ones.
//
//   chan_compact_index_kernel   mask [N][C] -> idx [N][K_n] (ascending kept channels), count [N] = K_n, k_steps [N] = max(3, ceil(K_n/16)),
//                               place [N][C]: the channel that goes to column p of the compacted rows, or -1 (below);
//                               col [N][C] (optional): its inverse, the column channel c went to, or -1 for a dropped channel
//   chan_compact_rows_kernel    rows [img][r][0..C) -> rows [img][r][0..16 k_steps[img]): column p = act(row[place[img][p]]), 0 where place is -1;
//                               AFFINE: act = relu(v * sc + sh) (the expression of gemm.hip's finish_store), the activation side;
//                               !AFFINE: act = identity with ONE source image for all samples, the weight side (w [Kpad][C] -> [N][Kpad][C])
//
// Placement. v_mfma_f32_32x32x2_f32 adds its two products one after the other (lanes 0-31's k first), each with one fp32 rounding,
// and gemm_nt_kernel feeds the k of an 8-deep chunk in the order 0, 4, 1, 5, 2, 6, 3, 7: a dense product is ONE chain of fused
// multiply-adds per output element in that order, in which a dropped channel's term changes nothing (fma(0, w, acc) == acc). The
// compacted product is bit-identical to it when its chain visits the kept channels in the same order: the r-th kept channel of that
// order (key = 8 (c >> 3) + 2 (c & 3) + ((c >> 2) & 1)) goes to the column the kernel visits r-th, 8 (r >> 3) + ((r & 7) >> 1) + 4 (r & 1).
//
// A workgroup brings a few whole rows in with 16-byte loads, parks them (after the affine) in LDS, and every thread picks the four
// kept channels of each of its 16-byte output pieces from there -- the gather never leaves LDS. The thread's channel numbers and the
// affine of the columns it stages live in registers for all rows the workgroup walks (they all belong to one sample).
#include "mss_common.h"
#include "../../include/mss_hip.h"

namespace {

constexpr int CC_NT = 256;

__global__ __launch_bounds__(CC_NT) void chan_compact_index_kernel(const float* __restrict__ mask, int C, int* __restrict__ idx,
                                                                   int* __restrict__ place, int* __restrict__ count,
                                                                   int* __restrict__ k_steps, int* __restrict__ col) {
  __shared__ int part[CC_NT];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int per = (C + CC_NT - 1) / CC_NT;             // consecutive channels per thread: thread order == channel order
  const int c0 = tid * per, c1 = min(C, c0 + per);
  const float* m = mask + (size_t)n * C;
  int kept = 0;
  for (int c = c0; c < c1; ++c) kept += m[c] != 0.f;
  part[tid] = kept;
  __syncthreads();
  // inclusive scan over the 256 counts (Hillis-Steele; integer, so any order gives the same result)
  for (int o = 1; o < CC_NT; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int pos = part[tid] - kept;
  int* out = idx + (size_t)n * C;
  int* pl = place + (size_t)n * C;
  int* cl = col ? col + (size_t)n * C : nullptr;        // optional inverse of place: the column channel c went to, or -1
  for (int c = c0; c < c1; ++c) pl[c] = -1;
  if (cl)
    for (int c = c0; c < c1; ++c) cl[c] = -1;           // a thread writes col only at its own channels
  __syncthreads();                                      // ... before any thread places a channel into another thread's columns
  for (int c = c0; c < c1; ++c)
    if (m[c] != 0.f) {
      // rank of c in the product's visiting order: kept channels of earlier 8-blocks, then those of its own block with a smaller key
      const int b0 = c & ~7, key = 2 * (c & 3) + ((c >> 2) & 1);
      int r = pos;                                      // ascending rank of c
      for (int q = 0; q < 8; ++q) {
        const int cq = b0 + q;
        const bool k = m[cq] != 0.f;                    // C % 16 == 0: the block is inside the row
        if (k && cq < c) --r;
        if (k && 2 * (q & 3) + ((q >> 2) & 1) < key) ++r;
      }
      const int slot = 8 * (r >> 3) + ((r & 7) >> 1) + 4 * (r & 1);
      pl[slot] = c;
      if (cl) cl[c] = slot;
      out[pos++] = c;
    }
  if (tid == CC_NT - 1) {
    const int total = part[tid];
    count[n] = total;
    const int ks = (total + 15) / 16;
    k_steps[n] = ks < 3 ? 3 : ks;
  }
}

// NI: 16-byte pieces per thread and row (C <= NI * 1024); R: rows per round of the workgroup (R * C floats of LDS).
template <int NI, int R, bool AFFINE>
__global__ __launch_bounds__(CC_NT) void chan_compact_rows_kernel(const float* __restrict__ x, int ldx, long long x_img_rows,
                                                                  float* __restrict__ y, int ldy, int rows, int C,
                                                                  const int* __restrict__ place,
                                                                  const int* __restrict__ k_steps, const float* __restrict__ sc,
                                                                  const float* __restrict__ sh, int blocks_per_img) {
  extern __shared__ __attribute__((aligned(16))) float cc_smem[];      // [R][C]
  const int tid = threadIdx.x;
  const int img = blockIdx.x / blocks_per_img, blk = blockIdx.x - img * blocks_per_img;
  const int kfill = 16 * k_steps[img];
  int sel[NI][4];
  f32x4 s[NI], h[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = tid * 4 + i * 1024;
#pragma unroll
    for (int e = 0; e < 4; ++e) sel[i][e] = (c + e < kfill) ? place[(size_t)img * C + c + e] : -1;
    if (AFFINE) {
      s[i] = h[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < C) {
        s[i] = *reinterpret_cast<const f32x4*>(sc + (size_t)img * C + c);
        h[i] = *reinterpret_cast<const f32x4*>(sh + (size_t)img * C + c);
      }
    }
  }
  const float* xi = x + (size_t)img * x_img_rows * ldx;
  float* yi = y + (size_t)img * rows * ldy;
#pragma unroll 1
  for (int r0 = blk * R; r0 < rows; r0 += blocks_per_img * R) {
    f32x4 v[R][NI];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int r = r0 + q < rows ? r0 + q : rows - 1;      // rows past the end re-read the last row; never stored
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int c = tid * 4 + i * 1024;
        if (c < C) v[q][i] = *reinterpret_cast<const f32x4*>(xi + (size_t)r * ldx + c);
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int c = tid * 4 + i * 1024;
        if (c < C) {
          f32x4 val = v[q][i];
          if (AFFINE) {
            val = val * s[i] + h[i];
            val.x = fmaxf(val.x, 0.f); val.y = fmaxf(val.y, 0.f);
            val.z = fmaxf(val.z, 0.f); val.w = fmaxf(val.w, 0.f);
          }
          *reinterpret_cast<f32x4*>(cc_smem + q * C + c) = val;
        }
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; ++q) {
      if (r0 + q < rows) {
        float* yr = yi + (size_t)(r0 + q) * ldy;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int c = tid * 4 + i * 1024;
          if (c < kfill) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = sel[i][e] >= 0 ? cc_smem[q * C + sel[i][e]] : 0.f;
            *reinterpret_cast<f32x4*>(yr + c) = o;
          }
        }
      }
    }
    __syncthreads();
  }
}

template <bool AFFINE>
int launch_rows(const float* x, int ldx, long long x_img_rows, float* y, int ldy, int N, int rows, int C, const int* place,
                const int* k_steps, const float* sc, const float* sh, hipStream_t stream) {
  if (!x || !y || !place || !k_steps || (AFFINE && (!sc || !sh))) return MSS_ERR_BAD_ARG;
  if (N <= 0 || rows <= 0) return MSS_OK;
  if (C % 16 || C < 48 || C > 2048 || ldx % 4 || ldy % 4 || ldx < C || ldy < C) return MSS_ERR_UNSUPPORTED;
  uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y);
  if (AFFINE) al |= reinterpret_cast<uintptr_t>(sc) | reinterpret_cast<uintptr_t>(sh);
  if (al & 15) return MSS_ERR_BAD_ARG;
  // 32 KB of LDS per workgroup (4 rows of 2048 channels, 8 of <= 1024), about four workgroups per CU over the whole launch; a
  // workgroup walks rows of ONE sample
  const int R = C > 1024 ? 4 : 8;
  int per_img = 1024 / N;
  const int need = (rows + R - 1) / R;
  if (per_img > need) per_img = need;
  if (per_img < 1) per_img = 1;
  const dim3 grid((unsigned)(per_img * N)), block(CC_NT);
  const size_t smem = (size_t)R * C * sizeof(float);
  if (C > 1024)
    hipLaunchKernelGGL((chan_compact_rows_kernel<2, 4, AFFINE>), grid, block, smem, stream, x, ldx, x_img_rows, y, ldy, rows, C, place,
                       k_steps, sc, sh, per_img);
  else
    hipLaunchKernelGGL((chan_compact_rows_kernel<1, 8, AFFINE>), grid, block, smem, stream, x, ldx, x_img_rows, y, ldy, rows, C, place,
                       k_steps, sc, sh, per_img);
  return mss_launch_status();
}

}  // namespace

extern "C" {

int mss_chan_compact_wanted(const MssConvArgs* a) {
  if (!MSS_ENV_INT("MSS_DROPOUT_COMPACT", 1)) return 0;
  if (!a->in_scale || !a->in_shift || a->in_ss_stride != a->C || !a->in_relu || a->w_split || a->out_scale || a->batch > 1) return 0;
  if (a->R * a->S != 1 || a->stride != 1 || a->pad != 0 || a->H != a->OH || a->W != a->OW) return 0;
  if ((a->OH * a->OW) % 128 || a->K <= 64 || a->Kpad % 128 || a->C % 16 || a->C < 48 || a->C > 2048 || a->ldx != a->C) return 0;
  const unsigned long long rows = (unsigned long long)a->N * a->OH * a->OW;
  if (rows * a->ldx * 4ull >= 0xffffffffull || (unsigned long long)a->N * a->Kpad * a->C * 4ull >= 0xffffffffull) return 0;
  return 1;
}

int mss_chan_compact_index(const float* mask, int N, int C, int* idx, int* place, int* count, int* k_steps, int* col, void* stream) {
  if (!mask || !idx || !place || !count || !k_steps) return MSS_ERR_BAD_ARG;
  if (N <= 0) return MSS_OK;
  if (C % 16 || C < 48) return MSS_ERR_UNSUPPORTED;     // 16 * k_steps <= C must hold with k_steps >= 3
  hipLaunchKernelGGL(chan_compact_index_kernel, dim3(N), dim3(CC_NT), 0, static_cast<hipStream_t>(stream), mask, C, idx, place,
                     count, k_steps, col);
  return mss_launch_status();
}

int mss_chan_compact_act_f32(const float* x, int ldx, float* out, int ldout, int N, int rows_per_image, int C, const int* place,
                             const int* k_steps, const float* scale, const float* shift, void* stream) {
  return launch_rows<true>(x, ldx, rows_per_image, out, ldout, N, rows_per_image, C, place, k_steps, scale, shift,
                           static_cast<hipStream_t>(stream));
}

int mss_chan_compact_weights_f32(const float* w, float* out, int N, int Kpad, int C, const int* place, const int* k_steps,
                                 void* stream) {
  return launch_rows<false>(w, C, 0, out, C, N, Kpad, C, place, k_steps, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

}  // extern "C"
