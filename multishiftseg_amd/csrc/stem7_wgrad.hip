// Weight gradient of the stem of the Mask2Former ResNet-50 backbone (conv 7x7, stride 2, padding 3, 3 -> 64; the forward is
// stem7.hip), with the backward of the max-pool behind it and of the ReLU in front of that fused into the loader of the dz operand.
// Reached through mss_conv2d_wgrad_f32 (conv_wgrad.hip), kernel MSS_WG_STEM7; which calls get here: wg_stem7_form / wg_stem7_check
// (wgrad_route.h), the plan: wg_plan_stem7.
//
//   dwp[tap][k][c] = sum over output pixels m of dz[m][k] * x[m @ tap][c]      (x: the image as NHWC with ONE ZERO pad channel)
//
// is a TN GEMM with the pixels as the reduction: 64 rows (k) x 49 * 4 = 196 columns (tap, c). One v_mfma_f32_16x16x4_f32 takes FOUR
// neighbouring output pixels of one row as its K = 4 step:
//  * operand A[i][kk] = dz[pixel kk][channel 16 v + i]: wave v of the four owns output channels 16 v .. 16 v + 15;
//  * operand B[kk][j] = x[pixel kk @ tap (r, 4 h + (j >> 2))][c = j & 3]: the 16 columns of one instruction are FOUR taps of one
//    filter row, so a filter row is two instructions (h = 0, 1) of which the last tap column (s = 7) does not exist -- 1/8 of the
//    multiplies are spent on it and its accumulator column is never stored. In the staged input patch ([row][column][4]) the lane's
//    address is base + 8 kk + j + an immediate: 40 consecutive floats, conflict-free.
//  * 7 x 2 accumulators of four registers hold the wave's 16 x 224 block of the result for the life of the workgroup: the whole
//    output lives in the accumulators of ONE workgroup and the work is split over pixel ranges only (wg_plan_stem7: a run of
//    4 x 16-pixel tiles per workgroup). The 14 instructions of a K step are independent, which covers the instruction's latency.
//  * Per tile the workgroup stages the input patch (13 x 38 pixels of 16 bytes, zero outside the image) and the dz tile
//    ([64 pixels][80]: the pitch puts the four pixels of a K step into four different groups of 16 banks) in LDS.
//
// Pool form (p.res = the stored stem output a0, after norm and ReLU; dy = the gradient at the POOLED map): dz is formed while the
// tile is staged. Pass 1 computes, for each of the 3 x 9 pool windows (3x3, stride 2, padding 1) that touch the tile and each
// channel, the arg-max among the window's in-image positions -- the FIRST maximum in row-major order, a NaN takes the window:
// F.max_pool2d's rule -- from a0 in global memory (each a0 value is read 2.25 times, from L2) and leaves [a0 at the arg-max > 0] * dy
// and the arg-max's place in the window (0 .. 8) in LDS. Pass 2 forms dz[oy][ox][k] as the sum, in ascending (py, px) order, over
// the up to four windows that contain (oy, ox) of the values whose arg-max is (oy, ox). No index tensor exists, nothing is scattered,
// no atomics: the sum is the same bits every run. (An a0 tile with its halo in LDS instead would take 6 x 18 x 256 B = 27 KB and save
// nothing: the window table is a quarter of that, and pass 2 reads only it.)
//
// Every split writes its whole [49][64][4] slab (into dwp itself where there is one split); wgrad_reduce_kernel /
// wgrad_reduce_par_kernel (conv_wgrad.hip) add the slabs in ascending split order.
#include "mss_common.h"
#include "../../include/mss_hip.h"
#include "wgrad_route.h"

void mss_wgrad_reduce_launch(const float* ws, float* dwp, long long slab4, int splits, hipStream_t stream);   // conv_wgrad.hip
int mss_stem7_wgrad_launch(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, float* ws, hipStream_t stream);

namespace {

constexpr int SW_TH = WG_STEM7_TH, SW_TW = WG_STEM7_TW;       // output pixels per tile: 4 x 16
constexpr int SW_PH = 2 * SW_TH + 5, SW_PW = 2 * SW_TW + 6;   // input patch: 13 x 38 pixels (one column more than the taps reach: s = 7)
constexpr int SW_ZP = 80;                                     // floats between two pixels of the dz tile
constexpr int SW_WR = SW_TH / 2 + 1, SW_WC = SW_TW / 2 + 1;   // pool windows that touch a tile: 3 x 9
constexpr int SW_SLAB = 49 * MSS_STEM7_K * 4;
static_assert(MSS_STEM7_K == 4 * 16 && SW_TH % 2 == 0 && SW_TW % 4 == 0, "four waves of 16 output channels; tiles start on even rows and columns");

struct Stem7WgradArgs {
  const float* x;      // [N][H][W][4]
  const float* dy;     // plain form: dz [N][OH][OW][lddy]; pool form: [N][PH][PW][lddy]
  const float* a0;     // pool form: [N][OH][OW][ldres]
  float* out;          // [splits][49][64][4]
  int N, H, W, OH, OW, PH, PW, lddy, ldres;
  int tiles_x, tiles_y, tiles_per_split;
  long long tiles;
};

template <bool POOL>
__global__ __launch_bounds__(256, 4) void stem7_wgrad_kernel(Stem7WgradArgs p) {
  __shared__ __attribute__((aligned(16))) float patch[SW_PH * SW_PW * 4];          // [row][column][4 channels]
  __shared__ __attribute__((aligned(16))) float dzt[SW_TH * SW_TW * SW_ZP];        // [pixel][channel], pitch SW_ZP
  __shared__ __attribute__((aligned(16))) float win_g[POOL ? SW_WR * SW_WC * 64 : 4];          // [window][channel]: gated dy
  __shared__ __attribute__((aligned(16))) unsigned char win_i[POOL ? SW_WR * SW_WC * 64 : 4];  // [window][channel]: arg-max place 0 .. 8

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int cb = __builtin_amdgcn_readfirstlane(tid >> 6);   // this wave's block of 16 output channels
  const int j = lane & 15, q = lane >> 4;                    // operand row / column, pixel of the K step; accumulator: column j, rows 4 q ..

  const int sp = mss_xcd_remap(blockIdx.x, gridDim.x);
  const long long t_begin = (long long)sp * p.tiles_per_split;
  const long long t_end = t_begin + p.tiles_per_split < p.tiles ? t_begin + p.tiles_per_split : p.tiles;

  f32x4 acc[7][2];
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int h = 0; h < 2; ++h) acc[r][h] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* abase = &dzt[q * SW_ZP + cb * 16 + j];
  const float* bbase = &patch[8 * q + j];

  for (long long t = t_begin; t < t_end; ++t) {
    const int tx = (int)(t % p.tiles_x), ty = (int)((t / p.tiles_x) % p.tiles_y), n = (int)(t / ((long long)p.tiles_x * p.tiles_y));
    const int oy0 = ty * SW_TH, ox0 = tx * SW_TW;
    __syncthreads();                                         // the previous tile's operands have been read

    // ---- the input patch -> LDS, zero outside the image
    {
      const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
      const float* img = p.x + (size_t)n * p.H * p.W * 4;
      for (int i = tid; i < SW_PH * SW_PW; i += 256) {
        const int py = i / SW_PW, px = i - py * SW_PW;
        const int iy = iy0 + py, ix = ix0 + px;
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
          val = *reinterpret_cast<const f32x4*>(img + ((size_t)iy * p.W + ix) * 4);
        *reinterpret_cast<f32x4*>(&patch[i * 4]) = val;
      }
    }

    const int wy0 = oy0 >> 1, wx0 = ox0 >> 1;                 // first pool window of the tile's table
    if (POOL) {
      // ---- pass 1: per (window, four channels) the arg-max place and the gated gradient
      const float* amap = p.a0 + (size_t)n * p.OH * p.OW * p.ldres;
      for (int i = tid; i < SW_WR * SW_WC * 16; i += 256) {
        const int cq = i & 15, wi = i >> 4;
        const int wr = wi / SW_WC, wc = wi - wr * SW_WC;
        const int py = wy0 + wr, px = wx0 + wc;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        unsigned places = 0;
        if (py < p.PH && px < p.PW) {
          const int first = (py == 0 ? 3 : 0) + (px == 0 ? 1 : 0);      // the first in-image position: where max_pool2d's index starts
          int at[4] = {first, first, first, first};
          f32x4 mx = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            const int oy = 2 * py - 1 + u;
            if ((unsigned)oy >= (unsigned)p.OH) continue;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
              const int ox = 2 * px - 1 + v;
              if ((unsigned)ox >= (unsigned)p.OW) continue;
              const f32x4 val = *reinterpret_cast<const f32x4*>(amap + ((size_t)oy * p.OW + ox) * p.ldres + cq * 4);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (val[e] > mx[e] || val[e] != val[e]) { mx[e] = val[e]; at[e] = u * 3 + v; }
            }
          }
          const f32x4 d = *reinterpret_cast<const f32x4*>(p.dy + (((size_t)n * p.PH + py) * p.PW + px) * p.lddy + cq * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            g[e] = mx[e] > 0.f ? d[e] : 0.f;                  // the ReLU gate at the arg-max (false for a NaN, as autograd's)
            places |= (unsigned)at[e] << (8 * e);
          }
        }
        *reinterpret_cast<f32x4*>(&win_g[wi * 64 + cq * 4]) = g;
        *reinterpret_cast<unsigned*>(&win_i[wi * 64 + cq * 4]) = places;
      }
      __syncthreads();
    }

    // ---- the dz tile -> LDS, zero outside the map
    for (int i = tid; i < SW_TH * SW_TW * 16; i += 256) {
      const int cq = i & 15, pix = i >> 4;
      const int a = pix / SW_TW, b = pix - a * SW_TW;
      const int oy = oy0 + a, ox = ox0 + b;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (oy < p.OH && ox < p.OW) {
        if (!POOL) {
          val = *reinterpret_cast<const f32x4*>(p.dy + (((size_t)n * p.OH + oy) * p.OW + ox) * p.lddy + cq * 4);
        } else {
          // the windows that contain (oy, ox): one along an even coordinate (place 1), two along an odd one (places 2, then 0)
          const int ny = 1 + (oy & 1), nx = 1 + (ox & 1);
          for (int u = 0; u < ny; ++u) {
            const int wr = (oy >> 1) + u - wy0, place_y = (oy & 1) ? 2 - 2 * u : 1;
            for (int v = 0; v < nx; ++v) {
              const int wc = (ox >> 1) + v - wx0, place_x = (ox & 1) ? 2 - 2 * v : 1;
              const unsigned place = (unsigned)(place_y * 3 + place_x);
              const int wi = wr * SW_WC + wc;
              const f32x4 g = *reinterpret_cast<const f32x4*>(&win_g[wi * 64 + cq * 4]);
              const unsigned places = *reinterpret_cast<const unsigned*>(&win_i[wi * 64 + cq * 4]);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (((places >> (8 * e)) & 255u) == place) val[e] += g[e];
            }
          }
        }
      }
      *reinterpret_cast<f32x4*>(&dzt[pix * SW_ZP + cq * 4]) = val;
    }
    __syncthreads();

    // ---- 16 K steps of four pixels x 14 instructions
#pragma unroll
    for (int a = 0; a < SW_TH; ++a) {
      if (oy0 + a >= p.OH) break;                            // workgroup-uniform: rows below the map hold zeros
#pragma unroll
      for (int g = 0; g < SW_TW / 4; ++g) {
        const float av = abase[(a * SW_TW + 4 * g) * SW_ZP];
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float bv = bbase[(2 * a + r) * SW_PW * 4 + 32 * g + 16 * h];
            acc[r][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[r][h], 0, 0, 0);
          }
      }
    }
  }

  // ---- the slab: accumulator row 4 q + e is channel 16 cb + 4 q + e, column j is (tap 4 h + (j >> 2), input channel j & 3)
  float* o = p.out + (size_t)sp * SW_SLAB + (size_t)(cb * 16 + 4 * q) * 4 + (j & 3);
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int s = 4 * h + (j >> 2);
      if (s < 7) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[((size_t)(r * 7 + s) * MSS_STEM7_K + e) * 4] = acc[r][h][e];
      }
    }
}

}  // namespace

// r: wg_plan_stem7(p); the arguments passed wg_stem7_check and ws holds r.ws_bytes (launch_route, conv_wgrad.hip).
int mss_stem7_wgrad_launch(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, float* ws, hipStream_t stream) {
  Stem7WgradArgs a;
  a.x = p.x; a.dy = dy; a.a0 = p.res;
  a.out = r.splits > 1 ? ws : dwp;
  a.N = p.N; a.H = p.H; a.W = p.W; a.OH = p.OH; a.OW = p.OW;
  a.PH = (p.OH - 1) / 2 + 1; a.PW = (p.OW - 1) / 2 + 1;
  a.lddy = lddy; a.ldres = p.ldres;
  a.tiles_x = mss_cdiv(p.OW, SW_TW); a.tiles_y = mss_cdiv(p.OH, SW_TH);
  a.tiles = wg_stem7_tiles(p);
  a.tiles_per_split = r.rows_per_split / (SW_TH * SW_TW);
  if (p.res) hipLaunchKernelGGL(stem7_wgrad_kernel<true>, dim3((unsigned)r.splits), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(stem7_wgrad_kernel<false>, dim3((unsigned)r.splits), dim3(256), 0, stream, a);
  if (const int rc = mss_launch_status()) return rc;
  if (r.splits > 1) {
    mss_wgrad_reduce_launch(ws, dwp, SW_SLAB / 4, r.splits, stream);
    return mss_launch_status();
  }
  return MSS_OK;
}
