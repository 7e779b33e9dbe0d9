// Weight gradient of the convolutions and Linears on the fp32 matrix cores of MI355X: the kernels, one launcher per kernel and the
// four C entry points. Which kernel a product gets, its grid, splits and scratch are decided in wgrad_route.h (plain host C++,
// checked alone by tests/wgrad_route_check.cpp); nothing here recomputes a plan.
#include "mss_epilogue.h"
#include "wgrad_route.h"
static_assert(MSS_WGRAD_PERIMG_TAIL_BYTES == (long long)TN_PERIMG_MAX_SLOTS * 128 * 128 * 4, "include/mss_hip.h and tn_perimg_plan.h disagree");
#include <stdlib.h>

bool mss_wgrad_tn_bf16x3_eligible(const MssConvArgs& p, int lddy);   // gemm_bf16x3.hip
long long mss_wgrad_tn_bf16x3_ws_bytes(const MssConvArgs& p, int Cp);
void mss_wgrad_tn_bf16x3_plan(const MssConvArgs& p, WgradRoute& r);
int mss_wgrad_tn_bf16x3_launch(const MssConvArgs& p, const float* dy, int lddy, float* dwp, int Cp, float* ws, long long ws_bytes, void* stream);
int mss_stem7_wgrad_launch(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, float* ws, hipStream_t stream);   // stem7_wgrad.hip

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------------------------------
// wgrad: dWp[tap][k][c] = sum_m dy[m][k] * act(x[m_tap][c])   (reduction over output pixels)
// MFMA rows = k (output channels), columns = c (input channels), contraction = pixels.
// Both operands sit in LDS as [pixel][channel] (their natural NHWC order) and are read with
// ds_read_b32: lane (i = l&31, kk = l>>5) reads row kk, column i -> 32 consecutive floats, so any
// row stride is conflict-free; the stride is a multiple of 4 floats so staging uses ds_write_b128.
// Same in-wave pipeline as the forward kernel: loads for pixel block t+1 issued first, written to
// LDS before the second-to-last chunk, one barrier before the last chunk.
// Grid: (ktiles*ctiles, taps, splits); the pixel range is split across blockIdx.z. No atomics: with one split the
// tile is stored straight into dWp; with several, split z stores its partial tile into slab z of a workspace
// ([splits][taps][Kpad][Cp], every element written by exactly one workgroup) and wgrad_reduce_kernel adds the slabs
// in split order -- the weight gradient is bit-reproducible run to run (the reference pins cudnn.deterministic,
// lib/utils/utils.py:10-13).
template <int BKO, int BCI, int BP, int WK>
__global__ __launch_bounds__(NT) void conv_wgrad_kernel(MssConvArgs p, const float* __restrict__ dy, int lddy,
                                                        float* __restrict__ dwp, int Cp, int pix_per_split) {
  constexpr int LDA = BKO + 4;  // dy tile  [BP][BKO]
  constexpr int LDB = BCI + 4;  // x  tile  [BP][BCI]
  constexpr int WC = 4 / WK;    // waves along K x waves along C (2x2; 1x4 for the 32-row tile of the 19-channel heads)
  constexpr int WTK = BKO / WK, WTC = BCI / WC;
  constexpr int TM = WTK / 32, TN = WTC / 32;
  constexpr int A_CPR = BKO / 4, B_CPR = BCI / 4;
  constexpr bool A_PART = BP * A_CPR < NT;                // dy tile smaller than one float4 per thread: upper threads idle
  constexpr int A_LD = A_PART ? 1 : BP * A_CPR / NT, B_LD = BP * B_CPR / NT;
  constexpr int A_RPP = NT / A_CPR, B_RPP = NT / B_CPR;   // pixel rows covered per staging pass
  constexpr int NKC = BP / 8;                             // chunks of 8 pixels = 4 MFMA k-steps
  static_assert(TM >= 1 && TN >= 1 && B_LD >= 1 && NKC >= 2, "");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                    // [2][BP][LDA]
  float* Bs = smem + 2 * BP * LDA;     // [2][BP][LDB]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WC, wn = wave % WC;
  const int ctiles = mss_cdiv(p.C, BCI);
  const int kt = blockIdx.x / ctiles, ct = blockIdx.x % ctiles;
  const int k0 = kt * BKO, c0 = ct * BCI;
  const int tap = blockIdx.y;           // output slab index: a filter tap, or (batched mode) a Winograd position
  int geo_tap = tap;
  if (p.batch > 1) {                    // 16 independent [K x T] x [T x C] products (Winograd weight gradient)
    p.x += (size_t)tap * p.x_bs;
    dy += (size_t)tap * p.y_bs;
    geo_tap = 0;
  }
  const int r = geo_tap / p.S, s = geo_tap - r * p.S;
  const int dyo = r * p.dil - p.pad, dxo = s * p.dil - p.pad;
  const int mbeg = blockIdx.z * pix_per_split;
  const int mend = min(p.M, mbeg + pix_per_split);
  const int ohw = p.OH * p.OW;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  // ---- per-thread staging descriptors: pointers advance by BP pixels per step; the pixel -> (n, y, x)
  // decode (two integer divisions) is only redone when a row of this thread wraps to the next image row
  const int a_ch = (tid % A_CPR) * 4, a_pr0 = tid / A_CPR;
  const int b_ch = (tid % B_CPR) * 4, b_pr0 = tid / B_CPR;
  const bool a_full = k0 + a_ch + 3 < p.K;          // whole float4 of output channels exists
  const bool a_act = !A_PART || a_pr0 < BP;
  const bool b_in = c0 + b_ch < p.C;
  const float* a_ptr[A_LD];
#pragma unroll
  for (int j = 0; j < A_LD; ++j) a_ptr[j] = dy + (size_t)(mbeg + a_pr0 + j * A_RPP) * lddy + k0 + a_ch;
  const size_t a_step = (size_t)BP * lddy;
  const float* b_ptr[B_LD];
  int b_n[B_LD], b_oy[B_LD], b_ox[B_LD], b_ix[B_LD];
  unsigned b_rowok = 0;
  auto place_row = [&](int j) {   // (n, oy, ox) -> source pointer / validity of the image row
    const int iy = b_oy[j] * p.stride + dyo;
    b_ix[j] = b_ox[j] * p.stride + dxo;
    const bool ok = b_in && b_n[j] < p.N && (unsigned)iy < (unsigned)p.H;
    b_rowok = (b_rowok & ~(1u << j)) | ((ok ? 1u : 0u) << j);
    b_ptr[j] = ok ? p.x + ((size_t)(b_n[j] * p.H + iy) * p.W) * p.ldx + c0 + b_ch : p.x;
  };
#pragma unroll
  for (int j = 0; j < B_LD; ++j) {
    const int m = mbeg + b_pr0 + j * B_RPP;
    const int n = m / ohw, rem = m - n * ohw;
    b_n[j] = n; b_oy[j] = rem / p.OW; b_ox[j] = rem - b_oy[j] * p.OW;
    place_row(j);
  }
  const bool has_affine = p.in_scale != nullptr;
  const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();
  f32x4 areg[A_LD], breg[B_LD], sreg[B_LD], hreg[B_LD];
  unsigned ld_ok = 0;
  int ld_m = mbeg;    // first pixel of the block the loader fetches next

  auto issue_loads = [&]() {
    const bool tail = ld_m + BP > mend;   // block-uniform: only the last step of a split can be ragged
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      const bool ok = a_act && (!tail || ld_m + a_pr0 + j * A_RPP < mend);
      const float* src = ok ? a_ptr[j] : dy + k0 + a_ch;
      f32x4 val;
      if (a_full) val = *reinterpret_cast<const f32x4*>(src);
      else {
        val.x = k0 + a_ch + 0 < p.K ? src[0] : 0.f;
        val.y = k0 + a_ch + 1 < p.K ? src[1] : 0.f;
        val.z = k0 + a_ch + 2 < p.K ? src[2] : 0.f;
        val.w = 0.f;
      }
      areg[j] = ok ? val : f32x4{0.f, 0.f, 0.f, 0.f};
      a_ptr[j] += a_step;
    }
    ld_ok = 0;
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      const bool ok = ((b_rowok >> j) & 1) && (unsigned)b_ix[j] < (unsigned)p.W &&
                      (!tail || ld_m + b_pr0 + j * B_RPP < mend);
      ld_ok |= (ok ? 1u : 0u) << j;
      const float* src = ok ? b_ptr[j] + (size_t)b_ix[j] * p.ldx : p.x;
      breg[j] = *reinterpret_cast<const f32x4*>(src);
      if (has_affine) {
        const size_t so = (ok ? (size_t)b_n[j] * p.in_ss_stride + c0 + b_ch : 0);
        sreg[j] = *reinterpret_cast<const f32x4*>(p.in_scale + so);
        hreg[j] = *reinterpret_cast<const f32x4*>(p.in_shift + so);
      }
      // advance this row's pixel by BP for the next step
      b_ox[j] += BP;
      b_ix[j] += BP * p.stride;
      if (b_ox[j] >= p.OW) {
        do { b_ox[j] -= p.OW; b_oy[j] += 1; } while (b_ox[j] >= p.OW);
        while (b_oy[j] >= p.OH) { b_oy[j] -= p.OH; b_n[j] += 1; }
        place_row(j);
      }
    }
    ld_m += BP;
  };
  auto finish_store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < A_LD; ++j)
      if (a_act) *reinterpret_cast<f32x4*>(&As[(buf * BP + a_pr0 + j * A_RPP) * LDA + a_ch]) = areg[j];
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      f32x4 val = breg[j];
      if (has_affine) val = val * sreg[j] + hreg[j];
      val.x = fmaxf(val.x, relu_floor); val.y = fmaxf(val.y, relu_floor);
      val.z = fmaxf(val.z, relu_floor); val.w = fmaxf(val.w, relu_floor);
      if (!((ld_ok >> j) & 1)) val = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(&Bs[(buf * BP + b_pr0 + j * B_RPP) * LDB + b_ch]) = val;
    }
  };

  const int fi = lane & 31, fk = lane >> 5;
  float fa[2][4][TM], fb[2][4][TN];
  auto load_frags = [&](int set, int buf, int kc) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int row = buf * BP + kc * 8 + ks * 2 + fk;
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[set][ks][i] = As[row * LDA + wm * WTK + i * 32 + fi];
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[set][ks][j] = Bs[row * LDB + wn * WTC + j * 32 + fi];
    }
  };
  auto mfma_chunk = [&](int set) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][ks][i], fb[set][ks][j], acc[i][j], 0, 0, 0);
  };

  const int n_it = mend > mbeg ? (mend - mbeg + BP - 1) / BP : 0;
  if (n_it > 0) { issue_loads(); finish_store(0); }
  __syncthreads();
  if (n_it > 0) load_frags(0, 0, 0);
  for (int it = 0; it < n_it; ++it) {
    const int buf = it & 1;
    // branch-free body (see the forward kernel): in the last step the loader runs past the split's
    // end, where every row is masked to a dummy address, and stages zeros nobody reads.
    // (The forward kernels' two-steps-ahead loader was measured here too: 104.8 -> 96.3 TFLOP/s. This loader's pixel
    // decode is VALU-heavy and does better at the top of the step, next to the fragment reads.)
    issue_loads();
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      if (kc + 1 < NKC) load_frags((kc + 1) & 1, buf, kc + 1);
      if (kc == NKC - 2) finish_store(buf ^ 1);
      if (kc == NKC - 1) {
        __syncthreads();
        load_frags(NKC & 1, buf ^ 1, 0);
      }
      mfma_chunk(kc & 1);
    }
  }

  const int colq = lane & 31, rowq = 4 * (lane >> 5);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    // rows in [K, Kpad) and columns in [C, Cp) were fed zeros, so their accumulators are exact zeros: storing them
    // too means every element of the [Kpad][Cp] slab is written and nobody has to clear it first
    const int col = c0 + wn * WTC + j * 32 + colq;
    if (col >= Cp) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = k0 + wm * WTK + i * 32 + (q & 3) + 8 * (q >> 2) + rowq;
        if (row < p.Kpad) dwp[(((size_t)blockIdx.z * gridDim.y + tap) * p.Kpad + row) * Cp + col] = acc[i][j][q];
      }
  }
}

// ------------------------------------------------------------------------------------------
// Batched TN GEMM for the Winograd-domain weight gradient: dU[p][k][c] = sum_t dY'[p][t][k] * X'[p][t][c].
// conv_wgrad_kernel computes the same thing with its convolution loader (pixel decode, tap geometry, per-row masks:
// 5 VALU instructions per MFMA) and one tile per workgroup; here nothing of that is left: both operands are plain
// row-major [T][channels] matrices, a PERSISTENT workgroup walks (position, k-tile, c-tile, T-range) work items, and the
// loader runs one 16-row step ahead, across work-item boundaries.
// MFMA rows = k, columns = c, contraction = t; LDS tiles [2][16][128+4]; fragments by ds_read_b32 (lane i reads column
// i of row 2s + (lane >> 5): 32 consecutive floats, conflict-free).
// Work item w = ((split * P + p) * ktiles + kt) * ctiles + ct; its 128x128 tile goes to slab `split` of dst.
constexpr int TN_BK = 128, TN_BC = 128, TN_BT = 16, TN_LD = 132;
__global__ __launch_bounds__(NT, 3) void gemm_tn_wgrad_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                              float* __restrict__ dst, int P, int T, int K, int C,
                                                              long long a_bs, long long b_bs, int Kpad, int Cp,
                                                              int ktiles, int ctiles, int splits, int t_per_split,
                                                              long long total) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                              // [2][16][132]
  float* Bs = smem + 2 * TN_BT * TN_LD;          // [2][16][132]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = tid >> 5, lcol = (tid & 31) * 4;        // loader: rows lrow, lrow + 8; 4 consecutive channels
  const long long stride = gridDim.x;

  // ---- loader state ----
  long long ld_w = mss_xcd_remap(blockIdx.x, gridDim.x);
  const float* a_ptr = A;
  const float* b_ptr = B;
  int ld_t = 0, ld_tend = 0;
  bool a_colok = false, b_colok = false;
  auto setup = [&](long long w) {
    const int ct = (int)(w % ctiles); w /= ctiles;
    const int kt = (int)(w % ktiles); w /= ktiles;
    const int p = (int)(w % P);
    const int sp = (int)(w / P);
    ld_t = sp * t_per_split;
    ld_tend = min(T, ld_t + t_per_split);
    a_colok = kt * TN_BK + lcol < K;             // K, C are multiples of 4: a float4 is inside or outside as a whole
    b_colok = ct * TN_BC + lcol < C;
    a_ptr = A + (size_t)p * a_bs + (size_t)ld_t * K + (a_colok ? kt * TN_BK + lcol : 0);
    b_ptr = B + (size_t)p * b_bs + (size_t)ld_t * C + (b_colok ? ct * TN_BC + lcol : 0);
  };
  f32x4 areg[2], breg[2];
  const bool edge_free = K % TN_BK == 0 && C % TN_BC == 0;
  auto issue_loads = [&]() {
    if (edge_free && ld_t + TN_BT <= ld_tend) {      // workgroup-uniform: no row or channel mask needed
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        areg[j] = *reinterpret_cast<const f32x4*>(a_ptr + (size_t)(lrow + 8 * j) * K);
        breg[j] = *reinterpret_cast<const f32x4*>(b_ptr + (size_t)(lrow + 8 * j) * C);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = ld_t + lrow + 8 * j;
      const bool ok = t < ld_tend;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const f32x4 va = *reinterpret_cast<const f32x4*>(ok ? a_ptr + (size_t)(lrow + 8 * j) * K : A);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(ok ? b_ptr + (size_t)(lrow + 8 * j) * C : B);
      areg[j] = (ok && a_colok) ? va : z;
      breg[j] = (ok && b_colok) ? vb : z;
    }
  };
  auto advance = [&]() {
    ld_t += TN_BT;
    if (ld_t < ld_tend) {
      a_ptr += (size_t)TN_BT * K;
      b_ptr += (size_t)TN_BT * C;
    } else {
      ld_w += stride;
      setup(ld_w < total ? ld_w : ld_w - stride);          // past the end: re-read the last item, never used
    }
  };
  auto finish_store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<f32x4*>(&As[(buf * TN_BT + lrow + 8 * j) * TN_LD + lcol]) = areg[j];
      *reinterpret_cast<f32x4*>(&Bs[(buf * TN_BT + lrow + 8 * j) * TN_LD + lcol]) = breg[j];
    }
  };
  const int fi = lane & 31, fk = lane >> 5;
  float fa[2][4][2], fb[2][4][2];
  auto load_frags = [&](int set, int buf, int kc) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int row = buf * TN_BT + kc * 8 + ks * 2 + fk;
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[set][ks][i] = As[row * TN_LD + wm * 64 + i * 32 + fi];
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[set][ks][j] = Bs[row * TN_LD + wn * 64 + j * 32 + fi];
    }
  };
  f32x16 acc[2][2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  };
  auto mfma_chunk = [&](int set) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][ks][i], fb[set][ks][j], acc[i][j], 0, 0, 0);
  };
  auto epilogue = [&](long long w) {
    const int ct = (int)(w % ctiles); w /= ctiles;
    const int kt = (int)(w % ktiles); w /= ktiles;      // w = split * P + p: the slab index
    float* o = dst + (size_t)w * Kpad * Cp;
    const int colq = lane & 31, rowq = 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = ct * TN_BC + wn * 64 + j * 32 + colq;
      if (col >= Cp) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = kt * TN_BK + wm * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + rowq;
          if (row < Kpad) o[(size_t)row * Cp + col] = acc[i][j][q];     // rows >= K / cols >= C were fed zeros
        }
    }
  };

  long long cur = ld_w;                     // item being multiplied (the launch guarantees cur < total)
  int steps_left;                           // 16-row steps left in the current item
  {
    long long w = cur / ((long long)ktiles * ctiles);
    const int sp = (int)(w / P);
    const int t0 = sp * t_per_split;
    steps_left = (min(T, t0 + t_per_split) - t0 + TN_BT - 1) / TN_BT;
  }
  setup(ld_w);
  issue_loads();
  finish_store(0);
  advance();
  zero_acc();
  __syncthreads();
  load_frags(0, 0, 0);
  int buf = 0;
  while (true) {
    issue_loads();                          // step +1, stored in this step
    load_frags(1, buf, 1);
    finish_store(buf ^ 1);
    advance();
    mfma_chunk(0);
    __syncthreads();
    load_frags(0, buf ^ 1, 0);
    mfma_chunk(1);
    buf ^= 1;
    if (--steps_left == 0) {
      epilogue(cur);
      cur += stride;
      if (cur >= total) break;
      zero_acc();
      long long w = cur / ((long long)ktiles * ctiles);
      const int sp = (int)(w / P);
      const int t0 = sp * t_per_split;
      steps_left = (min(T, t0 + t_per_split) - t0 + TN_BT - 1) / TN_BT;
    }
  }
}

// Same products, operands TRANSPOSED ON THE WAY INTO LDS so that the inner loop is the NT GEMM's (gemm.hip): waves 0-1 load
// A (dY'), waves 2-3 load B (X'); a thread fetches 4 consecutive t rows x 4 channels (each a coalesced 16-byte load), and the
// 4x4 block leaves for LDS as four ds_write_b128 of [channel][4 consecutive t] -- the transpose is register naming. LDS
// tiles are [128 channels][16 t + 4] with the NT kernel's chunk rotation, so a lane reads the 4 contraction steps of its
// channel with ONE ds_read_b128 (8 LDS reads per 32 MFMAs instead of 32 ds_read_b32). Arithmetic: the 16 t of a step are
// consumed in the order (s, s + 4 | s + 8, s + 12), s = 0..3, instead of (2s, 2s + 1): sums over t are re-associated, results
// differ from gemm_tn_wgrad_kernel in the last bits and are as deterministic (fixed order).
constexpr int TN2_LDK = 20;
// Tiles are 128 k x 256 c: 2x2 waves of 64 x 128, 2 workgroups per CU; every thread loads a 4x4 block of B and threads 0-127 one
// of A as well.
__global__ __launch_bounds__(NT, 2) void gemm_tn2_wgrad_kernel(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ dst, int P, int T, int K, int C, long long a_bs,
    long long b_bs, int Kpad, int Cp, int ktiles, int ctiles, int splits, int t_per_split, long long total) {
  constexpr int BC = 256, TNJ = BC / 64;                // c extent of a tile; 32-column MFMA blocks per wave
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                                   // [2][128][20]
  float* Bs = smem + 2 * 128 * TN2_LDK;               // [2][BC][20]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const long long stride = gridDim.x;
  // unit 0: B for every thread. unit 1 (threads 0-127): A.
  const int cq0 = tid & 63, tg0 = tid >> 6;
  // chunk rotation (r >> 2) + (r >> 4) of row r = 4 cq + e: the 16 lanes of a ds_write_b128 group then cover all 64 banks
  // (with (r >> 2) alone, rows 16 apart met in the same banks: PMC showed 2/3 of the LDS cycles as bank conflicts)
  float* const ldst0 = Bs + (4 * cq0) * TN2_LDK + ((tg0 + cq0 + (cq0 >> 2)) & 3) * 4;
  const bool has1 = tid < 128;                          // wave-uniform
  const int cq1 = tid & 31, tg1 = (tid >> 5) & 3;
  float* const ldst1 = As + (4 * cq1) * TN2_LDK + ((tg1 + cq1 + (cq1 >> 2)) & 3) * 4;

  const bool edge_free = K % 128 == 0 && C % BC == 0;   // no channel tile hangs over the edge: no per-lane column mask
  long long ld_w = mss_xcd_remap(blockIdx.x, gridDim.x);
  const float* ptr0 = B;
  const float* ptr1 = A;
  int ld_t = 0, ld_tend = 0;
  bool colok0 = false, colok1 = false;
  auto setup = [&](long long w) {
    const int ct = (int)(w % ctiles); w /= ctiles;
    const int kt = (int)(w % ktiles); w /= ktiles;
    const int p = (int)(w % P);
    const int sp = (int)(w / P);
    ld_t = sp * t_per_split;
    ld_tend = min(T, ld_t + t_per_split);
    const int col0 = ct * BC + 4 * cq0;
    colok0 = col0 < C;
    ptr0 = B + (size_t)p * b_bs + (size_t)ld_t * C + (colok0 ? col0 : 0);
    const int col1 = kt * 128 + 4 * cq1;
    colok1 = col1 < K;
    ptr1 = A + (size_t)p * a_bs + (size_t)ld_t * K + (colok1 ? col1 : 0);
  };
  f32x4 reg0[4], reg1[4];
  auto issue_loads = [&]() {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (edge_free && ld_t + 16 <= ld_tend) {        // workgroup-uniform: whole 16-row step inside, no ragged channel tile
#pragma unroll
      for (int e = 0; e < 4; ++e) reg0[e] = *reinterpret_cast<const f32x4*>(ptr0 + (size_t)(4 * tg0 + e) * C);
      if (has1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) reg1[e] = *reinterpret_cast<const f32x4*>(ptr1 + (size_t)(4 * tg1 + e) * K);
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 4 * tg0 + e;
      const bool ok = ld_t + r < ld_tend;
      const f32x4 v = *reinterpret_cast<const f32x4*>(ok ? ptr0 + (size_t)r * C : B);
      reg0[e] = (ok && colok0) ? v : z;
    }
    if (has1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * tg1 + e;
        const bool ok = ld_t + r < ld_tend;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ok ? ptr1 + (size_t)r * K : A);
        reg1[e] = (ok && colok1) ? v : z;
      }
    }
  };
  auto advance = [&]() {
    ld_t += 16;
    if (ld_t < ld_tend) {
      ptr0 += (size_t)16 * C;
      ptr1 += (size_t)16 * K;
    } else {
      ld_w += stride;
      setup(ld_w < total ? ld_w : ld_w - stride);
    }
  };
  auto finish_store = [&](int buf) {
    float* d = ldst0 + buf * BC * TN2_LDK;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x4 w = {reg0[0][e], reg0[1][e], reg0[2][e], reg0[3][e]};     // channel 4 cq + e, t = 4 tg .. 4 tg + 3
      *reinterpret_cast<f32x4*>(d + e * TN2_LDK) = w;
    }
    if (has1) {
      float* d1 = ldst1 + buf * 128 * TN2_LDK;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4 w = {reg1[0][e], reg1[1][e], reg1[2][e], reg1[3][e]};
        *reinterpret_cast<f32x4*>(d1 + e * TN2_LDK) = w;
      }
    }
  };
  const int frag_row = lane & 31, frag_h = lane >> 5;
  const int rot = (frag_row >> 2) + (frag_row >> 4);      // + 2 per 32-row block (the block base's (r >> 4) mod 4)
  const float* Abase = &As[(wm * 64 + frag_row) * TN2_LDK];
  const float* Bbase = &Bs[(wn * (BC / 2) + frag_row) * TN2_LDK];
  // logical chunk kc * 2 + frag_h of a row in an even / odd 32-row block
  const int koff[2][2] = {{((frag_h + rot) & 3) * 4, ((frag_h + rot + 2) & 3) * 4},
                          {((2 + frag_h + rot) & 3) * 4, ((2 + frag_h + rot + 2) & 3) * 4}};
  f32x4 fa[2][2], fb[2][TNJ];
  auto load_frags = [&](int set, int buf, int kc) {
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[set][i] = *reinterpret_cast<const f32x4*>(Abase + (buf * 128 + i * 32) * TN2_LDK + koff[kc][i & 1]);
#pragma unroll
    for (int j = 0; j < TNJ; ++j) fb[set][j] = *reinterpret_cast<const f32x4*>(Bbase + (buf * BC + j * 32) * TN2_LDK + koff[kc][j & 1]);
  };
  f32x16 acc[2][TNJ];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < TNJ; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  };
  auto mfma_chunk = [&](int set) {
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TNJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][s2], fb[set][j][s2], acc[i][j], 0, 0, 0);
  };
  auto epilogue = [&](long long w) {
    const int ct = (int)(w % ctiles); w /= ctiles;
    const int kt = (int)(w % ktiles); w /= ktiles;      // w = split * P + p: the slab index
    float* o = dst + (size_t)w * Kpad * Cp;
    const int colq = lane & 31, rowq = 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < TNJ; ++j) {
      const int col = ct * BC + wn * (BC / 2) + j * 32 + colq;
      if (col >= Cp) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = kt * 128 + wm * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + rowq;
          if (row < Kpad) o[(size_t)row * Cp + col] = acc[i][j][q];
        }
    }
  };

  long long cur = ld_w;
  int steps_left;
  {
    long long w = cur / ((long long)ktiles * ctiles);
    const int sp = (int)(w / P);
    const int t0 = sp * t_per_split;
    steps_left = (min(T, t0 + t_per_split) - t0 + 15) / 16;
  }
  setup(ld_w);
  issue_loads();
  finish_store(0);
  advance();
  zero_acc();
  __syncthreads();
  load_frags(0, 0, 0);
  int buf = 0;
  while (true) {
    issue_loads();                          // step +1, stored in this step
    load_frags(1, buf, 1);
    finish_store(buf ^ 1);
    advance();
    mfma_chunk(0);
    __syncthreads();
    load_frags(0, buf ^ 1, 0);
    mfma_chunk(1);
    buf ^= 1;
    if (--steps_left == 0) {
      epilogue(cur);
      cur += stride;
      if (cur >= total) break;
      zero_acc();
      long long w = cur / ((long long)ktiles * ctiles);
      const int sp = (int)(w / P);
      const int t0 = sp * t_per_split;
      steps_left = (min(T, t0 + t_per_split) - t0 + 15) / 16;
    }
  }
}

// dwp[tap][row][col] = sum over splits (ascending) of ws[split][tap][row][col], float4 over col (Cp % 4 == 0)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dwp,
                                                           long long slab4, int splits) {
  const f32x4* w4 = reinterpret_cast<const f32x4*>(ws);
  f32x4* d4 = reinterpret_cast<f32x4*>(dwp);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < slab4;
       i += (long long)gridDim.x * blockDim.x) {
    f32x4 a = w4[i];
    int sp = 1;
    for (; sp + 8 <= splits; sp += 8) {        // eight loads in flight, added in split order (the sum is bit-reproducible)
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = w4[(long long)(sp + u) * slab4 + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; sp < splits; ++sp) a += w4[(long long)sp * slab4 + i];
    d4[i] = a;
  }
}

// The same sum when there are MANY splits of a SMALL slab (the narrow head gradients: 1536 splits of 20 KB; a Linear of the pixel
// decoder: 256 splits of 256 KB): one thread per output float4 walks the splits one dependent load chain after the other
// (1536 / 8 round trips = 90 us for 30 MB). Here G threads share an output element: thread g adds the splits g, g + G, g + 2G, ...
// in ascending order, and the G partial sums are added in the order g = 0 .. G-1 through LDS -- a fixed tree, so the result is as
// reproducible as the sequential sum (it is a different rounding of the same sum).
template <int G>
__global__ __launch_bounds__(256) void wgrad_reduce_par_kernel(const float* __restrict__ ws, float* __restrict__ dwp, long long slab4,
                                                               int splits) {
  constexpr int EPB = 256 / G;                       // output float4s per workgroup
  __shared__ f32x4 part[G][EPB];
  const f32x4* w4 = reinterpret_cast<const f32x4*>(ws);
  const int el = threadIdx.x % EPB, g = threadIdx.x / EPB;
  const long long i = (long long)blockIdx.x * EPB + el;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (i < slab4) {
    int sp = g;
    for (; sp + 3 * G < splits; sp += 4 * G) {       // four loads in flight, added in ascending split order
      const f32x4 v0 = w4[(long long)sp * slab4 + i], v1 = w4[(long long)(sp + G) * slab4 + i];
      const f32x4 v2 = w4[(long long)(sp + 2 * G) * slab4 + i], v3 = w4[(long long)(sp + 3 * G) * slab4 + i];
      a += v0; a += v1; a += v2; a += v3;
    }
    for (; sp < splits; sp += G) a += w4[(long long)sp * slab4 + i];
  }
  part[g][el] = a;
  __syncthreads();
  if (g == 0 && i < slab4) {
    f32x4 t = part[0][el];
#pragma unroll
    for (int k = 1; k < G; ++k) t += part[k][el];
    reinterpret_cast<f32x4*>(dwp)[i] = t;
  }
}

// G: wg_reduce_group(slab4, splits) (wgrad_route.h)
inline void launch_wgrad_reduce(const float* ws, float* dwp, long long slab4, int splits, int G, hipStream_t stream) {
  if (G == 1) {
    long long blocks = (slab4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((int)blocks), dim3(256), 0, stream, ws, dwp, slab4, splits);
    return;
  }
#define RED(G_) hipLaunchKernelGGL(wgrad_reduce_par_kernel<G_>, dim3((unsigned)((slab4 + 256 / G_ - 1) / (256 / G_))), dim3(256), 0, stream, ws, dwp, slab4, splits)
  switch (G) {
    case 2: RED(2); break;
    case 4: RED(4); break;
    case 8: RED(8); break;
    case 16: RED(16); break;
    default: RED(32); break;
  }
#undef RED
}

// ---- TN weight gradient WITHOUT LDS (r04 experiment -> wgrad_route.h, MSS_WGRAD_TN=5 / default rule) --------------------------
// dW[k][c] = sum_r dy[r][k] * x[r][c]. In the 32x32x2 fp32 MFMA, operand A is [m][kk] with lane = m + 32 * kk: for THIS product the
// contraction index kk is the ROW of both operands, so the 32 lanes of one kk read 32 consecutive floats of one row -- the layout the
// tensors already have in memory. A lane therefore loads 16 bytes (4 consecutive columns) of row r0 + (lane >> 5) of dy and of x
// straight into registers and its four components feed four MFMAs each way: block (a, b) accumulates the output elements
// (k = k0 + 4 m + a, c = c0 + 4 n + b), i.e. the 128 x 128 tile of a WAVE is computed as 16 interleaved 32 x 32 blocks with
// 2 global loads per 16 MFMAs, no LDS staging, no transposing reads (gemm_tn_wgrad_kernel: one ds_read_b32 per MFMA and operand)
// and no workgroup barrier. The price: 256 accumulator registers per wave, so one wave per SIMD, and each operand row piece is
// fetched by every wave that needs it (from L2: 4 waves of a workgroup are the 4 column tiles of one k tile over the same rows).
// A ring of TND row pairs is in flight per wave. Output: whole 128 x 128 tiles of the (split, position) slab, 16-byte stores.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ const float tn_zero_row[4096] = {0.f};              // the A operand of rows past the end of a split
// AFFINE: x enters as relu(x * scale[c] + shift[c]) (the forward's BatchNorm + ReLU prologue, one affine for all rows), applied to the
// registers at consume time -- bot_aspp's 1280 -> 256 weight gradient (deepv3.py:235-240 reads the BN+ReLU of the five ASPP branches)
// PERIMG (batched, no splits): position-batch entry pb holds the rows of image pb % k_imgs alone, of which only the first
// cend = 16 * (k_base + k_steps[image]) columns exist (the dropped-channel X' of the composed ASPP route). A job whose c tile starts
// at or behind cend returns at once and leaves its tile of `out` unwritten; lanes whose columns lie behind cend inside a tile take
// their B operand from the row of zeros, so those columns of the tile are exact zeros and nothing behind cend is read.
template <bool AFFINE = false, bool PERIMG = false>
__global__ __launch_bounds__(256, 1) void gemm_tn_direct_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                                float* __restrict__ out, int P, int M, int K, int C, long long a_bs,
                                                                long long b_bs, int Kpad, int Cp, int ktiles, int ctiles, int splits,
                                                                int tps, long long total, long long full, float* __restrict__ tail_ws,
                                                                const float* __restrict__ scale = nullptr,
                                                                const float* __restrict__ shift = nullptr, int relu = 0, int lda = 0,
                                                                const int* __restrict__ k_steps = nullptr, int k_base = 0,
                                                                int k_imgs = 1, int pi_slots = 0) {
  if (lda <= 0) lda = K;               // row stride of A (dy): larger when dy is a channel slice of a wider buffer
  constexpr int KB = 4;                                        // 32-column blocks of dy per wave
  constexpr int TND = 8;                                       // row pairs per register block (two blocks: one consumed, one in flight)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // PERIMG, unpacked plan (MSS_WGRAD_PERIMG_PACK=0, more than TN_PERIMG_MAX_IMGS images): the jobs behind an image's extent are the
  // LAST c tiles of every (entry, k tile) -- with workgroups dealt round-robin to the 8 XCDs and 8 workgroups per (entry, k tile) at
  // C = 4096 they would all land on the same two XCDs. An XCD owns a contiguous run of workgroups instead, as in gemm_nt_kernel:
  // every XCD gets its share of live jobs, and the c tiles that read the same dY' rows share an L2.
  long long t;
  int sp = 0, nsp = 1;
  long long tail_tile = -1, ntail = 0;
  int ct, kt, pb;
  if (PERIMG && pi_slots > 0) {
    // PACKED per-image plan (tn_perimg_plan.h): live tiles numbered densely, the last partial round cut by rows when there is scratch
    // for its partial tiles (tail_ws). The plan is wave-uniform: k_steps comes in by scalar loads. Whole-tile jobs keep the
    // contiguous-run XCD ownership, over the LIVE workgroups only (the worst-case grid's surplus returns here); the tail round's
    // workgroups stay round-robin so that every XCD gets its share of the short jobs (full / 4 is a multiple of 8: slots % 32 == 0).
    const TnPerimgPlan pl = tn_perimg_plan(P / k_imgs, k_imgs, ktiles, ctiles, k_base, k_steps, pi_slots, M, tail_ws != nullptr);
    const int nwg = (int)((pl.total + 3) / 4), nrun = pl.tail ? (int)(pl.full / 4) : nwg;
    const int bid = (int)blockIdx.x;
    if (bid >= nwg) return;
    const long long job = (long long)(bid < nrun ? mss_xcd_remap(bid, nrun) : bid) * 4 + __builtin_amdgcn_readfirstlane(wave);
    TnPerimgJob jb;
    if (!tn_perimg_decode(pl, k_steps, job, jb)) return;
    ct = jb.ct; kt = jb.kt; pb = jb.pos * k_imgs + jb.img;
    if (jb.tail_tile >= 0) { sp = jb.sp; nsp = pl.splits; tail_tile = jb.tail_tile; ntail = pl.tail; tps = pl.tps; }
  } else {
    const long long job = (long long)(PERIMG ? mss_xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x) * 4 + wave;
    if (job >= total) return;                                   // no barrier anywhere in this kernel
    // Two job layouts. full < 0: every (position, tile) is cut into `splits` row ranges (slab per split in `out`, reduced afterwards).
    // full >= 0 (TAIL plan, r04: more tiles than wave slots and not a multiple of them -- 36 x 2 x 32 = 2304 tiles on 1024 SIMDs are
    // 2.25 rounds): the first `full` jobs are whole tiles written straight to the result; the remaining tiles are cut into `splits`
    // row ranges each, so that the last round is 1/splits as long; their partial tiles go to tail_ws [split][tail tile][128][128].
    t = job;
    if (full >= 0) {
      if (job >= full) {
        ntail = (total - full) / splits;
        sp = (int)((job - full) / ntail);
        tail_tile = (job - full) - (long long)sp * ntail;
        t = full + tail_tile;
        nsp = splits;
      }
    } else {
      nsp = splits;
    }
    ct = (int)(t % ctiles); t /= ctiles;
    kt = (int)(t % ktiles); t /= ktiles;
    if (full >= 0) pb = (int)t;
    else { sp = (int)(t % splits); pb = (int)(t / splits); }
  }
  const int half = lane >> 5, j = lane & 31;
  const int r0 = nsp > 1 ? sp * tps : 0, r1 = nsp > 1 ? (r0 + tps < M ? r0 + tps : M) : M;
  const float* a = A + (size_t)pb * a_bs + (size_t)(kt * (32 * KB) + KB * j);
  const float* b = B + (size_t)pb * b_bs + (size_t)(ct * 128 + 4 * j);
  size_t b_ld = (size_t)C;
  if (PERIMG) {
    const int cend = 16 * (k_base + k_steps[pb % k_imgs]);
    if (ct * 128 >= cend) return;                              // wave-uniform
    if (ct * 128 + 4 * j >= cend) { b = tn_zero_row + 4 * j; b_ld = 0; }
  }
  f32x16 acc[KB][4];
#pragma unroll
  for (int i = 0; i < KB; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][q][r] = 0.f;
  // Two register blocks of TND row pairs each: while the 4 * KB * TND MFMAs of one block run, the 2 * TND loads of the other are in
  // flight. Rows past the end of the split take their A operand from a row of zeros (tn_zero_row) and their B operand from the last
  // valid row: no mask arithmetic on loaded values (a use at fetch time would wait on the load; a multiply at consume time costs 4
  // VALU + hazard nops per 16 MFMAs). The loop body handles both blocks in straight-line code, so no
  // register of the ring is ever copied while its load is pending; the scheduling fences keep hipcc from sinking the loads down to
  // their uses (it does: shorter live ranges).
  f32x4 a0[TND], a1[TND];
  f32x4 b0[TND], b1[TND];
  const int last = r1 - 1;
  const float* az = tn_zero_row + (kt * (32 * KB) + KB * j);    // K <= 4096 (host check)
  auto fetch = [&](int row, f32x4& va, f32x4& vb) {
    const bool ok = row <= last;
    const size_t rr = (size_t)(ok ? row : last);
    va = *reinterpret_cast<const f32x4*>(ok ? a + rr * lda : az);  // a row past the end contributes A = 0: the product is zero
    vb = *reinterpret_cast<const f32x4*>(b + rr * (PERIMG ? b_ld : (size_t)C));
  };
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (AFFINE) {
    if (scale) sc = *reinterpret_cast<const f32x4*>(scale + ct * 128 + 4 * j);
    if (shift) sh = *reinterpret_cast<const f32x4*>(shift + ct * 128 + 4 * j);
  }
  const float fl = relu ? 0.f : -__builtin_huge_valf();
  auto compute = [&](const f32x4 (&va)[TND], const f32x4 (&vb)[TND]) {
#pragma unroll
    for (int d = 0; d < TND; ++d) {
      const f32x4 ca = va[d];
      f32x4 cb = vb[d];
      if (AFFINE) {
        cb = cb * sc + sh;
        cb.x = fmaxf(cb.x, fl); cb.y = fmaxf(cb.y, fl); cb.z = fmaxf(cb.z, fl); cb.w = fmaxf(cb.w, fl);
      }
#pragma unroll
      for (int i = 0; i < KB; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[i], cb[q], acc[i][q], 0, 0, 0);
    }
  };
  // (a mask-free main loop with a separate remainder loop was tried: a second loop that touches the accumulators makes hipcc keep
  // part of them in architectural registers and spill)
#pragma unroll
  for (int d = 0; d < TND; ++d) fetch(r0 + 2 * d + half, a0[d], b0[d]);
  for (int r = r0; r < r1; r += 4 * TND) {
#pragma unroll
    for (int d = 0; d < TND; ++d) fetch(r + 2 * TND + 2 * d + half, a1[d], b1[d]);
    __builtin_amdgcn_sched_barrier(0);
    compute(a0, b0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 0; d < TND; ++d) fetch(r + 4 * TND + 2 * d + half, a0[d], b0[d]);
    __builtin_amdgcn_sched_barrier(0);
    compute(a1, b1);
    __builtin_amdgcn_sched_barrier(0);
  }
  float* o;
  size_t ostride;
  if (tail_tile >= 0) {          // partial tile of the tail plan: compact [128][128]
    o = tail_ws + ((size_t)sp * ntail + tail_tile) * (128 * 128) + (size_t)(4 * j);
    ostride = 128;
  } else {
    o = out + ((size_t)(full >= 0 ? 0 : sp) * P + pb) * Kpad * Cp + (size_t)(kt * (32 * KB)) * Cp + (size_t)(ct * 128 + 4 * j);
    ostride = Cp;
  }
#pragma unroll
  for (int i = 0; i < KB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
      const f32x4 v = {acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
      *reinterpret_cast<f32x4*>(o + (size_t)(KB * m + i) * ostride) = v;
    }
}

// tail plan: result tile = sum over splits (ascending) of its partial tiles; one workgroup per (tail tile, 16 rows)
__global__ __launch_bounds__(256) void tn_tail_reduce_kernel(const float* __restrict__ tail_ws, float* __restrict__ dwp, long long full,
                                                             long long ntail, int splits, int ktiles, int ctiles, int Kpad, int Cp) {
  const long long ti = blockIdx.x / 16;
  const int part = blockIdx.x % 16;
  long long t = full + ti;
  const int ct = (int)(t % ctiles); t /= ctiles;
  const int kt = (int)(t % ktiles); t /= ktiles;
  const int pb = (int)t;
  const int e = part * 1024 + threadIdx.x * 4;                       // element of the 128 x 128 tile (4 consecutive columns)
  const int row = e >> 7, col = e & 127;
  const float* src = tail_ws + (size_t)ti * (128 * 128) + e;
  f32x4 a = *reinterpret_cast<const f32x4*>(src);
  for (int sp = 1; sp < splits; ++sp) a += *reinterpret_cast<const f32x4*>(src + (size_t)sp * ntail * (128 * 128));
  *reinterpret_cast<f32x4*>(dwp + (size_t)pb * Kpad * Cp + (size_t)(kt * 128 + row) * Cp + ct * 128 + col) = a;
}

// the same for the packed per-image plan: worst-case grid of (slots / 2) x 16 workgroups, the plan from tn_perimg_plan.h as in the
// kernel above; a workgroup at or behind the plan's tail tiles returns
__global__ __launch_bounds__(256) void tn_tail_reduce_perimg_kernel(const float* __restrict__ tail_ws, float* __restrict__ dwp, int P,
                                                                    int k_imgs, int ktiles, int ctiles, int k_base,
                                                                    const int* __restrict__ k_steps, int slots, int rows, int Kpad,
                                                                    int Cp) {
  const int ti = blockIdx.x / 16, part = blockIdx.x % 16;
  const TnPerimgPlan pl = tn_perimg_plan(P, k_imgs, ktiles, ctiles, k_base, k_steps, slots, rows, 1);
  if (ti >= pl.tail) return;
  TnPerimgJob jb;
  if (!tn_perimg_decode(pl, k_steps, pl.full + ti, jb)) return;
  const int pb = jb.pos * k_imgs + jb.img;
  const int e = part * 1024 + threadIdx.x * 4;
  const int row = e >> 7, col = e & 127;
  const float* src = tail_ws + (size_t)ti * (128 * 128) + e;
  f32x4 a = *reinterpret_cast<const f32x4*>(src);
  for (int sp = 1; sp < pl.splits; ++sp) a += *reinterpret_cast<const f32x4*>(src + (size_t)sp * pl.tail * (128 * 128));
  *reinterpret_cast<f32x4*>(dwp + (size_t)pb * Kpad * Cp + (size_t)(jb.kt * 128 + row) * Cp + jb.ct * 128 + col) = a;
}

// ---- narrow weight gradients (K <= 64 output channels: the 19-channel heads, bot_fine's 48) without LDS (r04) -----------------------
// dW[k][c] = sum_r dy[r][k] * act(x[r][c]) with a handful of output channels is a STREAM over x (1.07 GB for the 256-channel head
// input at 2 x 512 x 1024) with 2 K FLOP per element: conv_wgrad_kernel<32 / 64, 128, 16> stages 16 pixels at a time through LDS
// and runs at 2.4-3.0 TB/s. Here, as in gemm_tn_direct_kernel, the operands go from global memory straight into the MFMA layout:
// lane (j, half) loads KB2 floats of dy row r + half (columns KB2 * j ..; lanes past K read a row of zeros) and 16 bytes of x
// (channels ct * 128 + 4 j ..), 4 * KB2 MFMAs per row pair, a wave owns a [32 * KB2] x 128 tile (64 / 128 accumulators), two or three
// waves per SIMD keep >= 16 KB per wave in flight. The BatchNorm + ReLU prologue of the forward (deepv3.py:235-252) is applied to the
// x registers at consume time. Partial tiles per row split in slabs, added in split order by wgrad_reduce_kernel: deterministic.
__device__ float tn_zeros_rt[64];          // zero-initialised and never written; NOT const, so that the compiler keeps `cond ? row : zeros`
                                           // a select of two addresses in front of ONE load (a const array of zeros folds to a branch around the load)
template <int KB2, bool AFFINE>
__global__ __launch_bounds__(256, 2) void gemm_tn_narrow_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                int relu, float* __restrict__ out, int M, int K, int Kpad, int Cp,
                                                                int ctiles, int tps, long long total) {
  typedef typename std::conditional<KB2 == 2, f32x2, float>::type avec;
  constexpr int TND = 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long job = (long long)blockIdx.x * 4 + wave;
  if (job >= total) return;
  const int ct = (int)(job % ctiles), sp = (int)(job / ctiles);
  const int half = lane >> 5, j = lane & 31;
  const int r0 = sp * tps, r1 = r0 + tps < M ? r0 + tps : M;
  const bool a_ok = KB2 * j + KB2 - 1 < K;
  const float* a = A + KB2 * j;
  const float* b = B + (size_t)(ct * 128 + 4 * j);
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (AFFINE) {
    if (scale) sc = *reinterpret_cast<const f32x4*>(scale + ct * 128 + 4 * j);
    if (shift) sh = *reinterpret_cast<const f32x4*>(shift + ct * 128 + 4 * j);
  }
  const float fl = relu ? 0.f : -__builtin_huge_valf();
  f32x16 acc[KB2][4];
#pragma unroll
  for (int i = 0; i < KB2; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][q][r] = 0.f;
  avec a0[TND], a1[TND];
  f32x4 b0[TND], b1[TND];
  const int last = r1 - 1;
  auto fetch = [&](int row, avec& va, f32x4& vb) {
    const bool ok = row <= last;
    const size_t rr = (size_t)(ok ? row : last);
    va = *reinterpret_cast<const avec*>((ok && a_ok) ? a + rr * lda : tn_zeros_rt);
    vb = *reinterpret_cast<const f32x4*>(b + rr * ldb);
  };
  auto compute = [&](const avec (&va)[TND], const f32x4 (&vb)[TND]) {
#pragma unroll
    for (int d = 0; d < TND; ++d) {
      f32x4 cb = vb[d];
      if (AFFINE) {
        cb = cb * sc + sh;
        cb.x = fmaxf(cb.x, fl); cb.y = fmaxf(cb.y, fl); cb.z = fmaxf(cb.z, fl); cb.w = fmaxf(cb.w, fl);
      }
#pragma unroll
      for (int i = 0; i < KB2; ++i) {
        float ai;
        if constexpr (KB2 == 2) ai = va[d][i]; else ai = va[d];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, cb[q], acc[i][q], 0, 0, 0);
      }
    }
  };
#pragma unroll
  for (int d = 0; d < TND; ++d) fetch(r0 + 2 * d + half, a0[d], b0[d]);
  for (int r = r0; r < r1; r += 4 * TND) {
#pragma unroll
    for (int d = 0; d < TND; ++d) fetch(r + 2 * TND + 2 * d + half, a1[d], b1[d]);
    __builtin_amdgcn_sched_barrier(0);
    compute(a0, b0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 0; d < TND; ++d) fetch(r + 4 * TND + 2 * d + half, a0[d], b0[d]);
    __builtin_amdgcn_sched_barrier(0);
    compute(a1, b1);
    __builtin_amdgcn_sched_barrier(0);
  }
  float* o = out + (size_t)sp * Kpad * Cp + (size_t)(ct * 128 + 4 * j);
#pragma unroll
  for (int i = 0; i < KB2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = KB2 * ((r & 3) + 8 * (r >> 2) + 4 * half) + i;
      const f32x4 v = {acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
      if (k < Kpad) *reinterpret_cast<f32x4*>(o + (size_t)k * Cp) = v;       // rows K .. Kpad-1: zeros (their A lanes read the zero row)
    }
}

// ---- launchers: each takes the WgradRoute of wgrad_route.h as it is ----

// splits > 1: the kernel wrote every element of every partial slab of ws (see the kernels' epilogues), so whole slabs are swept
inline int finish_splits(const WgradRoute& r, const MssConvArgs& p, int Cp, const float* ws, float* dwp, hipStream_t stream) {
  if (r.splits > 1) launch_wgrad_reduce(ws, dwp, (long long)r.positions * p.Kpad * Cp / 4, r.splits, r.reduce_group, stream);
  return mss_launch_status();
}

template <int BKO, int WK>
int launch_wgrad_conv(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, int Cp, float* ws, hipStream_t stream) {
  constexpr int BCI = 128, BP = 16;
  const size_t smem = (size_t)2 * BP * (BKO + 4 + BCI + 4) * sizeof(float);
  // staging after the whole MFMA block, and BP=32, were measured: within 1-4 % slower
  auto kern = conv_wgrad_kernel<BKO, BCI, BP, WK>;
  hipLaunchKernelGGL(kern, dim3(r.ktiles * r.ctiles, r.positions, r.splits), dim3(NT), smem, stream, p, dy, lddy,
                     r.splits > 1 ? ws : dwp, Cp, r.rows_per_split);
  return finish_splits(r, p, Cp, ws, dwp, stream);
}

int launch_wgrad_narrow(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, int Cp, float* ws, hipStream_t stream) {
  float* out = r.splits > 1 ? ws : dwp;
  const bool aff = wg_has_prologue(p);
  const dim3 grid((unsigned)((r.total + 3) / 4));
#define NARROW(KB2_, AFF_)                                                                                                          \
  hipLaunchKernelGGL((gemm_tn_narrow_kernel<KB2_, AFF_>), grid, dim3(256), 0, stream, dy, lddy, p.x, p.ldx, p.in_scale, p.in_shift,  \
                     p.in_relu, out, p.M, p.K, p.Kpad, Cp, r.ctiles, r.rows_per_split, r.total)
  if (p.K <= 32) { if (aff) NARROW(1, true); else NARROW(1, false); }
  else { if (aff) NARROW(2, true); else NARROW(2, false); }
#undef NARROW
  return finish_splits(r, p, Cp, ws, dwp, stream);
}

// The one launch of gemm_tn_direct_kernel: `jobs` one-wave jobs of the route's plan into `out`; tail_ws: where the row ranges of a
// tail plan leave their partial tiles (else null); slots: the packed per-image plan's wave slots (0: the unpacked one, or no k_steps).
void launch_tn_direct(const WgradRoute& r, const MssConvArgs& p, long long jobs, const float* dy, int lddy, float* out, int Cp,
                      float* tail_ws, int slots, hipStream_t stream) {
  const bool perimg = p.k_steps != nullptr, aff = wg_has_prologue(p);      // (the per-image form has no prologue: checked at entry)
  const long long a_bs = p.batch > 1 ? p.y_bs : 0, b_bs = p.batch > 1 ? p.x_bs : 0;
  auto kern = perimg ? gemm_tn_direct_kernel<false, true> : aff ? gemm_tn_direct_kernel<true, false> : gemm_tn_direct_kernel<false, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((jobs + 3) / 4)), dim3(256), 0, stream, dy, p.x, out, r.positions, p.M, p.K, p.C, a_bs, b_bs,
                     p.Kpad, Cp, r.ktiles, r.ctiles, r.splits, r.rows_per_split, jobs, r.full, tail_ws, aff ? p.in_scale : (const float*)nullptr,
                     aff ? p.in_shift : (const float*)nullptr, aff ? p.in_relu : 0, lddy, p.k_steps, p.k_base, p.k_imgs, slots);
}

int launch_wgrad_tn_direct(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, int Cp, float* ws, hipStream_t stream) {
  if (r.full >= 0) {      // WG_TN_DIRECT_TAIL: whole tiles straight into dwp, the tail tiles' row ranges into ws, added in ascending split order
    const long long ntail = (r.total - r.full) / r.splits;
    launch_tn_direct(r, p, r.total, dy, lddy, dwp, Cp, ws, 0, stream);
    hipLaunchKernelGGL(tn_tail_reduce_kernel, dim3((unsigned)(ntail * 16)), dim3(256), 0, stream, ws, dwp, r.full, ntail, r.splits,
                       r.ktiles, r.ctiles, p.Kpad, Cp);
    return mss_launch_status();
  }
  launch_tn_direct(r, p, r.total, dy, lddy, r.splits > 1 ? ws : dwp, Cp, nullptr, 0, stream);
  return finish_splits(r, p, Cp, ws, dwp, stream);
}

// per-image entries over channel-compacted columns. Packed plan (tn_perimg_plan.h, default): the live tiles numbered densely
// on the device, the grid sized here for the worst case (every column kept; the host never reads k_steps). With scratch of
// slots x 64 KiB (MSS_WGRAD_PERIMG_TAIL_BYTES at the default 1024 slots) the last partial round is cut by rows and a reduce
// launch adds its partial tiles in ascending split order; without it every job is a whole tile.
int launch_wgrad_tn_perimg(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, int Cp, float* ws,
                           long long ws_bytes, const WgradSwitches& sw, hipStream_t stream) {
  if (sw.perimg_pack != 0 && p.k_imgs <= TN_PERIMG_MAX_IMGS) {
    int slots = sw.tn_slots / 32 * 32;      // per-image plan only (tests reach the tail plan)
    slots = slots < 32 ? 32 : slots > TN_PERIMG_MAX_SLOTS ? TN_PERIMG_MAX_SLOTS : slots;
    const int P = p.batch / p.k_imgs;
    const bool tail = sw.tn_tail != 0 && ws && ws_bytes >= (long long)slots * (128 * 128 * 4) && r.total > slots;
    const long long jobs = tn_perimg_worst_jobs(P, p.k_imgs, r.ktiles, r.ctiles, slots, tail);
    launch_tn_direct(r, p, jobs, dy, lddy, dwp, Cp, tail ? ws : nullptr, slots, stream);
    if (tail)
      hipLaunchKernelGGL(tn_tail_reduce_perimg_kernel, dim3((unsigned)(slots / 2 * 16)), dim3(256), 0, stream, ws, dwp, P, p.k_imgs, r.ktiles,
                         r.ctiles, p.k_base, p.k_steps, slots, p.M, p.Kpad, Cp);
    return mss_launch_status();
  }
  // unpacked: one whole-tile job per (entry, k tile, c tile); the jobs behind an image's extent return at once. No splits, no scratch.
  launch_tn_direct(r, p, r.total, dy, lddy, dwp, Cp, nullptr, 0, stream);
  return mss_launch_status();
}

// The persistent LDS kernels: the grid is the resident workgroups (an occupancy query, once), each walking the route's jobs.
int launch_wgrad_tn_lds(const WgradRoute& r, const MssConvArgs& p, const float* dy, float* dwp, int Cp, float* ws, hipStream_t stream) {
  const bool wide = r.kernel == WG_TN_WIDE;
  const long long a_bs = p.batch > 1 ? p.y_bs : 0, b_bs = p.batch > 1 ? p.x_bs : 0;
  const size_t smem = (size_t)4 * TN_BT * TN_LD * sizeof(float);
  MssKernelInfo ki;
  if (int rc = mss_kernel_info<gemm_tn_wgrad_kernel>(NT, smem, 3, &ki)) return rc;
  const long long slots = (long long)(wide ? 2 : ki.occ > 3 ? 3 : ki.occ) * ki.cus;
  const int grid = (int)(r.total < slots ? r.total : slots);
  float* out = r.splits > 1 ? ws : dwp;
  if (wide) {
    const size_t smem2 = (size_t)2 * (128 + 256) * TN2_LDK * sizeof(float);
    hipLaunchKernelGGL(gemm_tn2_wgrad_kernel, dim3(grid), dim3(NT), smem2, stream, dy, p.x, out, r.positions, p.M, p.K, p.C, a_bs,
                       b_bs, p.Kpad, Cp, r.ktiles, r.ctiles, r.splits, r.rows_per_split, r.total);
  } else {
    hipLaunchKernelGGL(gemm_tn_wgrad_kernel, dim3(grid), dim3(NT), smem, stream, dy, p.x, out, r.positions, p.M, p.K, p.C, a_bs,
                       b_bs, p.Kpad, Cp, r.ktiles, r.ctiles, r.splits, r.rows_per_split, r.total);
  }
  return finish_splits(r, p, Cp, ws, dwp, stream);
}

const WgradSplitBf16 split_bf16 = {mss_wgrad_tn_bf16x3_eligible, mss_wgrad_tn_bf16x3_ws_bytes, mss_wgrad_tn_bf16x3_plan};

// read per call through the cached lookup (mss_env_reset: tests switch routes inside one process)
WgradSwitches wgrad_switches() {
  WgradSwitches sw;
  sw.tn = MSS_ENV_INT("MSS_WGRAD_TN", 5);
  sw.tn_affine = MSS_ENV_INT("MSS_WGRAD_TN_AFFINE", 1);
  sw.tn_tail = MSS_ENV_INT("MSS_WGRAD_TN_TAIL", 1);
  sw.narrow = MSS_ENV_INT("MSS_WGRAD_NARROW", 1);
  sw.perimg_pack = MSS_ENV_INT("MSS_WGRAD_PERIMG_PACK", 1);
  sw.tn_slots = MSS_ENV_INT("MSS_WGRAD_TN_SLOTS", TN_PERIMG_MAX_SLOTS);
  return sw;
}

// One product on the kernel its route names (wgrad_resolve's: already the native one where the scratch is too small for the split-bf16 kernel).
int launch_route(const WgradRoute& r, const MssConvArgs& p, const float* dy, int lddy, float* dwp, int Cp, float* ws, long long ws_bytes,
                 const WgradSwitches& sw, hipStream_t s) {
  if (r.ws_bytes > 0 && (!ws || ws_bytes < r.ws_bytes)) return MSS_ERR_BAD_ARG;
  switch (r.kernel) {
    case WG_TN_BF16X3: return mss_wgrad_tn_bf16x3_launch(p, dy, lddy, dwp, Cp, ws, ws_bytes, s);
    case WG_TN_DIRECT_PERIMG: return launch_wgrad_tn_perimg(r, p, dy, lddy, dwp, Cp, ws, ws_bytes, sw, s);
    case WG_TN_DIRECT:
    case WG_TN_DIRECT_TAIL: return launch_wgrad_tn_direct(r, p, dy, lddy, dwp, Cp, ws, s);
    case WG_TN_WIDE:
    case WG_TN_LDS: return launch_wgrad_tn_lds(r, p, dy, dwp, Cp, ws, s);
    case WG_NARROW: return launch_wgrad_narrow(r, p, dy, lddy, dwp, Cp, ws, s);
    case WG_CONV_32: return launch_wgrad_conv<32, 1>(r, p, dy, lddy, dwp, Cp, ws, s);
    case WG_CONV_64: return launch_wgrad_conv<64, 2>(r, p, dy, lddy, dwp, Cp, ws, s);
    case WG_CONV_128: return launch_wgrad_conv<128, 2>(r, p, dy, lddy, dwp, Cp, ws, s);
    case WG_STEM7: return mss_stem7_wgrad_launch(r, p, dy, lddy, dwp, ws, s);
    case WG_TWO_PART: break;      // (mss_conv2d_wgrad_f32 launches its parts)
  }
  return MSS_ERR_BAD_ARG;
}

}  // namespace

void mss_wgrad_reduce_launch(const float* ws, float* dwp, long long slab4, int splits, hipStream_t stream) {
  launch_wgrad_reduce(ws, dwp, slab4, splits, wg_reduce_group(slab4, splits), stream);
}

extern "C" {

// 1 when mss_conv2d_wgrad_f32 evaluates these arguments (for a two-part product: its first part) with the split-bf16 TN kernel
// (args->route == 1 and the shape eligible), else 0. Profiling label: Cp == C and aligned pointers are assumed.
int mss_conv2d_wgrad_route(const MssConvArgs* args, int lddy) {
  MssConvArgs p = *args;
  p.M = p.N * p.OH * p.OW;
  if (p.M <= 0 || wg_stem7_form(p, 4)) return 0;
  const WgradSwitches sw = wgrad_switches();
  WgradFacts f;
  f.dense_dy = lddy == p.K;
  WgradRoute r = wgrad_route(p, lddy, p.C, f, sw, split_bf16);
  if (r.kernel == WG_TWO_PART) { f.dense_dy = false; r = wgrad_route(wgrad_part(p, r.wide_K, false), lddy, p.C, f, sw, split_bf16); }
  return r.kernel == WG_TN_BF16X3 ? 1 : 0;
}

// Bytes of scratch mss_conv2d_wgrad_f32 needs for these arguments (0: the pixel range is not split).
long long mss_conv2d_wgrad_workspace_bytes(const MssConvArgs* args, int Cp) {
  MssConvArgs p = *args;
  p.M = p.N * p.OH * p.OW;
  if (p.M <= 0) return 0;
  if (wg_stem7_form(p, Cp)) return wg_plan_stem7(p).ws_bytes;      // (the plan wgrad_resolve gives the launch)
  return wgrad_workspace_bytes(p, Cp, wgrad_switches(), split_bf16);
}

// dwp ([R*S][Kpad][Cp], Kpad >= K, Cp >= C multiples of 4) is fully overwritten (padding = 0); args
// describes the *forward* conv (x, geometry, optional prologue on x); dy is the NHWC output gradient with pixel
// stride lddy; ws: scratch of mss_conv2d_wgrad_workspace_bytes bytes (may be NULL when that is 0), contents
// irrelevant on entry. Deterministic: no atomics, fixed summation order.
int mss_conv2d_wgrad_f32(MssConvArgs* args, const float* dy, int lddy, float* dwp, int Cp, float* ws,
                         long long ws_bytes, void* stream) {
  const WgradSwitches sw = wgrad_switches();
  WgradCall c;
  if (const int rc = wgrad_resolve(args, dy, lddy, dwp, Cp, ws_bytes, sw, split_bf16, c)) return rc;
  if (c.empty) return MSS_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (c.route.kernel != WG_TWO_PART) return launch_route(c.route, c.p, dy, lddy, dwp, Cp, ws, ws_bytes, sw, s);
  // both parts one after the other on the same scratch, each writing its own rows of dwp
  const int wide = c.route.wide_K;
  const int rc = launch_route(c.part_route[0], c.part[0], dy, lddy, dwp, Cp, ws, ws_bytes, sw, s);
  if (rc != MSS_OK) return rc;
  return launch_route(c.part_route[1], c.part[1], dy + wide, lddy, dwp + (size_t)wide * Cp, Cp, ws, ws_bytes, sw, s);
}

// What that call launches: the same wgrad_resolve, nothing else (include/mss_hip.h).
int mss_conv2d_wgrad_plan(const MssConvArgs* args, const float* dy, int lddy, const float* dwp, int Cp, long long ws_bytes, int part,
                          MssWgradPlan* out) {
  if (!args || !out || part < 0 || part > 2) return MSS_ERR_BAD_ARG;
  WgradCall c;
  if (const int rc = wgrad_resolve(args, dy, lddy, dwp, Cp, ws_bytes, wgrad_switches(), split_bf16, c)) return rc;
  MssWgradPlan o = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!c.empty) {
    if (part != 0 && c.route.kernel != WG_TWO_PART) return MSS_ERR_BAD_ARG;
    const WgradRoute& r = part == 0 ? c.route : c.part_route[part - 1];
    o.kernel = r.kernel; o.ktiles = r.ktiles; o.ctiles = r.ctiles; o.positions = r.positions; o.splits = r.splits;
    o.rows_per_split = r.rows_per_split; o.total = r.total; o.full = r.full; o.ws_bytes = r.ws_bytes; o.wide_K = r.wide_K;
    o.reduce_group = r.reduce_group;
  } else if (part != 0) {
    return MSS_ERR_BAD_ARG;
  }
  *out = o;
  return MSS_OK;
}

}  // extern "C"
