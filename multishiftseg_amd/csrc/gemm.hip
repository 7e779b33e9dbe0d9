// Persistent NT GEMM on the fp32 matrix cores: Y[b][m][n] = sum_c act(X[b][m][c]) * W[b][n][c]  (+ epilogue).
//
// This is the 1x1 / stride-1 / padding-0 case of conv_igemm.hip without the implicit-GEMM machinery (no taps, no
// pixel decode, no dead-tap mask): the batched Winograd-domain products (winograd.hip; 36 GEMMs of
// [tiles x C] x [C x K] per layer), mask prediction of the M2F head, and the pre-activation 1x1 convolutions of the
// WideResNet trunk (wider_resnet.py:121-131,157) and the heads (deepv3.py:66,235-252).
//
// The inner loop is conv_igemm's (128x128x16 tile, 4 waves of 64x64, LDS double buffer with +4-float row padding,
// fragments double-buffered in registers, one barrier per K-step). What is new is the schedule around it: a
// workgroup is PERSISTENT and walks tiles t, t + grid, t + 2 grid, ...; the loader runs one K-step ahead ACROSS tile
// boundaries, so while the last K-step of a tile multiplies, the first K-step of the next tile is already on its way
// from HBM and lands in the other LDS buffer; the epilogue's stores are issued and the MFMAs of the next tile start
// right behind them. With short reductions (C = 128..512, i.e. 8..32 K-steps per tile) the start-up/drain of every
// tile was ~5 K-steps' worth of time in the one-tile-per-workgroup kernel.
//
// Tile order is n-fastest and an XCD owns a contiguous run of tiles, so the n-tiles that share an X tile hit in the
// same L2.
#include "mss_epilogue.h"
#include "mss_gemm_tiles.h"
#include "fwd_route.h"
#include <stdlib.h>

namespace {

constexpr int NT = 256, BM = MSS_GEMM_BM, BK = MSS_GEMM_BK;
// LDS rows are 16 floats with NO padding; the four 16-byte chunks of row r are rotated by (r >> 2): a staging write
// (16 lanes = 4 rows x 4 chunks) and a fragment read (16 lanes = 16 rows x 1 chunk) then both touch 16 disjoint
// 4-bank spans. (The +4-float padding of conv_igemm is conflict-free for the reads only: PMC showed a third of the
// LDS cycles as bank conflicts from the ds_write_b128 side.)
constexpr int LDK = BK;
constexpr int WTM = 64, TM = 2;
constexpr int CPR = BK / 4;            // float4 chunks per tile row
constexpr int RPP = NT / CPR;          // rows staged per pass
constexpr int A_LD = BM / RPP;
constexpr int NKC = BK / 8;

static_assert(NKC == 2, "the step body below is written for two 8-k chunks");

// VARIANT (MSS_GEMM_VARIANT): 2 = the loader runs TWO steps ahead with one register set: step k first stores the registers
// (step k+1's data, requested a whole step ago) to LDS and immediately re-issues them for step k+2, so no wave waits on a load it
// has just issued; 3 = the same with 32-bit operand offsets (below). (Variants 0 and 1, the loads one step ahead, were removed
// after round 6.)
// BN: output-channel extent of a tile. 128 (2x2 waves of 64x64, 4 workgroups per CU) or 256 (2x2 waves of 64x128: 64 MFMAs
// per wave and barrier instead of 32, a quarter less operand traffic per FLOP and half the per-tile prologue/epilogue
// share, at 2 workgroups per CU).
// PERIMG (variant 3, no prologue): the reduction length and the weights belong to the IMAGE a row tile lies in -- p.k_steps[img]
// K-steps over the weights at p.w + img * p.w_img_stride, img = (mt * BM) / p.H (p.H = rows per image; tiles never straddle images).
// The product behind csrc/chan_compact.hip: Dropout2d-zeroed input channels are compacted away per sample, so image n multiplies
// only its kept channels. Both numbers are uniform over a tile: k_steps[img] is read where the tile's offsets are formed (setup_off),
// the K-step body gains one scalar select. With p.k_imgs > 0 the images are the batch entries' (entry b belongs to image b % k_imgs) and
// every image runs p.k_base further K-steps in front.
template <bool AFFINE, int VARIANT, int BN, bool PERIMG = false>
__global__ __launch_bounds__(NT, BN == 256 ? 2 : 3) void gemm_nt_kernel(MssConvArgs p, long long first_tile, long long total_tiles,
                                                                        int tiles_per_batch, int group_m) {
  static_assert(!PERIMG || (VARIANT == 3 && !AFFINE), "the per-image mode exists on the variant-3 kernel without prologue only");
  constexpr int WTN = BN / 2, TN = WTN / 32, B_LD = BN / RPP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                       // [2][BM][LDK]
  float* Bs = As + 2 * BM * LDK;          // [2][BN][LDK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int chunk = tid % CPR, row0 = tid / CPR;
  const int wchunk = (chunk + (row0 >> 2)) & 3;          // RPP = 64 rows per pass: (row0 + j * 64) >> 2 has the same low bits
  const int n_it = p.C / BK;
  int cur_nit = n_it, ld_nit = n_it, nit_nxt = n_it;   // PERIMG: K-steps of the tile being multiplied / the loader is in / enters next
  const long long stride = gridDim.x;
  const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();

  // ---- loader state: the K-step the next issue_loads() fetches ----
  // VARIANT 3 (r03): 32-bit byte offsets from the (uniform) operand bases instead of 64-bit pointers, the offsets of the
  // workgroup's NEXT tile kept beside the current ones, and a branch-free advance() (a select on "this was the tile's last
  // K-step"): the K-step body becomes ONE basic block, which is what lets the requests below interleave the loader's
  // instructions with the MFMAs instead of leaving them in a clump in front of them (a 32x32x2 f32 MFMA holds the pipe for
  // 64 cycles; in variant 2 this wave issues ~45 other instructions with no MFMA in flight every K-step).
  const float* a_ptr[A_LD];
  const float* b_ptr[B_LD];
  unsigned a_off[A_LD], b_off[B_LD], a_nxt[A_LD], b_nxt[B_LD], s_off = 0, s_nxt = 0;
  const float* s_ptr = p.in_scale;
  const float* h_ptr = p.in_shift;
  long long ld_tile = first_tile + mss_xcd_remap(blockIdx.x, gridDim.x);   // this launch walks tiles [first_tile, total_tiles)
  int ld_k = 0;
  auto setup_off = [&](long long t, unsigned* ao, unsigned* bo, unsigned& so, int& nit) {
    const int b = (int)(t / tiles_per_batch);
    const int v = (int)(t - (long long)b * tiles_per_batch);
    int mt, nt; mss_tile_mn(v, p.mtiles, p.ntiles, group_m, mt, nt);
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      int row = mt * BM + row0 + j * RPP;
      row = row < p.M ? row : p.M - 1;
      ao[j] = (unsigned)(((size_t)b * p.x_bs + (size_t)row * p.ldx + chunk * 4) * sizeof(float));
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j)
      bo[j] = (unsigned)(((size_t)b * p.w_bs + (size_t)(nt * BN + row0 + j * RPP) * p.C + chunk * 4) * sizeof(float));
    if (PERIMG) {
      // p.k_imgs > 0 (the Winograd-domain products of the composed ASPP route): batch entry b = (position, image) holds ONE image's
      // rows, so a row tile never straddles images and the entry's weights are its own (w_bs; w_img_stride is 0); the first p.k_base
      // K-steps are columns every image has (the factor without Dropout2d)
      const int img = p.k_imgs > 0 ? b % p.k_imgs : (mt * BM) / p.H;
      nit = p.k_steps[img] + p.k_base;
      const unsigned wo = (unsigned)((size_t)img * (size_t)p.w_img_stride * sizeof(float));
#pragma unroll
      for (int j = 0; j < B_LD; ++j) bo[j] += wo;
    }
    if (AFFINE) so = (unsigned)(((size_t)((mt * BM) / p.H) * p.in_ss_stride + chunk * 4) * sizeof(float));
  };
  auto setup = [&](long long t) {
    if (VARIANT == 3) { setup_off(t, a_off, b_off, s_off, ld_nit); return; }
    const int b = (int)(t / tiles_per_batch);
    const int v = (int)(t - (long long)b * tiles_per_batch);
    int mt, nt; mss_tile_mn(v, p.mtiles, p.ntiles, group_m, mt, nt);
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      int row = mt * BM + row0 + j * RPP;
      row = row < p.M ? row : p.M - 1;                  // rows past the end re-read the last row; never stored
      a_ptr[j] = p.x + (size_t)b * p.x_bs + (size_t)row * p.ldx + chunk * 4;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j)
      b_ptr[j] = p.w + (size_t)b * p.w_bs + (size_t)(nt * BN + row0 + j * RPP) * p.C + chunk * 4;
    if (AFFINE) {
      // one affine per tile: per-sample affines (Dropout2d fold) are only routed here when tiles cannot straddle images
      const size_t so = (size_t)((mt * BM) / p.H) * p.in_ss_stride + chunk * 4;     // p.H = rows per image in this mode
      s_ptr = p.in_scale + so;
      h_ptr = p.in_shift + so;
    }
  };
  auto setup_next = [&]() {              // offsets of the tile the loader enters after its current one (past the end: the same)
    const long long t = ld_tile + stride;
    setup_off(t < total_tiles ? t : ld_tile, a_nxt, b_nxt, s_nxt, nit_nxt);
  };
  f32x4 areg[A_LD], breg[B_LD], sreg, hreg;
  auto issue_loads = [&]() {
    if (VARIANT == 3) {
      const char* xb = reinterpret_cast<const char*>(p.x);
      const char* wb = reinterpret_cast<const char*>(p.w);
#pragma unroll
      for (int j = 0; j < A_LD; ++j) areg[j] = *reinterpret_cast<const f32x4*>(xb + a_off[j]);
#pragma unroll
      for (int j = 0; j < B_LD; ++j) breg[j] = *reinterpret_cast<const f32x4*>(wb + b_off[j]);
      if (AFFINE) {
        sreg = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.in_scale) + s_off);
        hreg = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.in_shift) + s_off);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < A_LD; ++j) areg[j] = *reinterpret_cast<const f32x4*>(a_ptr[j]);
#pragma unroll
    for (int j = 0; j < B_LD; ++j) breg[j] = *reinterpret_cast<const f32x4*>(b_ptr[j]);
    if (AFFINE) {
      sreg = *reinterpret_cast<const f32x4*>(s_ptr);
      hreg = *reinterpret_cast<const f32x4*>(h_ptr);
    }
  };
  auto advance = [&]() {                 // next K-step of this tile, else first K-step of this workgroup's next tile
    if (VARIANT == 3) {
      const bool wrap = ++ld_k == (PERIMG ? ld_nit : n_it);
#pragma unroll
      for (int j = 0; j < A_LD; ++j) a_off[j] = wrap ? a_nxt[j] : a_off[j] + BK * (unsigned)sizeof(float);
#pragma unroll
      for (int j = 0; j < B_LD; ++j) b_off[j] = wrap ? b_nxt[j] : b_off[j] + BK * (unsigned)sizeof(float);
      if (AFFINE) s_off = wrap ? s_nxt : s_off + BK * (unsigned)sizeof(float);
      ld_k = wrap ? 0 : ld_k;
      if (PERIMG) ld_nit = wrap ? nit_nxt : ld_nit;
      return;
    }
    if (++ld_k < n_it) {
#pragma unroll
      for (int j = 0; j < A_LD; ++j) a_ptr[j] += BK;
#pragma unroll
      for (int j = 0; j < B_LD; ++j) b_ptr[j] += BK;
      if (AFFINE) { s_ptr += BK; h_ptr += BK; }
    } else {
      ld_k = 0;
      ld_tile += stride;
      setup(ld_tile < total_tiles ? ld_tile : ld_tile - stride);   // past the end: re-read the last tile, never used
    }
  };
  auto finish_store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      f32x4 val = areg[j];
      if (AFFINE) {
        val = val * sreg + hreg;
        val.x = fmaxf(val.x, relu_floor); val.y = fmaxf(val.y, relu_floor);
        val.z = fmaxf(val.z, relu_floor); val.w = fmaxf(val.w, relu_floor);
      }
      *reinterpret_cast<f32x4*>(&As[(buf * BM + row0 + j * RPP) * LDK + wchunk * 4]) = val;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j)
      *reinterpret_cast<f32x4*>(&Bs[(buf * BN + row0 + j * RPP) * LDK + wchunk * 4]) = breg[j];
  };

  const int frag_row = lane & 31, frag_h = lane >> 5;
  const int rot = frag_row >> 2;                           // tile rows are frag_row + multiples of 32: same rotation
  const float* Abase = &As[(wm * WTM + frag_row) * LDK];
  const float* Bbase = &Bs[(wn * WTN + frag_row) * LDK];
  const int koff[2] = {((frag_h + rot) & 3) * 4, ((2 + frag_h + rot) & 3) * 4};   // logical chunk kc * 2 + frag_h
  f32x4 fa[2][TM], fb[2][TN];
  auto load_frags = [&](int set, int buf, int kc) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
      fa[set][i] = *reinterpret_cast<const f32x4*>(Abase + (buf * BM + i * 32) * LDK + koff[kc]);
#pragma unroll
    for (int j = 0; j < TN; ++j)
      fb[set][j] = *reinterpret_cast<const f32x4*>(Bbase + (buf * BN + j * 32) * LDK + koff[kc]);
  };
  f32x16 acc[TM][TN];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  };
  auto mfma_chunk = [&](int set) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][s], fb[set][j][s], acc[i][j], 0, 0, 0);
  };
  auto epilogue = [&](long long t) {
    const int b = (int)(t / tiles_per_batch);
    const int v = (int)(t - (long long)b * tiles_per_batch);
    int mt, nt; mss_tile_mn(v, p.mtiles, p.ntiles, group_m, mt, nt);
    mss_epilogue_store<TM, TN>(acc, p, p.y + (size_t)b * p.y_bs, mt * BM + wm * WTM, nt * BN + wn * WTN, lane);
  };

  long long cur = ld_tile;               // tile being multiplied (the launch guarantees cur < total_tiles)
  setup(ld_tile);
  if (PERIMG) cur_nit = ld_nit;
  if (VARIANT == 3) setup_next();
  issue_loads();
  finish_store(0);
  advance();
  issue_loads(); advance();              // registers now hold K-step 1
  zero_acc();
  __syncthreads();
  load_frags(0, 0, 0);
  int buf = 0, k = 0;
  while (true) {
    load_frags(1, buf, 1);
    finish_store(buf ^ 1);             // K-step k+1, requested during step k-1
    issue_loads();                     // K-step k+2 (possibly of the next tile) into the registers just drained
    advance();
    mfma_chunk(0);
    if (VARIANT == 3) {
      // one fragment read / LDS write / global load / pair of VALU-SALU behind each of the first MFMAs of the chunk
#pragma unroll
      for (int i = 0; i < TM + TN; ++i) { __builtin_amdgcn_sched_group_barrier(0x8, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
#pragma unroll
      for (int i = 0; i < A_LD + B_LD; ++i) { __builtin_amdgcn_sched_group_barrier(0x8, 1, 0); __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); }
#pragma unroll
      for (int i = 0; i < A_LD + B_LD; ++i) { __builtin_amdgcn_sched_group_barrier(0x8, 1, 0); __builtin_amdgcn_sched_group_barrier(0x20, 1, 0); }
#pragma unroll
      for (int i = 0; i < 4 * TM * TN - (TM + TN) - 2 * (A_LD + B_LD); ++i) { __builtin_amdgcn_sched_group_barrier(0x8, 1, 0); __builtin_amdgcn_sched_group_barrier(0x6, 2, 0); }
    }
    __syncthreads();
    load_frags(0, buf ^ 1, 0);
    mfma_chunk(1);
    buf ^= 1;
    if (++k == (PERIMG ? cur_nit : n_it)) {
      epilogue(cur);
      cur += stride;
      if (cur >= total_tiles) break;
      zero_acc();
      k = 0;
      if (VARIANT == 3) {                // the loader entered tile `cur` at least one K-step ago (n_it >= 3): prepare the one after it
        ld_tile = cur;
        if (PERIMG) cur_nit = ld_nit;    // ... so ld_nit is tile `cur`'s
        setup_next();
      }
    }
  }
}

// A handful of rows (ASPP's image-pooling branch: [N, 4096] x [4096 -> 256], deepv3.py:84-88): one MFMA tile would walk the whole
// reduction alone (256 K-steps on one or two of 256 CUs: 0.25 ms for 4 MB of weights). Here a WAVE owns one output channel: its
// weight row streams through the lanes in 16-byte pieces, the <= 8 input rows come from cache, one wave reduction per row.
template <int MAXM>
__global__ __launch_bounds__(256) void gemm_few_rows_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                            float* __restrict__ y, int ldy, int M, int C, int K) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  float acc[MAXM];
#pragma unroll
  for (int m = 0; m < MAXM; ++m) acc[m] = 0.f;
  const float* wr = w + (size_t)k * C;
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + c);
#pragma unroll
    for (int m = 0; m < MAXM; ++m)
      if (m < M) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)m * ldx + c);
        acc[m] += (wv.x * xv.x + wv.y * xv.y) + (wv.z * xv.z + wv.w * xv.w);
      }
  }
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    const float s = mss_wave_sum(acc[m]);
    if (m < M && lane == 0) y[(size_t)m * ldy + k] = s;
  }
}

template <bool AFFINE, int VARIANT, int BN, bool PERIMG = false>
int launch_gemm(const MssConvArgs& p, hipStream_t stream, long long first = 0, long long end = -1) {
  const int batch = p.batch > 1 ? p.batch : 1;
  const int tiles_per_batch = p.mtiles * p.ntiles;
  if (end < 0) end = (long long)tiles_per_batch * batch;
  const long long total = end - first;                 // tiles of this launch
  if (total <= 0) return MSS_OK;
  const size_t smem = (size_t)2 * (BM + BN) * LDK * sizeof(float);
  MssKernelInfo ki;                      // resident workgroups per CU (BN = 128: 4 with 32 KB LDS and <= 128 registers)
  if (int rc = mss_kernel_info<gemm_nt_kernel<AFFINE, VARIANT, BN, PERIMG>>(NT, smem, 3, &ki)) return rc;
  // gemm_rounds.h: the residency whose last round is fuller by 2 % (r06: re-measured, 36 x 4096 x 512 -> 512 at one per CU 133.5 vs 125 TFLOP/s forced to two; the split kernel differs)
  const int grid = mss_gemm_grid(total, ki.occ, ki.cus, 0.02);
  // the square-ish tile order only for whole launches: the hybrid wide + narrow split (MSS_GEMM_TAIL) relies on tile ranges
  const int group_m = (first == 0 && end == (long long)tiles_per_batch * batch) ? MSS_ENV_INT("MSS_GEMM_GROUP_M", GEMM_GROUP_M_DEFAULT) : 0;
  hipLaunchKernelGGL((gemm_nt_kernel<AFFINE, VARIANT, BN, PERIMG>), dim3(grid), dim3(NT), smem, stream, p, first, end, tiles_per_batch, group_m);
  return mss_launch_status();
}

// The instantiation (affine, variant, bn) of the route -- one of the twelve that exist: the 128 x 64 tile and the per-image mode are
// variant 3 only, the per-image mode has no prologue (fwd_route.h never asks for another). `bn` is a parameter because a hybrid
// launches two widths.
template <int VARIANT, int BN>
int launch_gemm_affine(const MssConvArgs& p, bool affine, hipStream_t stream, long long first, long long end) {
  return affine ? launch_gemm<true, VARIANT, BN>(p, stream, first, end) : launch_gemm<false, VARIANT, BN>(p, stream, first, end);
}
int launch_gemm_as(const MssConvArgs& p, const FwdRoute& r, int bn, hipStream_t stream, long long first = 0, long long end = -1) {
  if (r.kernel == FWD_GEMM_NT_PERIMG) return bn == 256 ? launch_gemm<false, 3, 256, true>(p, stream) : launch_gemm<false, 3, 128, true>(p, stream);
  if (bn == 64) return launch_gemm_affine<3, 64>(p, r.affine, stream, first, end);
  if (r.variant == 3) return bn == 256 ? launch_gemm_affine<3, 256>(p, r.affine, stream, first, end) : launch_gemm_affine<3, 128>(p, r.affine, stream, first, end);
  return bn == 256 ? launch_gemm_affine<2, 256>(p, r.affine, stream, first, end) : launch_gemm_affine<2, 128>(p, r.affine, stream, first, end);
}

}  // namespace

// The launches of fwd_route.h's FWD_FEW_ROWS, FWD_GEMM_NT and FWD_GEMM_NT_PERIMG; p as fwd_fill_args left it.
int mss_gemm_nt_launch(MssConvArgs p, const FwdRoute& r, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (r.kernel == FWD_FEW_ROWS) {
    const dim3 grid((p.K + 3) / 4);
    if (r.BM == 8) hipLaunchKernelGGL(gemm_few_rows_kernel<8>, grid, dim3(256), 0, s, p.x, p.ldx, p.w, p.y, p.ldy, p.M, p.C, p.K);
    else if (r.BM == 16) hipLaunchKernelGGL(gemm_few_rows_kernel<16>, grid, dim3(256), 0, s, p.x, p.ldx, p.w, p.y, p.ldy, p.M, p.C, p.K);
    else hipLaunchKernelGGL(gemm_few_rows_kernel<32>, grid, dim3(256), 0, s, p.x, p.ldx, p.w, p.y, p.ldy, p.M, p.C, p.K);
    return mss_launch_status();
  }
  if (r.rounds.mode != MSS_GEMM_HYBRID) return launch_gemm_as(p, r, r.BN, s);
  // wide tiles [0, full), then narrow tiles [2 * full, 2 * tiles256): narrow tile 2w + {0, 1} is wide tile w's left / right half (gemm_rounds.h)
  const long long full = r.rounds.full, tiles256 = r.rounds.full + r.rounds.rem;
  const int rc = launch_gemm_as(p, r, 256, s, 0, full);
  if (rc) return rc;
  p.ntiles = 2 * r.ntiles;
  return launch_gemm_as(p, r, 128, s, 2 * full, 2 * tiles256);
}
