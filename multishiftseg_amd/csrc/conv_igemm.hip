// Implicit-GEMM convolution on the fp32 matrix cores of MI355X (v_mfma_f32_32x32x2_f32).
//
// Replaces, for the DeepWV3Plus path, every nn.Conv2d the reference runs through cuDNN
// (reference: lib/network/deepv3/deepv3.py:47-92,217-285; wider_resnet.py:64-182,288-364).
// All 54 convs are bias-free, 1x1 or 3x3, stride 1/2, dilation 1/2/4/12/24/36, padding = dilation.
//
// GEMM view: C[m][k] = sum_{tap,c} A[m][(tap,c)] * Wp[tap][k][c]
//   m   = output pixel (n, oy, ox)   -> MFMA row i
//   k   = output channel             -> MFMA column j (lane & 31): stores are 128-B segments
//   A   = NHWC input gathered at (oy*stride - pad + r*dil, ox*stride - pad + s*dil), zero outside
// Activations are NHWC with an explicit pixel stride (ldx/ldy) so a conv can read from / write
// into a channel slice of a wider (concat) tensor without a copy.
//
// Fused on the A side (prologue): per-channel affine + ReLU, i.e. eval- or train-mode
// BatchNorm+ReLU of the *previous* layer (pre-activation blocks, wider_resnet.py:43-48,169-182);
// the affine may be per-sample so that Dropout2d's channel mask folds in too.
// Fused on the C side (epilogue): per-channel affine, residual add, ReLU.
//
// Taps that are dead for the whole 128-pixel tile (all rows fall in the zero padding, common
// for dilation 12/24/36 on /8 maps) are skipped with a block-uniform decision.
#include "mss_epilogue.h"
#include <stdlib.h>

#include "fwd_route.h"

// the launchers of the other kernel families: they take the route as decided, and test nothing themselves
int mss_gemm_nt_launch(MssConvArgs p, const FwdRoute& r, void* stream);          // gemm.hip: few rows, dense, hybrid and per-image launches
int mss_fwd_bf16x3_launch(MssConvArgs p, const FwdRoute& r, void* stream);       // gemm_bf16x3.hip: the three split-bf16 families
int mss_stem7_launch(MssConvArgs p, void* stream);                               // stem7.hip
int mss_conv_dgrad_s2_launch(MssConvArgs p, const FwdRoute& r, void* stream);    // conv_dgrad_s2.hip

namespace {

constexpr int NT = 256;

template <int BM, int BN, int BK, int WM, int WN, bool PER_SAMPLE, bool AFFINE>
__global__ __launch_bounds__(NT) void conv_igemm_kernel(MssConvArgs p) {
  constexpr int LDK = BK + 4;            // +4 floats: ds_read_b128 of 16 distinct rows is conflict-free
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int CPR = BK / 4;            // float4 chunks per tile row
  constexpr int RPP = NT / CPR;          // rows staged per pass
  constexpr int A_LD = BM / RPP, B_LD = BN / RPP;
  static_assert(WM * WN == 4, "4 waves per workgroup");
  static_assert(A_LD >= 1 && B_LD >= 1, "tile too small for 256 threads");

  // all LDS in ONE dynamic array (a static __shared__ in front would shift its 16-B alignment)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int* live_mask_p = reinterpret_cast<int*>(smem);  // first 16 B reserved
  float* As = smem + 4;                   // [2][BM][LDK]
  float* Bs = As + 2 * BM * LDK;          // [2][BN][LDK]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  // batched mode (Winograd: 16 independent GEMMs in one launch): blockIdx.y picks the operand set
  p.x += (size_t)blockIdx.y * p.x_bs;
  p.w += (size_t)blockIdx.y * p.w_bs;
  p.y += (size_t)blockIdx.y * p.y_bs;
  const int v = mss_xcd_remap(blockIdx.x, gridDim.x);
  const int mt = v / p.ntiles, nt = v % p.ntiles;
  const int m0 = mt * BM, n0 = nt * BN;

  const int chunk = tid % CPR;
  const int row0 = tid / CPR;

  // ---- per-thread descriptors of the A rows it stages ----
  int a_nb[A_LD], a_iy0[A_LD], a_ix0[A_LD], a_n[A_LD];
  const int ohw = p.OH * p.OW;
  int my_live = 0;
  if (tid == 0) *live_mask_p = 0;
#pragma unroll
  for (int j = 0; j < A_LD; ++j) {
    int m = m0 + row0 + j * RPP;
    if (m < p.M) {
      int n = m / ohw, rem = m - n * ohw;
      int oy = rem / p.OW, ox = rem - oy * p.OW;
      a_n[j] = n;
      a_nb[j] = n * p.H * p.W;
      a_iy0[j] = oy * p.stride - p.pad;
      a_ix0[j] = ox * p.stride - p.pad;
      for (int t = 0; t < p.R * p.S; ++t) {
        int iy = a_iy0[j] + (t / p.S) * p.dil, ix = a_ix0[j] + (t % p.S) * p.dil;
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) my_live |= 1 << t;
      }
    } else {
      a_n[j] = 0; a_nb[j] = 0; a_iy0[j] = -0x40000000; a_ix0[j] = -0x40000000;
    }
  }
  __syncthreads();
  if (my_live) atomicOr(live_mask_p, my_live);
  __syncthreads();
  const int live = *live_mask_p;
  const int nlive = __popc(live);
  const int cblocks = p.C / BK;
  const int n_it = nlive * cblocks;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- loader: runs one K-step ahead of the MFMA loop, split "issue early / write late":
  // issue_loads() only issues global loads (no wait, no branch: rows that fall in the zero padding
  // read a dummy valid address and are zeroed later); finish_store() runs AFTER the MFMA block of
  // the current step, applies the fused BatchNorm+ReLU prologue and writes the LDS tile. The loads'
  // latency is therefore covered by 64 MFMAs instead of stalling the wave 4x per step.
  // PER_SAMPLE: the prologue affine differs per image (Dropout2d fold) AND a tile may straddle two
  // images; then each staged row looks its affine up at LDS-write time. Otherwise one affine per
  // tile (offset by the tile's image when in_ss_stride != 0) rides along with the early loads.
  constexpr int S_LD = 1;
  f32x4 areg[A_LD], breg[B_LD], sreg[S_LD], hreg[S_LD];
  const float* a_ptr[A_LD];
  const float* b_ptr[B_LD];
  const float* s_ptr[S_LD];
  const float* h_ptr[S_LD];
  unsigned a_ok = 0;       // bit j: row j of this thread is inside the image for the current tap
  unsigned ld_ok = 0;      // a_ok of the step whose data sits in the staging registers
  int ld_cc = 0;           // its first channel (per-sample lookup at write time)
  int ld_tap = -1, ld_c0 = 0, ld_left = live;
  constexpr bool has_affine = AFFINE;
  const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();

  auto next_tap = [&]() {
    ld_tap = __ffs(ld_left) - 1;
    ld_left &= ld_left - 1;
    ld_c0 = 0;
    const int r = ld_tap / p.S, s = ld_tap - r * p.S;
    const int dy = r * p.dil, dx = s * p.dil;
    a_ok = 0;
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      const int iy = a_iy0[j] + dy, ix = a_ix0[j] + dx;
      const bool ok = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      a_ok |= (ok ? 1u : 0u) << j;
      a_ptr[j] = ok ? p.x + (size_t)(a_nb[j] + iy * p.W + ix) * p.ldx + chunk * 4 : p.x;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j)
      b_ptr[j] = p.w + ((size_t)ld_tap * p.Kpad + n0 + row0 + j * RPP) * p.C + chunk * 4;
    if (has_affine) {
#pragma unroll
      for (int j = 0; j < S_LD; ++j) {
        const size_t so = (size_t)(m0 / ohw) * p.in_ss_stride + chunk * 4;   // image of the tile's first row
        s_ptr[j] = p.in_scale + so;
        h_ptr[j] = p.in_shift + so;
      }
    }
  };

  auto issue_loads = [&]() {   // straight-line: every pointer is always a valid address
#pragma unroll
    for (int j = 0; j < A_LD; ++j) areg[j] = *reinterpret_cast<const f32x4*>(a_ptr[j]);
#pragma unroll
    for (int j = 0; j < B_LD; ++j) breg[j] = *reinterpret_cast<const f32x4*>(b_ptr[j]);
    if (has_affine) {
#pragma unroll
      for (int j = 0; j < S_LD; ++j) {
        sreg[j] = *reinterpret_cast<const f32x4*>(s_ptr[j]);
        hreg[j] = *reinterpret_cast<const f32x4*>(h_ptr[j]);
      }
    }
    ld_cc = ld_c0 + chunk * 4;
    ld_ok = a_ok;
  };
  auto advance = [&]() {       // move the loader to the next K-step (stays put after the last one)
    if (ld_c0 + BK >= p.C) {
      if (ld_left) next_tap();
    } else {
      ld_c0 += BK;
#pragma unroll
      for (int j = 0; j < A_LD; ++j)
        if ((a_ok >> j) & 1) a_ptr[j] += BK;
#pragma unroll
      for (int j = 0; j < B_LD; ++j) b_ptr[j] += BK;
      if (has_affine) {
#pragma unroll
        for (int j = 0; j < S_LD; ++j) { s_ptr[j] += BK; h_ptr[j] += BK; }
      }
    }
  };

  auto finish_store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      f32x4 val = areg[j];
      if (has_affine) {
        if (PER_SAMPLE) {
          const size_t so = (size_t)a_n[j] * p.in_ss_stride + ld_cc;
          val = val * *reinterpret_cast<const f32x4*>(p.in_scale + so) + *reinterpret_cast<const f32x4*>(p.in_shift + so);
        } else {
          val = val * sreg[0] + hreg[0];
        }
      }
      val.x = fmaxf(val.x, relu_floor); val.y = fmaxf(val.y, relu_floor);
      val.z = fmaxf(val.z, relu_floor); val.w = fmaxf(val.w, relu_floor);
      if (!((ld_ok >> j) & 1)) val = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(&As[(buf * BM + row0 + j * RPP) * LDK + chunk * 4]) = val;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j)
      *reinterpret_cast<f32x4*>(&Bs[(buf * BN + row0 + j * RPP) * LDK + chunk * 4]) = breg[j];
  };

  if (n_it > 0) {
    next_tap();
    issue_loads();
    finish_store(0);
    advance();
    issue_loads();       // the loader runs TWO K-steps ahead with one register set (see the loop): registers = step 1
    advance();
  }
  __syncthreads();

  // ---- main loop, software pipelined inside the wave -------------------------------------------
  // A K-step is NKC chunks of 8 k (= 4 MFMA k-steps x TM x TN tiles). The A/B fragments of chunk
  // kc+1 are read from LDS while chunk kc multiplies (two fragment register sets); the staging
  // registers are written to the other LDS buffer before the second-to-last chunk, the single
  // workgroup barrier sits before the last chunk, and the first fragments of the NEXT K-step are
  // read right after it -- so neither the global-load latency, nor the LDS round trip, nor the
  // barrier skew is ever exposed without MFMAs in flight.
  constexpr int NKC = BK / 8;
  const int frag_row = lane & 31, frag_k = (lane >> 5) * 4;
  const float* Abase = &As[(wm * WTM + frag_row) * LDK + frag_k];
  const float* Bbase = &Bs[(wn * WTN + frag_row) * LDK + frag_k];
  f32x4 fa[2][TM], fb[2][TN];
  auto load_frags = [&](int set, int buf, int kc) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
      fa[set][i] = *reinterpret_cast<const f32x4*>(Abase + (buf * BM + i * 32) * LDK + kc * 8);
#pragma unroll
    for (int j = 0; j < TN; ++j)
      fb[set][j] = *reinterpret_cast<const f32x4*>(Bbase + (buf * BN + j * 32) * LDK + kc * 8);
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

  if (n_it > 0) load_frags(0, 0, 0);
  for (int it = 0; it < n_it; ++it) {
    const int buf = it & 1;
    // The body is branch-free so the scheduler may interleave loads, LDS traffic, prologue math and
    // MFMAs freely: in the last step the loader re-reads its (still valid) last tile and stages it
    // into the buffer nobody reads any more.
    // The staging registers hold step it+1, requested a whole K-step ago: they go to LDS first and are re-issued at once
    // for step it+2, so no wave ever waits on a load it has just issued (gemm.hip VARIANT 2: +3-7 % on every shape).
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      if (kc + 1 < NKC) load_frags((kc + 1) & 1, buf, kc + 1);
      if (kc == NKC - 2) { finish_store(buf ^ 1); issue_loads(); advance(); }
      if (kc == NKC - 1) {
        __syncthreads();
        load_frags(NKC & 1, buf ^ 1, 0);
      }
      mfma_chunk(kc & 1);
    }
  }

  // ---- epilogue (mss_epilogue.h): affine / residual / ReLU, stores never serialised on a memory round trip ----
  mss_epilogue_store<TM, TN>(acc, p, p.y, m0 + wm * WTM, n0 + wn * WTN, lane);
}

template <int BM, int BN, int BK, int WM, int WN, bool PS, bool AFF>
int launch_conv_t(const MssConvArgs& p, hipStream_t stream) {
  const size_t smem = ((size_t)2 * (BM + BN) * (BK + 4) + 4) * sizeof(float);
  constexpr auto kern = conv_igemm_kernel<BM, BN, BK, WM, WN, PS, AFF>;
  if (int rc = mss_kernel_info<kern>(NT, smem)) return rc;         // raises the limit for the 128x128x32 tile's 73,744 bytes
  hipLaunchKernelGGL(kern, dim3(p.mtiles * p.ntiles, p.batch > 1 ? p.batch : 1), dim3(NT), smem, stream, p);
  return mss_launch_status();
}

// the route's (affine, per_sample) on one tile, then its tile: the nine instantiations of conv_igemm_kernel
template <int BM, int BN, int BK, int WM, int WN>
int launch_conv_tile(const MssConvArgs& p, const FwdRoute& r, hipStream_t stream) {
  if (!r.affine) return launch_conv_t<BM, BN, BK, WM, WN, false, false>(p, stream);
  return r.per_sample ? launch_conv_t<BM, BN, BK, WM, WN, true, true>(p, stream) : launch_conv_t<BM, BN, BK, WM, WN, false, true>(p, stream);
}
int launch_conv(const MssConvArgs& p, const FwdRoute& r, hipStream_t stream) {
  if (r.BN == 64) return launch_conv_tile<256, 64, 16, 4, 1>(p, r, stream);
  return r.BK == 32 ? launch_conv_tile<128, 128, 32, 2, 2>(p, r, stream) : launch_conv_tile<128, 128, 16, 2, 2>(p, r, stream);
}

// [K][C][R][S] (PyTorch) -> [R*S][Kpad][Cp], zero padded. flip=1 builds the dgrad weights:
// a conv from K channels back to C channels with the taps rotated 180 degrees.
// col != nullptr (flip == 0): src is n_img tensors [n][K][C][R][S] whose channels from c0 on are per-image COMPACTED columns
// (col[n][c - c0] = the column of image n that holds channel c, -1: none); dst gets, in original channel order, the sum over the
// images in ascending n -- exact zero for a channel no image holds. The weight gradients of the dropped-channel ASPP products.
__global__ void pack_weights_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int C,
                                    int R, int S, int Kpad, int Cp, int flip, const int* __restrict__ col, int n_img, int c0) {
  const size_t total = (size_t)R * S * Kpad * Cp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    int c = i % Cp;
    int k = (i / Cp) % Kpad;
    int t = i / ((size_t)Cp * Kpad);
    int r = t / S, s = t % S;
    float val = 0.f;
    if (col) {
      if (k < K && c < C)
        for (int n = 0; n < n_img; ++n) {
          const int cc = c < c0 ? c : col[(size_t)n * (C - c0) + c - c0];
          if (cc >= 0) val += src[((((size_t)n * K + k) * C + (c < c0 ? c : c0 + cc)) * R + r) * S + s];
        }
    } else if (!flip) {
      if (k < K && c < C) val = src[(((size_t)k * C + c) * R + r) * S + s];
    } else {
      // output channel index k runs over the conv's *input* channels (C of src), input index c over src's K
      if (k < C && c < K) val = src[(((size_t)c * C + k) * R + (R - 1 - r)) * S + (S - 1 - s)];
    }
    dst[i] = val;
  }
}

// [R*S][Kpad][Cp] packed gradient -> accumulate/assign into [K][C][R][S]
// place != nullptr: dst is n_img tensors [n][K][C][R][S]; image n's gets src's channels [0, c0) as they are, then channel
// c0 + place[n][p] in column c0 + p for p < 16 * k_steps[n] (place -1: zero), zeros behind -- the composed ASPP weights in the
// per-image compacted column order of the dropped-channel products.
__global__ void unpack_wgrad_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int C,
                                    int R, int S, int Kpad, int Cp, int accumulate, const int* __restrict__ place,
                                    const int* __restrict__ k_steps, int n_img, int c0) {
  if (place) {
    const size_t per = (size_t)K * C * R * S, all = per * n_img;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < all; i += (size_t)gridDim.x * blockDim.x) {
      const size_t e = i % per;
      const int n = (int)(i / per);
      const int s = e % S, r = (e / S) % R;
      const int cc = (e / ((size_t)S * R)) % C, k = e / ((size_t)S * R * C);
      int c = cc;                                           // source channel, -1: a zero column
      if (cc >= c0) {
        const int pc = cc - c0 < 16 * k_steps[n] ? place[(size_t)n * (C - c0) + cc - c0] : -1;
        c = pc >= 0 ? c0 + pc : -1;
      }
      dst[i] = c >= 0 ? src[((size_t)(r * S + s) * Kpad + k) * Cp + c] : 0.f;
    }
    return;
  }
  const size_t total = (size_t)K * C * R * S;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    int s = i % S;
    int r = (i / S) % R;
    int c = (i / ((size_t)S * R)) % C;
    int k = i / ((size_t)S * R * C);
    float val = src[((size_t)(r * S + s) * Kpad + k) * Cp + c];
    dst[i] = accumulate ? dst[i] + val : val;
  }
}

// The same two movements by lines: one workgroup owns one k and WP_CH channels. Its part of [K][C][R][S] is ONE contiguous
// run of channels * taps floats, its part of the tap-major side taps runs of `channels` floats; the run is transposed through LDS
// (tile[tap][channel]), so every global access of a wave is contiguous -- except a gathered column, which stays a 4-byte access
// (per-image compacted side: runs of `taps` floats). The flat loops above touched every 128-byte line of the [K][C][R][S] side in
// R * S far-apart passes and divided 64-bit indices per element. They keep flip = 1, one tap (the two layouts differ by the padding only:
// the flat loop is contiguous on both sides), rows of fewer than WP_MIN_C channels (the stem's 64 x 3 x 7 x 7: 16-byte runs on the
// tap-major side) and more than WP_MAX_TAPS taps.
constexpr int WP_CH = 128;
constexpr int WP_MIN_C = 32;
constexpr int WP_ILP = 4;                // elements a thread has in flight
constexpr int WP_COL_IMGS = 2;           // images whose column index a gather-sum workgroup keeps in LDS (the train step has 2)
constexpr int WP_MAX_TAPS = 121;          // 121 x (128 + 4) floats = 63 888 B of LDS

// LDS row pitch: the [K][C][R][S]-side loop walks tile[t * pitch + c] tap-fastest; pitch = 4 (mod 32) keeps 3 x 3 taps x 4 channels
// of a half-wave on 32 different banks but for 4, pitch = 1 (mod 32) does so for 32 taps and more of one channel
__host__ __device__ static inline int wp_pitch(int taps) { return WP_CH + (taps > 16 ? 1 : 4); }
static inline bool wp_by_lines(int channels, int taps) { return channels >= WP_MIN_C && taps >= 2 && taps <= WP_MAX_TAPS; }

// element j = tid + 256 * i of a run of [channels][taps]: (c, t) of the first one by one 32-bit division per thread, the following by adding
struct WpRunIndex {
  int c, t, dc, dt, taps;
  __device__ WpRunIndex(int tid, int taps_) : c(tid / taps_), t(tid % taps_), dc(256 / taps_), dt(256 % taps_), taps(taps_) {}
  __device__ void next() {
    c += dc; t += dt;
    if (t >= taps) { t -= taps; ++c; }
  }
};

// [K][C][T] -> [T][Kpad][Cp], zero padded; col: the gather-sum of pack_weights_kernel. grid = Kpad * ceil(Cp / WP_CH), 256 threads.
__global__ __launch_bounds__(256) void pack_weights_lines_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int C, int T,
                                                                  int Kpad, int Cp, const int* __restrict__ col, int n_img, int c0) {
  extern __shared__ float wp_tile[];
  const int chunks = (Cp + WP_CH - 1) / WP_CH, pitch = wp_pitch(T), tid = threadIdx.x;
  const int k = blockIdx.x / chunks, cb = (blockIdx.x - k * chunks) * WP_CH;
  const int nc_dst = Cp - cb < WP_CH ? Cp - cb : WP_CH;                       // columns of the destination rows
  const int nc_src = k < K && C > cb ? (C - cb < WP_CH ? C - cb : WP_CH) : 0;  // of them: channels that exist
  const int run = nc_src * T;
  const float* base = src + ((size_t)(k < K ? k : 0) * C + cb) * T;
  // gather-sum: the channel of image n's tensor that holds channel c (-1: none), looked up once per workgroup for the first images
  __shared__ int wp_col[WP_COL_IMGS][WP_CH];
  auto source_channel = [&](int n, int c) {
    if (c < c0) return c;
    const int cc = col[(size_t)n * (C - c0) + c - c0];
    return cc >= 0 ? c0 + cc : -1;
  };
  if (col && run > 0) {
    for (int i = tid; i < WP_COL_IMGS * WP_CH; i += 256) {
      const int n = i / WP_CH, c = i - n * WP_CH;
      wp_col[n][c] = n < n_img && c < nc_src ? source_channel(n, cb + c) : -1;
    }
    __syncthreads();
  }
  // WP_ILP elements per thread and pass: their loads are issued together, then their LDS stores (a workgroup moves only a few KB, so
  // what it waits for is the latency of its loads, not their bytes)
  WpRunIndex at(tid, T);
  for (int j0 = tid; j0 < run; j0 += WP_ILP * 256) {
    int cs[WP_ILP], ts[WP_ILP];
    float v[WP_ILP];
#pragma unroll
    for (int u = 0; u < WP_ILP; ++u) { cs[u] = at.c; ts[u] = at.t; at.next(); }
    if (!col) {
#pragma unroll
      for (int u = 0; u < WP_ILP; ++u) v[u] = j0 + u * 256 < run ? base[j0 + u * 256] : 0.f;
    } else {
      // two images' loads in flight, added in ascending n from 0.f as the flat loop adds them
#pragma unroll
      for (int u = 0; u < WP_ILP; ++u) v[u] = 0.f;
      for (int n = 0; n < n_img; n += 2) {
        float a[2][WP_ILP];
        bool has[2][WP_ILP];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int u = 0; u < WP_ILP; ++u) {
            int sc = -1;
            if (n + m < n_img && j0 + u * 256 < run) sc = n + m < WP_COL_IMGS ? wp_col[n + m][cs[u]] : source_channel(n + m, cb + cs[u]);
            has[m][u] = sc >= 0;
            a[m][u] = sc >= 0 ? src[(((size_t)(n + m) * K + k) * C + sc) * T + ts[u]] : 0.f;
          }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int u = 0; u < WP_ILP; ++u)
            if (has[m][u]) v[u] += a[m][u];
      }
    }
#pragma unroll
    for (int u = 0; u < WP_ILP; ++u)
      if (j0 + u * 256 < run) wp_tile[ts[u] * pitch + cs[u]] = v[u];
  }
  __syncthreads();
  const int c = tid & (WP_CH - 1);
  if (c < nc_dst)
    for (int t = tid / WP_CH; t < T; t += 256 / WP_CH)
      dst[((size_t)t * Kpad + k) * Cp + cb + c] = c < nc_src ? wp_tile[t * pitch + c] : 0.f;
}

// [T][Kpad][Cp] -> [K][C][T] (n_img of them with `place`, as unpack_wgrad_kernel). grid = images * K * ceil(C / WP_CH), 256 threads.
__global__ __launch_bounds__(256) void unpack_wgrad_lines_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int C, int T,
                                                                  int Kpad, int Cp, int accumulate, const int* __restrict__ place,
                                                                  const int* __restrict__ k_steps, int c0) {
  extern __shared__ float wp_tile[];
  const int chunks = (C + WP_CH - 1) / WP_CH, pitch = wp_pitch(T), tid = threadIdx.x;
  const int nk = blockIdx.x / chunks, cb = (blockIdx.x - nk * chunks) * WP_CH;
  const int n = nk / K, k = nk - n * K;
  const int nc = C - cb < WP_CH ? C - cb : WP_CH;
  const int c = tid & (WP_CH - 1);
  if (c < nc) {
    int sc = cb + c;                                       // source channel, -1: a zero column
    if (place && sc >= c0) {
      const int pc = sc - c0 < 16 * k_steps[n] ? place[(size_t)n * (C - c0) + sc - c0] : -1;
      sc = pc >= 0 ? c0 + pc : -1;
    }
    constexpr int DT = 256 / WP_CH;
    for (int t0 = tid / WP_CH; t0 < T; t0 += WP_ILP * DT) {
      float v[WP_ILP];
#pragma unroll
      for (int u = 0; u < WP_ILP; ++u) v[u] = sc >= 0 && t0 + u * DT < T ? src[((size_t)(t0 + u * DT) * Kpad + k) * Cp + sc] : 0.f;
#pragma unroll
      for (int u = 0; u < WP_ILP; ++u)
        if (t0 + u * DT < T) wp_tile[(t0 + u * DT) * pitch + c] = v[u];
    }
  }
  __syncthreads();
  float* base = dst + ((size_t)nk * C + cb) * T;
  const int run = nc * T;
  WpRunIndex at(tid, T);
  for (int j0 = tid; j0 < run; j0 += WP_ILP * 256) {
    float v[WP_ILP], before[WP_ILP];
#pragma unroll
    for (int u = 0; u < WP_ILP; ++u) {
      v[u] = j0 + u * 256 < run ? wp_tile[at.t * pitch + at.c] : 0.f;
      at.next();
    }
    if (accumulate) {
#pragma unroll
      for (int u = 0; u < WP_ILP; ++u) before[u] = j0 + u * 256 < run ? base[j0 + u * 256] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < WP_ILP; ++u)
      if (j0 + u * 256 < run) base[j0 + u * 256] = accumulate ? before[u] + v[u] : v[u];
  }
}

}  // namespace

extern "C" {

// the switches of fwd_route.h, each cached at its site (mss_common.h) until mss_env_reset()
static FwdSwitches fwd_switches() {
  FwdSwitches sw;
  sw.gemm = MSS_ENV_INT("MSS_GEMM", 1);
  sw.variant = MSS_ENV_INT("MSS_GEMM_VARIANT", 3);
  sw.tail = MSS_ENV_INT("MSS_GEMM_TAIL", -1);
  sw.split_mfma = MSS_ENV_INT("MSS_GEMM_SPLIT_MFMA", 16);
  return sw;
}

int mss_conv2d_forward_f32(MssConvArgs* args, void* stream) {
  MssConvArgs p = *args;
  const FwdRoute r = fwd_route(p, fwd_switches());
  if (r.status != MSS_OK) return r.status;
  if (r.M <= 0) return MSS_OK;
  fwd_fill_args(p, r);
  switch (r.kernel) {
    case FWD_DGRAD_S2: return mss_conv_dgrad_s2_launch(p, r, stream);
    case FWD_STEM7: return mss_stem7_launch(p, stream);
    case FWD_FEW_ROWS: case FWD_GEMM_NT: case FWD_GEMM_NT_PERIMG: return mss_gemm_nt_launch(p, r, stream);
    case FWD_GEMM_NT_BF16X3: case FWD_CONV_BF16X3: case FWD_ROWAFF_BF16X3: return mss_fwd_bf16x3_launch(p, r, stream);
    default: return launch_conv(p, r, static_cast<hipStream_t>(stream));
  }
}

// Which kernel mss_conv2d_forward_f32 runs for these arguments (include/mss_hip.h has the codes): the launch's own decision.
int mss_conv2d_forward_route(const MssConvArgs* args) { return fwd_route_code(fwd_route(*args, fwd_switches())); }

// Kpad the packed layout must use for a conv with K output channels (multiple of the N tile).
int mss_conv2d_kpad(int K) { return K <= 64 ? 64 : ((K + 127) / 128) * 128; }

int mss_conv2d_pack_weights_f32(const float* w, float* packed, int K, int C, int R, int S, int Kpad, int Cp,
                                int flip, const int* col, int n_img, int c0, void* stream) {
  if (!w || !packed) return MSS_ERR_BAD_ARG;
  if (col && (flip || n_img < 1 || c0 < 0 || c0 >= C)) return MSS_ERR_BAD_ARG;
  const long long wgs = (long long)Kpad * ((Cp + WP_CH - 1) / WP_CH);
  if (!flip && wp_by_lines(Cp, R * S) && wgs >= 1 && wgs <= 0x7fffffffll) {
    hipLaunchKernelGGL(pack_weights_lines_kernel, dim3((unsigned)wgs), dim3(256), (size_t)R * S * wp_pitch(R * S) * sizeof(float),
                       static_cast<hipStream_t>(stream), w, packed, K, C, R * S, Kpad, Cp, col, n_img, c0);
    return mss_launch_status();
  }
  const size_t total = (size_t)R * S * Kpad * Cp;
  int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                     packed, K, C, R, S, Kpad, Cp, flip, col, n_img, c0);
  return mss_launch_status();
}

int mss_conv2d_unpack_wgrad_f32(const float* packed, float* grad, int K, int C, int R, int S, int Kpad, int Cp,
                                int accumulate, const int* place, const int* k_steps, int n_img, int c0, void* stream) {
  if (!grad || !packed) return MSS_ERR_BAD_ARG;
  if (place && (accumulate || !k_steps || n_img < 1 || c0 < 0 || c0 >= C)) return MSS_ERR_BAD_ARG;
  const long long wgs = (long long)(place ? n_img : 1) * K * ((C + WP_CH - 1) / WP_CH);
  if (wp_by_lines(C, R * S) && wgs >= 1 && wgs <= 0x7fffffffll) {
    hipLaunchKernelGGL(unpack_wgrad_lines_kernel, dim3((unsigned)wgs), dim3(256), (size_t)R * S * wp_pitch(R * S) * sizeof(float),
                       static_cast<hipStream_t>(stream), packed, grad, K, C, R * S, Kpad, Cp, accumulate, place, k_steps, c0);
    return mss_launch_status();
  }
  const size_t total =(size_t)K * C * R * S * (place ? n_img : 1);
  int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(unpack_wgrad_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), packed,
                     grad, K, C, R, S, Kpad, Cp, accumulate, place, k_steps, n_img, c0);
  return mss_launch_status();
}

}  // extern "C"
