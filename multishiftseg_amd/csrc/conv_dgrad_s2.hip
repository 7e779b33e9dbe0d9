// Data gradient of a STRIDE-2 convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), gather form.
//
// The backward of the three strided bottleneck blocks of the ResNet-50 backbone (res3.0, res4.0, res5.0: conv2 3x3 / padding 1 and
// the 1x1 shortcut). Reached through mss_conv2d_forward_f32 with args->stride == -2 (include/mss_hip.h, above MssConvArgs):
//   x = dz [N, H, W, C]      the strided convolution's OUTPUT grid and output channels
//   w = the flip-packed filter [R*S][Kpad][C] of mss_conv2d_pack_weights_f32(flip = 1): tap (r', s') holds W[:, :, R-1-r', S-1-s']
//   y = dx [N, OH, OW, K]    the strided convolution's input grid, OH / OW given by the caller
//   dx[n, oy, ox, k] = sum over the taps (r', s') with (oy + pad - R + 1 + r') and (ox + pad - S + 1 + s') EVEN of
//                      dz[n, (oy + pad - R + 1 + r') / 2, (ox + pad - S + 1 + s') / 2, :] . w[(r', s')][k][:]
// Which taps have that parity depends on (oy & 1, ox & 1) alone. A tile of consecutive dx pixels would mix the four parity classes,
// so its live tap set would be the union (all of them) and 3/4 of the MFMAs of a 3x3 layer would multiply structural zeros. The
// output pixels are therefore enumerated PER PARITY CLASS: the M dimension is four pixel lists, each padded to whole tiles (their
// tiles interleaved in the grid), and every workgroup holds pixels of one class -- its live taps are block-uniform and exactly the non-zero ones:
//   3x3 / padding 1:  class (0,0) 1 tap, (0,1) and (1,0) 2 taps, (1,1) 4 taps: 9 taps over the four classes, the forward's count;
//   1x1 / padding 0:  class (0,0) 1 tap, the other three none -- those tiles skip the product and write epilogue(0).
// Every element of dx in columns [0, K) is written on every call; no atomics, a fixed summation order, bit-reproducible.
// Loader ("issue early / write late", two K-steps ahead), MFMA loop and epilogue order are conv_igemm_kernel's (conv_igemm.hip,
// mss_epilogue.h); what differs is the row enumeration, the tap geometry and an epilogue that scatters rows through a per-tile table.
#include "mss_epilogue.h"
#include "fwd_route.h"

namespace {

constexpr int DG_NT = 256;

// class index -> parity
__host__ __device__ inline int dg_py(int ci) { return ci < 2 ? 1 : 0; }
__host__ __device__ inline int dg_px(int ci) { return (ci & 1) ? 0 : 1; }
// pixels of one image with oy & 1 == py, ox & 1 == px
__host__ __device__ inline int dg_class_h(int OH, int py) { return (OH + 1 - py) >> 1; }

template <int BM, int BN, int BK, int WM, int WN, bool AFFINE>
__global__ __launch_bounds__(DG_NT) void conv_dgrad_s2_kernel(MssConvArgs p) {
  constexpr int NT = DG_NT;
  constexpr int LDK = BK + 4;            // +4 floats: ds_read_b128 of 16 distinct rows is conflict-free
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int CPR = BK / 4;            // float4 chunks per tile row
  constexpr int RPP = NT / CPR;          // rows staged per pass
  constexpr int A_LD = BM / RPP, B_LD = BN / RPP;
  static_assert(WM * WN == 4, "4 waves per workgroup");
  static_assert(A_LD >= 1 && B_LD >= 1, "tile too small for 256 threads");
  static_assert(BM % 4 == 0, "row table keeps the carve 16-byte aligned");

  extern __shared__ __attribute__((aligned(16))) float smem[];   // all LDS in ONE dynamic array, every carve a multiple of 16 B
  int* live_mask_p = reinterpret_cast<int*>(smem);  // first 16 B reserved
  float* As = smem + 4;                   // [2][BM][LDK]
  float* Bs = As + 2 * BM * LDK;          // [2][BN][LDK]
  int* orow = reinterpret_cast<int*>(Bs + 2 * BN * LDK);   // [BM]: dx row of each tile row, -1 past the end of the class

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  // ---- the tile's parity class (block-uniform). M tile index = 4 * (tile within its class) + class: neighbouring workgroups hold
  // different classes, so the store-bound tiles of a tap-less class (1x1: three of four) run beside MFMA-bound ones instead of
  // after them. The grid has 4 * max(tiles of a class) M tiles; the few past the end of a smaller class leave at once. ----
  const int v = mss_xcd_remap(blockIdx.x, gridDim.x);
  const int mtv = v / p.ntiles, nt = v % p.ntiles;
  const int n0 = nt * BN;
  const int ci = mtv & 3, mt = mtv >> 2;
  const int ch = dg_class_h(p.OH, dg_py(ci)), cw = dg_class_h(p.OW, dg_px(ci));
  const int cm = p.N * ch * cw;
  if (mt * BM >= cm) return;              // whole workgroup, before any barrier
  const int py = dg_py(ci), px = dg_px(ci);
  const int m0 = mt * BM;
  // live taps of the class: r' with (py + pad - R + 1 + r') even; its source row is cy + (py + pad - R + 1 + r') / 2
  const int ey = py + p.pad - p.R + 1, ex = px + p.pad - p.S + 1;
  int class_live = 0;
  for (int t = 0; t < p.R * p.S; ++t) {
    const int r = t / p.S, s = t - r * p.S;
    if (!((ey + r) & 1) && !((ex + s) & 1)) class_live |= 1 << t;
  }

  const int chunk = tid % CPR;
  const int row0 = tid / CPR;

  // ---- per-thread descriptors of the A rows it stages ----
  int a_nb[A_LD], a_cy[A_LD], a_cx[A_LD];
  const int chw = ch * cw;
  int my_live = 0;
  if (tid == 0) *live_mask_p = 0;
#pragma unroll
  for (int j = 0; j < A_LD; ++j) {
    const int m = m0 + row0 + j * RPP;
    if (m < cm) {
      const int n = m / chw, rem = m - n * chw;
      const int cy = rem / cw, cx = rem - cy * cw;
      a_nb[j] = n * p.H * p.W;
      a_cy[j] = cy;
      a_cx[j] = cx;
      for (int t = 0; t < p.R * p.S; ++t) {
        if (!((class_live >> t) & 1)) continue;
        const int r = t / p.S, s = t - r * p.S;
        const int iy = cy + ((ey + r) >> 1), ix = cx + ((ex + s) >> 1);
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) my_live |= 1 << t;
      }
      if (chunk == 0) orow[row0 + j * RPP] = (n * p.OH + 2 * cy + py) * p.OW + 2 * cx + px;
    } else {
      a_nb[j] = 0; a_cy[j] = -0x40000000; a_cx[j] = -0x40000000;
      if (chunk == 0) orow[row0 + j * RPP] = -1;
    }
  }
  __syncthreads();
  if (my_live) atomicOr(live_mask_p, my_live);     // LDS, an OR of bit sets: order-independent
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

  // ---- loader: one register set, two K-steps ahead (conv_igemm_kernel) ----
  f32x4 areg[A_LD], breg[B_LD], sreg, hreg;
  const float* a_ptr[A_LD];
  const float* b_ptr[B_LD];
  const float* s_ptr = p.in_scale;
  const float* h_ptr = p.in_shift;
  unsigned a_ok = 0;       // bit j: row j of this thread is inside the dz grid for the current tap
  unsigned ld_ok = 0;      // a_ok of the step whose data sits in the staging registers
  int ld_tap = -1, ld_c0 = 0, ld_left = live;
  const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();

  auto next_tap = [&]() {
    ld_tap = __ffs(ld_left) - 1;
    ld_left &= ld_left - 1;
    ld_c0 = 0;
    const int r = ld_tap / p.S, s = ld_tap - r * p.S;
    const int dy = (ey + r) >> 1, dx = (ex + s) >> 1;
    a_ok = 0;
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      const int iy = a_cy[j] + dy, ix = a_cx[j] + dx;
      const bool ok = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      a_ok |= (ok ? 1u : 0u) << j;
      a_ptr[j] = ok ? p.x + (size_t)(a_nb[j] + iy * p.W + ix) * p.ldx + chunk * 4 : p.x;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j)
      b_ptr[j] = p.w + ((size_t)ld_tap * p.Kpad + n0 + row0 + j * RPP) * p.C + chunk * 4;
    if (AFFINE) {
      s_ptr = p.in_scale + chunk * 4;
      h_ptr = p.in_shift + chunk * 4;
    }
  };

  auto issue_loads = [&]() {   // straight-line: every pointer is always a valid address
#pragma unroll
    for (int j = 0; j < A_LD; ++j) areg[j] = *reinterpret_cast<const f32x4*>(a_ptr[j]);
#pragma unroll
    for (int j = 0; j < B_LD; ++j) breg[j] = *reinterpret_cast<const f32x4*>(b_ptr[j]);
    if (AFFINE) {
      sreg = *reinterpret_cast<const f32x4*>(s_ptr);
      hreg = *reinterpret_cast<const f32x4*>(h_ptr);
    }
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
      if (AFFINE) { s_ptr += BK; h_ptr += BK; }
    }
  };

  auto finish_store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      f32x4 val = areg[j];
      if (AFFINE) val = val * sreg + hreg;
      val.x = fmaxf(val.x, relu_floor); val.y = fmaxf(val.y, relu_floor);
      val.z = fmaxf(val.z, relu_floor); val.w = fmaxf(val.w, relu_floor);
      if (!((ld_ok >> j) & 1)) val = f32x4{0.f, 0.f, 0.f, 0.f};       // the prologue touches in-grid operand rows only
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
    issue_loads();
    advance();
  }
  __syncthreads();

  // ---- main loop, software pipelined inside the wave (conv_igemm_kernel) ----
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

  // ---- epilogue: the arithmetic and order of mss_epilogue_store (affine, residual added or gating, ReLU; all residual loads of a
  // 32x32 sub-tile first, then the arithmetic, then the guarded stores), rows scattered through the tile's row table ----
  const int colq = lane & 31, rowq = 4 * (lane >> 5);
  const float floor_v = p.out_relu ? 0.f : -__builtin_huge_valf();
  const size_t ldy = (size_t)p.ldy;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * WTN + j * 32 + colq;
    if (col < p.K) {
      float osc = 1.f, osh = 0.f;
      if (p.out_scale) { osc = p.out_scale[col]; osh = p.out_shift[col]; }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const volatile int* ot = orow + wm * WTM + i * 32 + rowq;      // read per use: 16 row numbers held across the loads cost a wave/SIMD
        float rv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = 0.f;
        if (p.res) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = ot[(r & 3) + 8 * (r >> 2)];
            rv[r] = p.res[(size_t)(row < 0 ? 0 : row) * p.ldres + col];
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = ot[(r & 3) + 8 * (r >> 2)];
          const float lin = acc[i][j][r] * osc + osh;
          const float val = fmaxf(p.res_mask ? (rv[r] > 0.f ? lin : 0.f) : lin + rv[r], floor_v);
          if (row >= 0) p.y[(size_t)row * ldy + col] = val;
        }
      }
    }
  }
}

template <int BM, int BN, int BK, int WM, int WN>
int launch_dgrad_s2(MssConvArgs& p, hipStream_t stream) {
  int most = 0;                          // class (0, 0) has the most pixels; written as a maximum so the kernel's rule is the only one
  for (int c = 0; c < 4; ++c) {
    const int t = mss_cdiv((long long)p.N * dg_class_h(p.OH, dg_py(c)) * dg_class_h(p.OW, dg_px(c)), BM);
    most = t > most ? t : most;
  }
  p.mtiles = 4 * most;
  if ((long long)p.mtiles * p.ntiles > 0x7fffffffLL) return MSS_ERR_UNSUPPORTED;
  const size_t smem = ((size_t)2 * (BM + BN) * (BK + 4) + 4 + BM) * sizeof(float);
  static_assert(((size_t)2 * (BM + BN) * (BK + 4) + 4 + BM) * sizeof(float) <= 65536, "fits the default dynamic LDS limit");
  const dim3 grid(p.mtiles * p.ntiles);
  if (p.in_scale)
    hipLaunchKernelGGL((conv_dgrad_s2_kernel<BM, BN, BK, WM, WN, true>), grid, dim3(DG_NT), smem, stream, p);
  else
    hipLaunchKernelGGL((conv_dgrad_s2_kernel<BM, BN, BK, WM, WN, false>), grid, dim3(DG_NT), smem, stream, p);
  return mss_launch_status();
}

}  // namespace

// p as fwd_route.h checked it (fwd_plan_dgrad_s2: shapes, Kpad, alignment) with p.M and p.ntiles filled in; r.BN chooses the tile.
int mss_conv_dgrad_s2_launch(MssConvArgs p, const FwdRoute& r, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  return r.BN == 64 ? launch_dgrad_s2<256, 64, 16, 4, 1>(p, s) : launch_dgrad_s2<128, 128, 16, 2, 2>(p, s);
}
