// Which kernel mss_conv2d_forward_f32 (conv_igemm.hip) runs for a call, with which tile, loader variant and round plan: ONE decision,
// plain host C++ (no HIP include, no getenv), read by the launch, by mss_conv2d_forward_route (the profiling label) and by a
// stand-alone program (tests/fwd_route_check.cpp). DESIGN 3.26 has the table. No pointer is dereferenced: pointers are compared with
// null and their alignment is read.
#pragma once
#include <stdint.h>

#include "../../include/mss_hip.h"
#include "gemm_rounds.h"
#include "mss_gemm_dims.h"

// The MSS_GEMM* switches that take part in the decision (conv_igemm.hip reads them with MSS_ENV_INT; these are the defaults).
// MSS_GEMM_GROUP_M and MSS_GEMM_SPLIT_STATIC choose no kernel and stay with the launchers.
struct FwdSwitches {
  // MSS_GEMM: read per call (not cached): the parity tests switch routes inside one process (MSS_GEMM=0: every layer on the
  // implicit-GEMM kernel; tests/test_gpu_fullsize.py compares it with the GEMM/Winograd routes). 0 only skips the NT GEMM kernels;
  // the per-image products (k_steps) exist on them alone and keep them.
  int gemm = 1;
  // MSS_GEMM_VARIANT: measured (tools/bench_bgemm.py, tools/bench_1x1.py, r02): variant 2 is +3-7 % on every shape (C = 128: 82.7 -> 86.9,
  // 512: 127 -> 132, 1024 -> 2048: 132 -> 136 TFLOP/s; 1x1 2048 -> 4096 with prologue/residual/statistics: 123 -> 128)
  // r03: variant 3 (32-bit offsets, branch-free advance, loader instructions interleaved with the MFMAs) is +4-6 % from C = 256 up
  // (36 x 16384 x 256 -> 256: 125 -> 130, 512 -> 512: 128 -> 136, 1024 -> 2048: 133 -> 140, 1x1 2048 -> 4096: 139 -> 146 TFLOP/s) and
  // +0.5 % at C = 128, bit-identical results (tools/bench_gemm_variant.py, alternating A/B); shapes it does not take fall back to 2
  // variant 3 addresses its operands with 32-bit byte offsets and needs >= 3 K-steps per tile (see the kernel); MSS_GEMM_VARIANT=2
  // forces variant 2 everywhere (the reference of the bitwise test)
  int variant = 3;
  // MSS_GEMM_TAIL. Tile width and rounds (gemm_rounds.h, mss_gemm_rounds). 256-wide tiles when the output channels split evenly, the
  // reduction is long enough and there is work for two rounds of the 512 slots. Measured (tools/bench_bgemm.py, bench_1x1.py): 1x1 2048 -> 4096
  // 127 -> 133, ASPP 4096 -> 256 123 -> 131, 1024 -> 2048 136 -> 138, C = 304 122 -> 126 TFLOP/s; C = 256: 122 -> 121 (not taken).
  //
  // Hybrid last round (MSS_GEMM_TAIL: -1 default rules, 0 never, 1 wherever it fits): when the wide tiles leave a partial last round
  // that is at most 3/4 full, the whole rounds run on wide tiles and the remainder as twice as many narrow tiles in a second launch
  // -- narrow tile 2w + {0, 1} is wide tile w's left / right half in the same n-fastest order -- e.g. 64 x 15 x 2 = 1920
  // wide tiles (mod4 through F(6x6)): 3 wide rounds + exactly one round of 768 narrow tiles instead of 3.75 -> 4.
  // Bit-identical results. Measured: isolated 0.582 -> 0.558 ms (64 x 1892 x 512 -> 512) and 1.172 -> 1.129 ms (64 x 2112 x
  // 512 -> 1024); in the step 67.3 -> 67.1 ms of gemm_nt (the narrow round is slower per FLOP and costs a second launch): for
  // batched products it stays opt-in (MSS_GEMM_TAIL=1), 0.2 ms per step does not pay for one GEMM call becoming two kernel launches.
  // r03: a default rule for nearly-empty last rounds (rem <= 128; only one-image eval products qualify) measured +-0 on the eval
  // forward (42.15 -> 42.15 ms). The two launches use the variant-3 kernels where the shape allows.
  // r04 default rule: single-position products with at most four whole rounds, where the idle part of the last round is a
  // visible share of the launch -- the pixel decoder's Linears over 16 x 10 164 tokens are 1271 wide tiles = 2.48 rounds: decoder
  // forward + backward 66.15 -> 65.78 ms with the hybrid, bit-identical.
  // Default rule for single-position products between one and two wide rounds: one wide round, then at most one narrow
  // round, where all-narrow tiles (MSS_GEMM_TAIL=0 keeps them) walk uneven chains -- the composed ASPP head's compose and project
  // products, 7168 x 4096 -> 4096 = 896 wide tiles = 512 + 384. Still one C call and one trace row.
  int tail = -1;
  // MSS_GEMM_SPLIT_MFMA=32: the round-5 form (one product per v_mfma_f32_32x32x16_bf16) for A/B and for outputs mss_epilogue_store16 cannot take
  // The 16x16x32 form takes the products WITHOUT a prologue -- the Winograd-domain batches and the plain 1x1 layers / Linears: measured
  // 1.02-1.08x the 32x32x16 form on the 128 x 256 tile, 1.0-1.07x on the 128-wide one (profiles/r06/split_mfma_ab.md). An MFMA of that
  // shape holds the SIMD's vector issue for 8 of its 16 cycles, and the BatchNorm + ReLU prologue's ten more registers put the wide
  // kernel into scratch inside the K-loop (0.96-0.99x): the prologue, implicit-GEMM and per-sample-affine kernels stay on the round-5
  // form. MSS_GEMM_SPLIT_MFMA=32: that form everywhere (A/B, tests).
  int split_mfma = 16;
};

enum FwdKernel {
  FWD_CONV_IGEMM,         // conv_igemm_kernel<BM, BN, BK, ...> (conv_igemm.hip)
  FWD_DGRAD_S2,           // conv_dgrad_s2_kernel (conv_dgrad_s2.hip): args->stride == -2
  FWD_STEM7,              // stem7_conv_kernel (stem7.hip)
  FWD_FEW_ROWS,           // gemm_few_rows_kernel<8 / 16 / 32> (gemm.hip)
  FWD_GEMM_NT,            // gemm_nt_kernel<AFFINE, VARIANT, BN> (gemm.hip), one launch or the hybrid's two
  FWD_GEMM_NT_PERIMG,     // gemm_nt_kernel<false, 3, BN, true>: MssConvArgs.k_steps, the one-batch and the k_imgs form
  FWD_GEMM_NT_BF16X3,     // gemm_nt_bf16x3_kernel<AFFINE, BN> (gemm_bf16x3.hip): args->w_split
  FWD_CONV_BF16X3,        // gemm_nt_bf16x3_kernel<AFFINE, BN, CONV>: the implicit-GEMM layers on the split route
  FWD_ROWAFF_BF16X3,      // gemm_nt_bf16x3_kernel<true, 128, false, ROWAFF>: a per-sample affine on tiles that straddle images
  FWD_KERNELS
};

struct FwdRoute {
  int status = MSS_OK;              // MSS_ERR_BAD_ARG / MSS_ERR_UNSUPPORTED: the call is refused; only `kernel` still means something --
                                    // the kernel whose checks refused it, or that would have been asked had the general checks passed
  FwdKernel kernel = FWD_CONV_IGEMM;
  int M = 0;                        // N * OH * OW; <= 0 with status MSS_OK: nothing to launch
  int BM = 0, BN = 0, BK = 0;       // the tile: all three for conv_igemm_kernel / conv_dgrad_s2_kernel; BN 64 / 128 / 256 of the GEMM kernels
                                    // (a hybrid: of its first launch); BM = the few-rows kernel's row bucket 8 / 16 / 32
  int variant = 0;                  // gemm_nt_kernel: 2 or 3
  bool affine = false;              // the instantiation with the prologue
  bool per_sample = false;          // ... which looks its affine up per row: tiles straddle images (conv_igemm_kernel's PER_SAMPLE, ROWAFF)
  int mfma = 0;                     // the split kernels: 16 (v_mfma_f32_16x16x32_bf16) or 32
  MssGemmRounds rounds = {MSS_GEMM_NARROW, 0, 0, 0};      // FWD_GEMM_NT: the plan; the other GEMM launches: NARROW or WIDE as their BN
  int mtiles = 0, ntiles = 0;       // what the launcher puts into p.mtiles / p.ntiles (a hybrid's second launch: 2 * ntiles;
                                    // FWD_DGRAD_S2: mtiles is the kernel's own parity-class rule, set by its launcher)
  int rows_per_group = 0;           // what the launcher puts into p.H: rows that share one affine / one image's weights; 0: p.H stays
};

// p.M, p.mtiles, p.ntiles, p.H as the kernels read them
static inline void fwd_fill_args(MssConvArgs& p, const FwdRoute& r) {
  p.M = r.M; p.mtiles = r.mtiles; p.ntiles = r.ntiles;
  if (r.rows_per_group) p.H = r.rows_per_group;
}

static inline int fwd_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline bool fwd_aligned16(const void* a, const void* b = nullptr) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }
static inline FwdRoute fwd_refuse(FwdRoute r, int status) { r.status = status; return r; }

// Does an operand leave the 32-bit offsets of a kernel? `entries` blocks `stride` elements apart, the last one `extent` elements long,
// `bytes` per element (4: fp32; 6: an fp32 weight as three bf16 planes); over from `limit` bytes on: 0xffffffff for unsigned byte
// offsets, 0x7fffffff for the signed pixel offsets of the split route's implicit-GEMM loader. Whole-batch spans pass the batch and
// its stride, per-entry spans (the entries' bases are 64-bit) one entry. A negative span (negative batch strides: no caller has
// them) wraps and counts as over, except with signed_cmp -- the 128 x 64 tile's test compared signed and keeps its answer.
static inline bool fwd_span32(long long entries, long long stride, unsigned long long extent, unsigned bytes, unsigned long long limit,
                              bool signed_cmp = false) {
  const unsigned long long span = ((unsigned long long)(entries - 1) * (unsigned long long)stride + extent) * bytes;
  return signed_cmp ? (long long)span >= (long long)limit : span >= limit;
}
static inline long long fwd_batch(const MssConvArgs& p) { return p.batch > 1 ? p.batch : 1; }
// x and the fp32 weights of the whole batch within unsigned 32-bit byte offsets: what variant 3 of gemm_nt_kernel addresses with
static inline bool fwd_gemm_span32(const MssConvArgs& p, bool signed_cmp = false) {
  return fwd_span32(fwd_batch(p), p.x_bs, (unsigned long long)p.M * p.ldx, 4, 0xffffffffull, signed_cmp) ||
         fwd_span32(fwd_batch(p), p.w_bs, (unsigned long long)p.Kpad * p.C, 4, 0xffffffffull, signed_cmp);
}

// args->stride == -2: is this one of the taken shapes? (asked before anything else looks at the arguments)
static inline bool mss_conv_dgrad_s2_wanted(const MssConvArgs& p) { return p.stride == -2; }

// Exactly the shape the backbone's stem has; everything else keeps the answer mss_conv2d_forward_f32 gave before this route existed.
static inline bool mss_stem7_eligible(const MssConvArgs& p) {
  if (p.R != 7 || p.S != 7 || p.stride != 2 || p.pad != 3 || p.dil != 1) return false;
  if (p.C != 4 || p.ldx != 4 || p.K != MSS_STEM7_K || p.Kpad < MSS_STEM7_K || p.batch > 1) return false;
  if (p.in_scale || p.in_shift || p.res || p.stats || p.w_split || p.k_steps) return false;
  if (p.N < 0 || p.H <= 0 || p.W <= 0 || p.OH != (p.H - 1) / 2 + 1 || p.OW != (p.W - 1) / 2 + 1) return false;
  if (p.ldy < MSS_STEM7_K || p.ldy % 4 || !fwd_aligned16(p.y, p.x)) return false;
  if (p.out_scale && !p.out_shift) return false;
  return true;
}

// 33..64 output channels over many rows (the 48-channel heads and bot_fine, 1 M pixels) on the persistent kernel with a 128 x 64
// tile instead of conv_igemm's one-tile-per-workgroup 256 x 64 kernel: 0.203 -> 0.184 ms (256 -> 48) and 0.116 -> 0.087 ms
// (128 -> 48) at 1 x 512 x 1024
static inline bool gemm_bn64_wanted(const MssConvArgs& p) {
  // r05: from K >= 32 (33 before): 256 -> 32 over 162 k rows (the tail of the pixel decoder's
  // 288-wide projection, 31 TFLOP/s on conv_igemm's 256 x 64 tile)
  // r06: batched products too (the 48-channel tail of the 304-wide Winograd-domain data gradient of final.0: 64 x 29412 x 256 -> 48,
  // conv_igemm's one-tile-per-workgroup kernel streamed its 1.9 GB of X' at 2.6 TB/s: 2.58 -> 2.47 ms native, 1.92 -> 1.75 ms on the
  // split route for the whole 304-wide product)
  return p.K <= 64 && p.K >= 32 && p.C / MSS_GEMM_BK >= 3 && p.M >= 16384;
}

// Shapes gemm_nt_kernel takes; p.M is set.
static inline bool mss_gemm_nt_eligible(const MssConvArgs& p) {
  if (p.R * p.S != 1 || p.stride != 1 || p.pad != 0 || p.H != p.OH || p.W != p.OW) return false;
  if ((p.K <= 64 && !gemm_bn64_wanted(p)) || p.C % MSS_GEMM_BK || p.C < 2 * MSS_GEMM_BK) return false;        // narrow outputs stay on the 256x64 tile
  if (p.in_relu && !p.in_scale) return false;                      // ReLU without affine: not a shape this path sees
  if (p.in_scale && p.in_ss_stride && (p.OH * p.OW) % MSS_GEMM_BM) return false;   // per-sample affine: tiles must not straddle images
  return true;
}

// 1x1 layers over <= 32 pixels with nothing fused (the ASPP image-pooling product: one row per image -- 16 at 16 x 768 x 768, where
// the MFMA tile path took 0.255 ms): gemm_few_rows_kernel (p.M is set)
static inline bool mss_gemm_few_rows(const MssConvArgs& p) {
  return p.R * p.S == 1 && p.stride == 1 && p.pad == 0 && p.H == p.OH && p.W == p.OW && p.M > 0 && p.M <= 32 && p.batch <= 1 &&
         p.C % 4 == 0 && p.ldx % 4 == 0 && !p.in_scale && !p.in_relu && !p.out_scale && !p.out_relu && !p.res && !p.stats &&
         fwd_aligned16(p.x, p.w);
}

// Shapes the split route takes: what gemm_nt_kernel's 128- / 256-wide variant-3 kernels take (p.M set) with
// the weights' planes inside 32-bit byte offsets.
static inline bool mss_gemm_nt_bf16x3_eligible(const MssConvArgs& p) {
  if (!p.w_split || p.K <= 64 || p.C / MSS_GEMM_BK < 3 || p.Kpad % 128) return false;
  if (p.batch > 1 && p.w_bs != (long long)p.Kpad * p.C) return false;
  if (fwd_span32(1, 0, (unsigned long long)p.M * p.ldx, 4, 0xffffffffull)) return false;             // per batch entry (the entries' bases are 64-bit)
  if (fwd_span32(fwd_batch(p), (long long)p.Kpad * p.C, (unsigned long long)p.Kpad * p.C, 6, 0xffffffffull)) return false;
  return fwd_aligned16(p.w_split);
}

// 1x1 / stride-1 layers whose prologue affine is per sample while 128-row tiles straddle images ((OH * OW) % 128 != 0: mod6 / mod7's
// last convolutions at 16 x 700 x 700) -- the one GEMM shape the NT GEMM kernels leave to conv_igemm_kernel's PER_SAMPLE path
static inline bool rowaff_eligible(const MssConvArgs& p) {
  if (!p.w_split || p.R * p.S != 1 || p.stride != 1 || p.pad != 0 || p.H != p.OH || p.W != p.OW || p.batch > 1) return false;
  if (!p.in_scale || !p.in_ss_stride || (p.OH * p.OW) % MSS_GEMM_BM == 0 || p.K <= 64 || p.Kpad % 128 || p.C % MSS_GEMM_BK || p.C / MSS_GEMM_BK < 3) return false;
  if (fwd_span32(1, 0, (unsigned long long)p.M * p.ldx, 4, 0xffffffffull) || fwd_span32(1, 0, (unsigned long long)p.Kpad * p.C, 6, 0xffffffffull)) return false;
  return fwd_aligned16(p.w_split);
}

// The implicit-GEMM layers on the split route: what conv_igemm_kernel takes with > 64 output channels and ONE prologue affine
static inline bool mss_conv_bf16x3_eligible(const MssConvArgs& p) {
  if (rowaff_eligible(p)) return true;
  if (!p.w_split || p.K <= 64 || p.Kpad % 128 || p.C % MSS_GEMM_BK || p.batch > 1 || p.res_mask) return false;
  const int taps = p.R * p.S;
  if ((p.S != 1 && p.S != 3) || taps > 9 || taps * (p.C / MSS_GEMM_BK) < 3) return false;
  if (taps == 1 && p.stride == 1 && p.pad == 0) return false;                       // a plain GEMM: the NT route takes it
  if (p.in_scale && p.in_ss_stride) return false;                                   // per-sample affines (Dropout2d fold): native
  if (p.in_relu && !p.in_scale) return false;
  if (fwd_span32(1, 0, (unsigned long long)p.N * p.H * p.W * p.ldx, 4, 0x7fffffffull)) return false;   // signed 32-bit pixel offsets
  if (fwd_span32(taps, (long long)p.Kpad * p.C, (unsigned long long)p.Kpad * p.C, 6, 0xffffffffull)) return false;
  return fwd_aligned16(p.w_split);
}

// what mss_epilogue_store16's 16-byte accesses need
static inline bool split_mf16_ok(const MssConvArgs& p) {
  if (p.K % 4 || p.ldy % 4 || !fwd_aligned16(p.y) || (p.batch > 1 && p.y_bs % 4)) return false;
  if (p.res && (p.ldres % 4 || !fwd_aligned16(p.res))) return false;
  if (p.out_scale && !fwd_aligned16(p.out_scale, p.out_shift)) return false;
  return !p.stats || fwd_aligned16(p.stats);
}

// ---- the plans: `r` arrives with M set ------------------------------------------------------------------------------------------------

// stride == -2 (conv_dgrad_s2.hip): checks its own shapes, ignores w_split
static inline FwdRoute fwd_plan_dgrad_s2(const MssConvArgs& p, FwdRoute r) {
  r.kernel = FWD_DGRAD_S2;
  if (p.stats || p.batch > 1 || p.k_steps) return fwd_refuse(r, MSS_ERR_UNSUPPORTED);
  if (p.dil != 1 || p.R != p.S || !((p.R == 3 && p.pad == 1) || (p.R == 1 && p.pad == 0))) return fwd_refuse(r, MSS_ERR_UNSUPPORTED);
  if (p.C <= 0 || p.C % 16 || p.ldx % 4 || p.K <= 0) return fwd_refuse(r, MSS_ERR_UNSUPPORTED);
  if (p.in_scale && p.in_ss_stride) return fwd_refuse(r, MSS_ERR_UNSUPPORTED);                  // one prologue affine for all samples
  if (p.in_scale && !p.in_shift) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  if (p.out_scale && !p.out_shift) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  if (p.res_mask && !p.res) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  if (p.N < 0 || p.OH < 1 || p.OW < 1 || p.H < 1 || p.W < 1 || p.ldx < p.C || p.ldy < p.K || (p.res && p.ldres < p.K)) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  // the forward's floor loses a row / column, so OH and OW are the caller's; they must be a size the forward maps to H x W
  if (p.H != (p.OH + 2 * p.pad - p.R) / 2 + 1 || p.W != (p.OW + 2 * p.pad - p.S) / 2 + 1) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  if (!fwd_aligned16(p.x, p.w)) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  if (p.in_scale && !fwd_aligned16(p.in_scale, p.in_shift)) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  if ((long long)p.N * p.OH * p.OW > 0x7fffffffLL || (long long)p.N * p.H * p.W > 0x7fffffffLL) return fwd_refuse(r, MSS_ERR_UNSUPPORTED);
  r.M = p.N * p.OH * p.OW;
  if (r.M <= 0) return r;
  // the tiles of conv_igemm.hip: 256 x 64 for the <= 64-channel packs (Kpad 64), 128 x 128 x 16 otherwise
  r.BM = p.K <= 64 ? 256 : 128; r.BN = p.K <= 64 ? 64 : 128; r.BK = 16;
  r.affine = p.in_scale != nullptr;
  r.ntiles = fwd_cdiv(p.K, r.BN);
  if (p.Kpad < r.ntiles * r.BN) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  return r;
}

// the per-image product behind csrc/chan_compact.hip: image n = rows [n * OH * OW, (n + 1) * OH * OW) runs k_steps[n] K-steps
// over its own weights w + n * w_img_stride. It exists on gemm_nt_kernel only (variant 3, no prologue: the compaction pass applied
// it), so a shape that does not qualify is an error, never another route.
static inline FwdRoute fwd_plan_perimg(const MssConvArgs& p, FwdRoute r) {
  r.kernel = FWD_GEMM_NT_PERIMG;
  r.variant = 3;
  if (!mss_gemm_nt_eligible(p) || p.in_scale || p.w_split || p.K <= 64 || p.C / MSS_GEMM_BK < 3 || p.w_img_stride % 4 || p.w_img_stride < 0 ||
      p.k_base < 0 || p.k_imgs < 0)
    return fwd_refuse(r, MSS_ERR_UNSUPPORTED);
  // batch entries of one image each (the dropped-channel Winograd-domain products, k_imgs > 0): p.M rows per entry, the last row tile
  // of an entry partial; k_base + k_steps[b % k_imgs] K-steps, >= 3 since k_steps is. Otherwise whole row tiles per image.
  if (p.k_imgs > 0 ? (p.batch < 2 || p.batch % p.k_imgs || p.w_img_stride || p.N != 1 || p.k_base * MSS_GEMM_BK > p.C) : (p.batch > 1 || (p.OH * p.OW) % MSS_GEMM_BM))
    return fwd_refuse(r, MSS_ERR_UNSUPPORTED);
  r.rows_per_group = p.k_imgs > 0 ? p.M : p.OH * p.OW;        // rows per entry / per image
  r.mtiles = fwd_cdiv(p.M, MSS_GEMM_BM);
  r.ntiles = fwd_cdiv(p.K, 128);
  if (p.Kpad < r.ntiles * 128) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  const bool over = p.k_imgs > 0 ? fwd_gemm_span32(p)
                                 : fwd_span32(1, 0, (unsigned long long)p.M * p.ldx, 4, 0xffffffffull) ||
                                       fwd_span32(p.N, p.w_img_stride, (unsigned long long)p.Kpad * p.C, 4, 0xffffffffull);
  if (over) return fwd_refuse(r, MSS_ERR_UNSUPPORTED);
  // tile width: the dense products' rule on this launch's tile counts (k_imgs), or without its fill test (gemm_rounds.h)
  const bool wide = p.k_imgs > 0 ? mss_gemm_wide(r.mtiles, p.K, p.C, p.batch) : mss_gemm_wide_perimg(r.mtiles, p.K, p.C);
  r.BN = wide ? 256 : 128;
  if (wide) r.ntiles = p.K / 256;
  r.rounds.mode = wide ? MSS_GEMM_WIDE : MSS_GEMM_NARROW;
  return r;
}

// The NT GEMM kernels (gemm.hip and its split-bf16 form). False: the shape is not theirs and the next route is asked.
static inline bool fwd_plan_gemm(const MssConvArgs& p, const FwdSwitches& sw, FwdRoute& r) {
  if (!mss_gemm_nt_eligible(p)) return false;
  r.affine = p.in_scale != nullptr;
  r.rows_per_group = (p.in_scale && p.in_ss_stride) ? p.OH * p.OW : p.M;   // rows per affine group
  r.mtiles = fwd_cdiv(p.M, MSS_GEMM_BM);
  if (p.K <= 64) {                                       // the 128 x 64 tile (gemm_bn64_wanted): variant 3 only
    r.kernel = FWD_GEMM_NT; r.BN = 64; r.variant = 3; r.ntiles = 1;
    if (p.Kpad < 64) { r.status = MSS_ERR_BAD_ARG; return true; }
    if (fwd_gemm_span32(p, true)) { r = FwdRoute(); r.M = p.M; return false; }      // beyond 32-bit offsets: conv_igemm_kernel
    return true;
  }
  r.ntiles = fwd_cdiv(p.K, 128);
  r.kernel = mss_gemm_nt_bf16x3_eligible(p) ? FWD_GEMM_NT_BF16X3 : FWD_GEMM_NT;      // the split-bf16 route is chosen by the caller (args->w_split)
  if (p.Kpad < r.ntiles * 128) { r.status = MSS_ERR_BAD_ARG; return true; }
  if (r.kernel == FWD_GEMM_NT_BF16X3) {
    r.mfma = (!r.affine && sw.split_mfma != 32 && split_mf16_ok(p)) ? 16 : 32;
    r.rounds.mode = mss_gemm_wide(r.mtiles, p.K, p.C, p.batch) ? MSS_GEMM_WIDE : MSS_GEMM_NARROW;     // the native route's width, one launch
  } else {
    r.variant = (sw.variant == 3 && p.C / MSS_GEMM_BK >= 3 && !fwd_gemm_span32(p)) ? 3 : 2;
    r.rounds = mss_gemm_rounds(r.mtiles, p.K, p.C, p.batch, sw.tail);
  }
  r.BN = r.rounds.mode != MSS_GEMM_NARROW ? 256 : 128;
  if (r.BN == 256) r.ntiles = p.K / 256;
  return true;
}

static inline FwdRoute fwd_plan_conv_bf16x3(const MssConvArgs& p, FwdRoute r) {
  r.affine = p.in_scale != nullptr;
  r.mfma = 32;
  r.mtiles = fwd_cdiv(p.M, MSS_GEMM_BM);
  r.ntiles = fwd_cdiv(p.K, 128);
  r.BN = 128;
  if (rowaff_eligible(p)) {
    r.kernel = FWD_ROWAFF_BF16X3;
    r.per_sample = true;
    r.rows_per_group = p.OH * p.OW;                      // rows per image
    return r;
  }
  r.kernel = FWD_CONV_BF16X3;                            // p.H stays the image's height
  if (mss_gemm_wide_split_conv(r.mtiles, p.K)) { r.BN = 256; r.ntiles = p.K / 256; r.rounds.mode = MSS_GEMM_WIDE; }
  return r;
}

static inline FwdRoute fwd_plan_igemm(const MssConvArgs& p, FwdRoute r) {
  r.kernel = FWD_CONV_IGEMM;
  // K-step: 16 (41 KB LDS, 144 registers -> 3 workgroups/CU, 3 waves/SIMD) is the faster choice except
  // for the ASPP shape (4096 input channels, 256 output channels), where the 32-deep step wins
  // (measured: 128 vs 119 TFLOP/s).
  if (p.K <= 64) { r.BM = 256; r.BN = 64; r.BK = 16; }
  else { r.BM = r.BN = 128; r.BK = (p.C % 32 == 0 && p.C >= 2048 && p.K <= 256) ? 32 : 16; }
  r.affine = p.in_scale != nullptr;
  // a tile can only straddle two images when the image's pixel count is not a multiple of BM
  r.per_sample = r.affine && p.in_ss_stride && (p.OH * p.OW) % r.BM != 0;
  r.mtiles = fwd_cdiv(p.M, r.BM);
  r.ntiles = fwd_cdiv(p.K, r.BN);
  if (p.Kpad < r.ntiles * r.BN) return fwd_refuse(r, MSS_ERR_BAD_ARG);
  return r;
}

// The order of the routes; x, w and y are set (fwd_route looks).
static inline FwdRoute fwd_route_checked(MssConvArgs p, const FwdSwitches& sw) {
  FwdRoute r;
  if (mss_conv_dgrad_s2_wanted(p)) return fwd_plan_dgrad_s2(p, r);
  if (mss_stem7_eligible(p)) {                           // the one shape with C == 4 and 49 taps
    r.kernel = FWD_STEM7;
    r.M = p.N * p.OH * p.OW;                             // (N == 0: nothing to launch)
    r.BN = MSS_STEM7_K; r.ntiles = 1;
    return r;
  }
  // what every other kernel needs; a call refused here still learns its kernel below
  int general = MSS_OK;
  if (p.C % 16 || p.ldx % 4 || p.R * p.S > 9 || p.R * p.S < 1) general = MSS_ERR_UNSUPPORTED;
  else if (!fwd_aligned16(p.x, p.w)) general = MSS_ERR_BAD_ARG;
  else if (p.in_scale && !fwd_aligned16(p.in_scale, p.in_shift)) general = MSS_ERR_BAD_ARG;
  else if (p.batch > 1 && (p.res || p.stats || p.x_bs % 4 || p.w_bs % 4 || p.batch > 65535)) general = MSS_ERR_BAD_ARG;
  else if (p.res_mask && !p.res) general = MSS_ERR_BAD_ARG;
  p.M = r.M = p.N * p.OH * p.OW;
  if (p.M <= 0) return fwd_refuse(r, general);
  if (mss_gemm_few_rows(p) && (sw.gemm || p.k_steps)) {
    r.kernel = FWD_FEW_ROWS;
    r.BM = p.M <= 8 ? 8 : p.M <= 16 ? 16 : 32;
  }
  else if (p.k_steps) r = fwd_plan_perimg(p, r);         // per-image reduction lengths: gemm_nt_kernel is the only kernel that has them
  else if (sw.gemm && fwd_plan_gemm(p, sw, r)) {}
  else if (mss_conv_bf16x3_eligible(p)) r = fwd_plan_conv_bf16x3(p, r);     // the split-bf16 route (args->w_split), implicit-GEMM form
  else r = fwd_plan_igemm(p, r);
  return general != MSS_OK ? fwd_refuse(r, general) : r;
}

// The decision: the only text that knows the order of the routes.
static inline FwdRoute fwd_route(const MssConvArgs& args, const FwdSwitches& sw) {
  MssConvArgs p = args;
  // the checks that hold for every kernel: the first one that fails is the call's status, and the decision goes on to name the kernel
  // (mss_conv2d_forward_route labels calls whose output pointer is not set yet)
  const int general = (!p.x || !p.w || !p.y) ? MSS_ERR_BAD_ARG : MSS_OK;
  FwdRoute r = fwd_route_checked(p, sw);
  if (general != MSS_OK) r.status = general;
  return r;
}

// The answer of mss_conv2d_forward_route (include/mss_hip.h); a refused call: the code of r.kernel all the same
static inline int fwd_route_code(const FwdRoute& r) {
  static const int code[FWD_KERNELS] = {0, 6, 5, 2, 1, 1, 3, 4, 4};
  return code[r.kernel];
}
