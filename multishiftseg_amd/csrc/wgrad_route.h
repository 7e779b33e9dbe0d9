// Which kernel mss_conv2d_wgrad_f32 (conv_wgrad.hip) runs for a product, with which grid, splits and scratch: ONE decision, plain
// host C++ (no HIP include, no getenv), read by the launch, by the workspace query, by the profiling label and by a stand-alone
// program (tests/wgrad_route_check.cpp). DESIGN 3.18 has the table.
#pragma once
#include <stdint.h>

#include "../../include/mss_hip.h"
#include "mss_gemm_dims.h"
#include "tn_perimg_plan.h"

// The MSS_WGRAD_* switches (conv_wgrad.hip reads them with MSS_ENV_INT once per call; these are the defaults).
struct WgradSwitches {
  // MSS_WGRAD_TN: 5 (default, r04) the LDS-free gemm_tn_direct_kernel wherever K and C are multiples of 128 and its one-wave jobs
  // fill at least 3/4 of the SIMDs -- measured against the LDS kernels (tools/bench_wgrad_tn.py): ASPP F(6x6) 64 x 2304 x 4096 -> 256
  // 116.9 -> 121.9 TFLOP/s, F(4x4) 36 x 5184 118.1 -> 123.9, decoder F(6x6) 64 x 29412 x 256 -> 256 119.9 -> 131.4, the pixel
  // decoder's Linears 162624 x 256 -> 256 / 1024 -> 256 / 256 -> 1024 107.9 / 121.5 / 121.8 -> 111.9 / 129.7 / 129.5, 1x1 65536 x
  // 4096 -> 256 123.5 -> 132.6 --; elsewhere gemm_tn2_wgrad_kernel where its 256-wide c tiles need no pixel split and fill their
  // rounds (C % 256 == 0 and at least 2 rounds of 512 slots: wg_tn_wide), else gemm_tn_wgrad_kernel. The other values force one
  // kernel onto shapes the default would not give it (tests): 0 the convolution-loader kernel (no TN route), 1 gemm_tn_wgrad_kernel,
  // 4 gemm_tn2_wgrad_kernel whenever C % 256 == 0, 7 gemm_tn_direct_kernel at any size.
  int tn = 5;
  int tn_affine = 1;                      // MSS_WGRAD_TN_AFFINE: 0 keeps products with a prologue on x off the TN route
  int tn_tail = 1;                        // MSS_WGRAD_TN_TAIL: 0 = no tail plan (whole-product and per-image form)
  int narrow = 1;                         // MSS_WGRAD_NARROW: 0 = no gemm_tn_narrow_kernel (and so no two-part route)
  int perimg_pack = 1;                    // MSS_WGRAD_PERIMG_PACK: 0 = the unpacked per-image plan
  int tn_slots = TN_PERIMG_MAX_SLOTS;     // MSS_WGRAD_TN_SLOTS: wave slots of the packed per-image plan (tests reach its tail plan)
};

// (the values are include/mss_hip.h's MSS_WG_*: mss_conv2d_wgrad_plan publishes them)
enum WgradKernel {
  WG_CONV_32 = MSS_WG_CONV_32,                        // conv_wgrad_kernel<32, 128, 16, 1>: the 19-channel heads
  WG_CONV_64 = MSS_WG_CONV_64,                        // conv_wgrad_kernel<64, 128, 16, 2>: bot_fine's 48
  WG_CONV_128 = MSS_WG_CONV_128,                      // conv_wgrad_kernel<128, 128, 16, 2>
  WG_NARROW = MSS_WG_NARROW,                          // gemm_tn_narrow_kernel (32 or 64 output rows; with or without prologue)
  WG_TN_LDS = MSS_WG_TN_LDS,                          // gemm_tn_wgrad_kernel
  WG_TN_WIDE = MSS_WG_TN_WIDE,                        // gemm_tn2_wgrad_kernel
  WG_TN_DIRECT = MSS_WG_TN_DIRECT,                    // gemm_tn_direct_kernel, whole tiles or row splits of every tile
  WG_TN_DIRECT_TAIL = MSS_WG_TN_DIRECT_TAIL,          // gemm_tn_direct_kernel with the tail plan (full >= 0) + tn_tail_reduce_kernel
  WG_TN_DIRECT_PERIMG = MSS_WG_TN_DIRECT_PERIMG,      // gemm_tn_direct_kernel<false, true>: MssConvArgs.k_steps
  WG_TN_BF16X3 = MSS_WG_TN_BF16X3,                    // the split-bf16 TN kernel (gemm_bf16x3.hip): args->route == 1
  WG_TWO_PART = MSS_WG_TWO_PART,                      // K = 128 j + r: the first wide_K channels as one product, then the last r on WG_NARROW
  WG_STEM7 = MSS_WG_STEM7,                            // stem7_wgrad_kernel (stem7_wgrad.hip): the 7x7 / stride-2 / 4 -> 64 stem, recognised in wgrad_resolve
};

struct WgradRoute {
  WgradKernel kernel = WG_CONV_128;
  int ktiles = 0, ctiles = 0;
  int positions = 1;            // independent products of the launch: filter taps, or the batch
  int splits = 1;               // row ranges
  int rows_per_split = 0;
  long long total = 0;          // jobs (workgroups or waves) the kernel's job decode assumes
  long long full = -1;          // tail plan of gemm_tn_direct_kernel: whole-tile jobs in front of the split ones; -1: none
  long long ws_bytes = 0;       // scratch this launch needs
  int wide_K = 0;               // WG_TWO_PART: channels of the first product (the parts' routes: wgrad_route on wgrad_part)
  int reduce_group = 0;         // wg_reduce_group of the launch that adds the partial slabs; 0: no such launch
};

// What the workspace query cannot know.
struct WgradFacts {
  bool dense_dy = true;         // lddy == K
  bool dy8 = true;              // dy 8-byte aligned
  bool x16 = true;              // x 16-byte aligned
  bool affine16 = true;         // in_scale / in_shift (where set) 16-byte aligned
};

// The split-bf16 TN kernel's own rule and plan stay in gemm_bf16x3.hip; the decision takes them as two callables (null: no such route).
struct WgradSplitBf16 {
  bool (*eligible)(const MssConvArgs& p, int lddy) = nullptr;
  long long (*ws_bytes)(const MssConvArgs& p, int Cp) = nullptr;
  // optional: writes the tiles, positions, splits, rows per split and job count of its plan into r (for mss_conv2d_wgrad_plan)
  void (*plan)(const MssConvArgs& p, WgradRoute& r) = nullptr;
};

static inline int wg_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Pixel splits: the smallest split count whose job count fills its last round of `slots` resident jobs to >= 95 %
// (a 1152-block grid on 768 slots runs 2 rounds for 1.5 rounds of work); more splits only add partial-slab traffic.
// Small slabs (the 19 x 256 head gradient: 2 tiles) need hundreds of splits to fill the chip.
static inline int split_search(long long base_jobs, int slots, int max_splits) {
  int splits = 1;
  double best = 0.0;
  for (int sp = 1; sp <= max_splits; ++sp) {
    const long long total = base_jobs * sp;
    const double eff = (double)total / (double)(((total + slots - 1) / slots) * slots);
    if (eff > best + 1e-9) { best = eff; splits = sp; }
    if (eff >= 0.95 && total >= slots) break;
  }
  return splits;
}

static inline int wg_positions(const MssConvArgs& p) { return p.batch > 1 ? p.batch : 1; }
static inline bool wg_has_prologue(const MssConvArgs& p) { return p.in_scale || p.in_shift || p.in_relu; }
// rows cut into `splits` ranges of a multiple of `granule` rows; ranges that would be empty are dropped
static inline void wg_cut_rows(WgradRoute& r, int M, int splits, int granule) {
  r.rows_per_split = wg_cdiv(wg_cdiv(M, splits), granule) * granule;
  r.splits = wg_cdiv(M, r.rows_per_split);
}
static inline long long wg_slab_bytes(const WgradRoute& r, const MssConvArgs& p, int Cp) {
  return r.splits > 1 ? (long long)r.splits * r.positions * p.Kpad * Cp * 4 : 0;
}
// The launch that adds `splits` partial slabs of slab4 float4s each (wgrad_reduce_kernel / wgrad_reduce_par_kernel<G>): how many
// threads share one output float4. ~64 k threads are wanted, so G split-lanes per element while each lane still has >= 4 splits
// (>= 8 G splits); 1 = the sequential kernel, one thread per float4 walking all the splits.
static inline int wg_reduce_group(long long slab4, int splits) {
  int G = 1;
  while (G < 32 && slab4 * G < 65536 && splits >= 8 * G) G *= 2;
  return G;
}
// scratch and reducer of a plan whose splits each write a whole [positions][Kpad][Cp] slab
static inline void wg_plan_slabs(WgradRoute& r, const MssConvArgs& p, int Cp) {
  r.ws_bytes = wg_slab_bytes(r, p, Cp);
  r.reduce_group = r.splits > 1 ? wg_reduce_group((long long)r.positions * p.Kpad * Cp / 4, r.splits) : 0;
}

// conv_wgrad_kernel<BKO, 128, 16>: one workgroup per (k tile x c tile, tap or batch entry, split), 768 slots =
// 3 workgroups per CU (34 KB LDS, 154 registers)
static inline WgradRoute wg_plan_conv(const MssConvArgs& p, int Cp) {
  WgradRoute r;
  r.kernel = p.K <= 32 ? WG_CONV_32 : p.K <= 64 ? WG_CONV_64 : WG_CONV_128;      // output-channel tile: 32 rows (1x4 waves) for the 19-channel heads, 64 for bot_fine's 48, else 128
  const int bko = p.K <= 32 ? 32 : p.K <= 64 ? 64 : 128, bp = 16;
  r.ktiles = wg_cdiv(p.K, bko); r.ctiles = wg_cdiv(p.C, 128); r.positions = p.batch > 1 ? p.batch : p.R * p.S;
  const int base = r.ktiles * r.ctiles * r.positions;
  int max_splits = wg_cdiv(p.M, bp * 8);
  if (max_splits > 1024) max_splits = 1024;
  if (max_splits < 1) max_splits = 1;
  wg_cut_rows(r, p.M, split_search(base, 768, max_splits), bp);
  r.total = (long long)base * r.splits;
  wg_plan_slabs(r, p, Cp);
  return r;
}

// gemm_tn_narrow_kernel
static inline bool wg_narrow_eligible(const MssConvArgs& p, int lddy, int Cp, WgradFacts f, const WgradSwitches& sw) {
  if (sw.narrow == 0) return false;
  if (p.R * p.S != 1 || p.stride != 1 || p.pad != 0 || p.batch > 1 || p.OH != p.H || p.OW != p.W) return false;
  if (p.K > 64 || (p.K > 32 && p.K % 2) || p.C % 128 || Cp != p.C || p.ldx % 4) return false;
  if ((p.in_scale || p.in_shift) && p.in_ss_stride != 0) return false;      // per-sample affines (Dropout2d folds): the LDS kernel
  if (p.M < 16384) return false;                                           // below that the launch is all ramp
  if (p.K > 32 && (lddy % 2 || !f.dy8)) return false;
  return f.x16 && ((!p.in_scale && !p.in_shift) || f.affine16);
}
static inline WgradRoute wg_plan_narrow(const MssConvArgs& p, int Cp) {
  WgradRoute r;
  r.kernel = WG_NARROW;
  r.ktiles = 1; r.ctiles = p.C / 128;
  int splits = (p.K <= 32 ? 3072 : 2048) / r.ctiles;   // one round of the resident waves: 3 per SIMD (166 registers), 2 for the 64-row tile (248)
  const int max_splits = wg_cdiv(p.M, 512);
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  wg_cut_rows(r, p.M, splits, 2);
  r.total = (long long)r.ctiles * r.splits;
  wg_plan_slabs(r, p, Cp);
  return r;
}

// The persistent LDS kernels: gemm_tn_wgrad_kernel (128-wide c tiles, 768 slots) and gemm_tn2_wgrad_kernel (256-wide, 512 slots)
static inline WgradRoute wg_plan_tn_lds(const MssConvArgs& p, int Cp, bool wide) {
  WgradRoute r;
  r.kernel = wide ? WG_TN_WIDE : WG_TN_LDS;
  r.ktiles = wg_cdiv(p.K, 128); r.ctiles = wg_cdiv(p.C, wide ? 256 : 128); r.positions = wg_positions(p);
  const long long base = (long long)r.positions * r.ktiles * r.ctiles;
  int max_splits = wg_cdiv(p.M, 16 * 8);
  // one position with few output tiles and very many rows (the decoder's Linear layers: 162 624 tokens x 256 -> 256 is 4 tiles):
  // 64 splits would fill a third of the slots
  const int cap = p.batch > 1 ? 64 : 256;
  if (max_splits > cap) max_splits = cap;
  if (max_splits < 1) max_splits = 1;
  wg_cut_rows(r, p.M, split_search(base, wide ? 512 : 768, max_splits), 16);
  r.total = base * r.splits;
  wg_plan_slabs(r, p, Cp);
  return r;
}
static inline bool wg_tn_wide(const MssConvArgs& p, int Cp, const WgradSwitches& sw) {
  if (sw.tn == 4) return p.C % 256 == 0;            // tests: the wide kernel at any size, pixel splits included
  if (sw.tn < 5 || p.C % 256) return false;
  const WgradRoute w = wg_plan_tn_lds(p, Cp, true);
  const double eff = (double)w.total / (double)(((w.total + 511) / 512) * 512);
  return w.splits == 1 && w.total >= 1024 && eff >= 0.9;
}

// plan of the LDS-free kernel: one WAVE per (position, split, 128 x 128 tile), 1024 wave slots (one per SIMD)
static inline WgradRoute wg_plan_tn_direct(const MssConvArgs& p, int Cp, const WgradSwitches& sw) {
  WgradRoute r;
  r.kernel = WG_TN_DIRECT;
  r.ktiles = p.K / 128; r.ctiles = p.C / 128; r.positions = wg_positions(p);
  const long long base = (long long)r.positions * r.ktiles * r.ctiles;
  const int slots = 1024;
  int max_splits = wg_cdiv(p.M, 256);
  // more tiles than slots, and the last round mostly empty: whole tiles for the full rounds, the rest cut so that they fill one
  // short round (the ASPP F(4x4) product: 2304 tiles = 2048 whole + 256 x 4 quarter jobs; only the 256 tail tiles are reduced)
  if (sw.tn_tail != 0 && base > slots && base % slots != 0 && (double)base / (double)(((base + slots - 1) / slots) * slots) < 0.95) {
    const long long tail = base % slots;
    int ts = (int)(slots / tail);
    if (ts > max_splits) ts = max_splits;
    if (ts > 16) ts = 16;
    if (ts >= 2) {
      r.kernel = WG_TN_DIRECT_TAIL;
      r.full = base - tail;
      wg_cut_rows(r, p.M, ts, 2);
      r.total = r.full + tail * r.splits;
      r.ws_bytes = (r.total - r.full) * (128ll * 128 * 4);
      return r;
    }
  }
  const int cap = p.batch > 1 ? 64 : 256;
  if (max_splits > cap) max_splits = cap;
  if (max_splits < 1) max_splits = 1;
  wg_cut_rows(r, p.M, split_search(base, slots, max_splits), 2);
  r.total = base * r.splits;
  wg_plan_slabs(r, p, Cp);
  return r;
}
// Whether the LDS-free kernel takes the product; `plan` is then its plan.
static inline bool wg_tn_direct(const MssConvArgs& p, int Cp, const WgradSwitches& sw, WgradRoute& plan) {
  if ((sw.tn != 5 && sw.tn != 7) || p.K % 128 || p.C % 128 || p.K > 4096) return false;
  plan = wg_plan_tn_direct(p, Cp, sw);
  if (sw.tn == 7) return true;                                  // tests: the direct kernel at any size
  // one wave per job and at least 256 rows per split: a product with few rows (the pixel decoder at ONE image: 10 164 tokens x
  // 256 -> 256 is 4 tiles x 39 splits = 156 waves for 1024 SIMDs; forward + backward 8.4 -> 9.2 ms) keeps the workgroup-tile kernels
  return plan.total * 4 >= 1024 * 3;
}
// The TN route of the batched (Winograd-domain) weight gradient and of plain 1x1 layers. `direct`: wg_tn_direct's answer
static inline bool wg_tn_eligible(const MssConvArgs& p, int lddy, WgradFacts f, const WgradSwitches& sw, bool direct) {
  if (sw.tn == 0 || p.R * p.S != 1 || p.K % 4 || p.C % 4 || p.ldx != p.C || lddy < p.K || lddy % 4) return false;
  if (!f.dense_dy && (p.batch > 1 || !direct)) return false;      // a slice of a wider dy: the LDS-free kernel takes a row stride
  if (wg_has_prologue(p)) {
    // a prologue on x: only the LDS-free kernel applies one (a single affine for all rows, 16-byte aligned vectors), one position
    if (p.batch > 1 || p.in_ss_stride != 0 || !direct || sw.tn_affine == 0) return false;
    if ((p.in_scale || p.in_shift) && !f.affine16) return false;
  }
  if (p.batch > 1) return p.x_bs % 4 == 0 && p.y_bs % 4 == 0 && p.N == 1 && p.H == 1;   // Winograd-domain products
  // a plain 1x1 / stride-1 layer over dense rows (ASPP 4096 -> 256: 95 -> see DESIGN 3.3): the same GEMM with one position;
  // narrow outputs (<= 64 channels: bot_fine, the heads) keep conv_wgrad_kernel's 64- / 32-row tiles
  return p.stride == 1 && p.pad == 0 && p.K >= 128 && p.C >= 128 && p.OH == p.H && p.OW == p.W;
}

// The arguments of one part of the two-part route (second: the narrow one). dy advances by wide_K floats and dwp by wide_K * Cp
// for the second part; lddy stays, so neither part has a dense dy.
static inline MssConvArgs wgrad_part(const MssConvArgs& p, int wide_K, bool second) {
  MssConvArgs t = p;
  if (second) { t.K = p.K - wide_K; t.Kpad = p.Kpad - wide_K; t.route = 0; }      // (the narrow kernel is a streaming kernel: nothing to split into bf16 terms)
  else t.K = t.Kpad = wide_K;
  return t;
}
// K = 128 j + r output channels with 0 < r <= 64 over many pixels (the pixel decoder's merged 288-wide projection = 256 + 32: as ONE
// product its third 128-row tile is 3/4 padding, 71 - 79 TFLOP/s): the first 128 j channels as one product on the wide kernels and
// the last r on the narrow streaming kernel, each writing its own rows of dwp. Returns the wide part's channel count, 0 = no split
// (the shape, or the pointer alignment the narrow kernel needs, known only at launch: then the unsplit product runs).
static inline int wg_wide_part(const MssConvArgs& p, int lddy, int Cp, WgradFacts f, const WgradSwitches& sw) {
  const int r = p.K % 128;
  if (p.batch > 1 || p.K <= 128 || r == 0 || r > 64 || Cp != p.C || p.Kpad < p.K) return 0;
  f.dense_dy = false;
  return wg_narrow_eligible(wgrad_part(p, p.K - r, true), lddy, Cp, f, sw) ? p.K - r : 0;
}

// The decision. p.M is set (> 0) and the arguments passed mss_conv2d_wgrad_f32's checks.
static inline WgradRoute wgrad_route(const MssConvArgs& p, int lddy, int Cp, WgradFacts f, const WgradSwitches& sw,
                                     const WgradSplitBf16& bf = WgradSplitBf16()) {
  if (p.k_steps) {
    // per-image entries over channel-compacted columns: one job per (entry, k tile, c tile) at most, no splits, no scratch needed
    // (with MSS_WGRAD_PERIMG_TAIL_BYTES of it the launch cuts the last partial round by rows: tn_perimg_plan.h)
    WgradRoute r;
    r.kernel = WG_TN_DIRECT_PERIMG;
    r.ktiles = p.K / 128; r.ctiles = p.C / 128; r.positions = p.batch;
    r.rows_per_split = p.M;
    r.total = (long long)p.batch * r.ktiles * r.ctiles;
    return r;
  }
  if (const int wide = wg_wide_part(p, lddy, Cp, f, sw)) {
    f.dense_dy = false;
    const long long wa = wgrad_route(wgrad_part(p, wide, false), lddy, Cp, f, sw, bf).ws_bytes;
    const long long wb = wgrad_route(wgrad_part(p, wide, true), lddy, Cp, f, sw, bf).ws_bytes;
    WgradRoute r;
    r.kernel = WG_TWO_PART;
    r.wide_K = wide;
    r.ws_bytes = wa > wb ? wa : wb;      // one after the other on the same scratch
    return r;
  }
  // (whole 128 x 256 tiles only: a caller that pads dwp beyond K x C keeps the native kernels, which clear the padding)
  if (bf.eligible && Cp == p.C && p.Kpad == p.K && bf.eligible(p, lddy)) {
    WgradRoute r;
    r.kernel = WG_TN_BF16X3;
    r.ws_bytes = bf.ws_bytes(p, Cp);
    if (bf.plan) {
      bf.plan(p, r);
      r.reduce_group = r.splits > 1 ? wg_reduce_group((long long)r.positions * p.Kpad * Cp / 4, r.splits) : 0;
    }
    return r;
  }
  WgradRoute d;
  const bool direct = wg_tn_direct(p, Cp, sw, d);
  if (wg_tn_eligible(p, lddy, f, sw, direct)) return direct ? d : wg_plan_tn_lds(p, Cp, wg_tn_wide(p, Cp, sw));
  if (wg_narrow_eligible(p, lddy, Cp, f, sw)) return wg_plan_narrow(p, Cp);
  return wg_plan_conv(p, Cp);
}

// Scratch that covers the launch whatever the facts turn out to be: the maximum over every combination of them (for a two-part
// route that is the larger of its parts). Winograd-domain products (batch > 1) always have a dense dy.
static inline long long wgrad_workspace_bytes(const MssConvArgs& p, int Cp, const WgradSwitches& sw,
                                              const WgradSplitBf16& bf = WgradSplitBf16()) {
  long long need = 0;
  for (int m = 0; m < 16; ++m) {
    WgradFacts f;
    f.dense_dy = !(m & 1); f.dy8 = !(m & 2); f.x16 = !(m & 4); f.affine16 = !(m & 8);
    if (!f.dense_dy && p.batch > 1) continue;
    const long long b = wgrad_route(p, f.dense_dy ? p.K : p.K + 4, Cp, f, sw, bf).ws_bytes;
    if (b > need) need = b;
  }
  return need;
}

// ---- The stem of the ResNet-50 backbone (stem7_wgrad.hip; the form is documented above mss_conv2d_wgrad_f32 in include/mss_hip.h).
// It is recognised by wgrad_resolve in front of the general checks and never reaches wgrad_route.
constexpr int WG_STEM7_TH = 4, WG_STEM7_TW = 16;      // output pixels of one tile of stem7_wgrad_kernel
constexpr int WG_STEM7_MAX_SPLITS = 1024;             // four workgroups per CU (their LDS and registers allow it); every split writes a 50 KB slab
static inline bool wg_stem7_form(const MssConvArgs& p, int Cp) {
  return p.R == 7 && p.S == 7 && p.stride == 2 && p.pad == 3 && p.dil == 1 && p.C == 4 && p.ldx == 4 && p.K == 64 && p.Kpad == 64 && Cp == 4 &&
         p.batch <= 1 && !p.in_scale && !p.in_shift && !p.in_relu && !p.k_steps;
}
static inline long long wg_stem7_tiles(const MssConvArgs& p) {
  return (long long)p.N * wg_cdiv(p.OH, WG_STEM7_TH) * wg_cdiv(p.OW, WG_STEM7_TW);
}
// One workgroup per split: a run of consecutive tiles (image, tile row, tile column), at least two, accumulated in registers into ONE
// [49][64][4] slab. rows_per_split counts the pixels of a split's tiles (tiles x 64, whatever part of them lies inside the map).
static inline WgradRoute wg_plan_stem7(const MssConvArgs& p) {
  WgradRoute r;
  r.kernel = WG_STEM7;
  r.ktiles = r.ctiles = 1; r.positions = 49;
  const long long tiles = wg_stem7_tiles(p);
  long long per = (tiles + WG_STEM7_MAX_SPLITS - 1) / WG_STEM7_MAX_SPLITS;
  if (per < 2) per = 2;
  r.splits = (int)((tiles + per - 1) / per);
  r.rows_per_split = (int)(per * WG_STEM7_TH * WG_STEM7_TW);
  r.total = r.splits;
  wg_plan_slabs(r, p, 4);
  return r;
}
// The stem form's own argument checks (p.M set, > 0). res: the stored stem output a0 of the pool form, or null.
static inline int wg_stem7_check(const MssConvArgs& p, const float* dy, int lddy) {
  if (p.H < 1 || p.W < 1 || p.OH != (p.H - 1) / 2 + 1 || p.OW != (p.W - 1) / 2 + 1) return MSS_ERR_BAD_ARG;
  if (lddy < 64 || lddy % 4) return MSS_ERR_BAD_ARG;
  if (p.res && (p.res_mask != 1 || p.ldres < 64 || p.ldres % 4)) return MSS_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(p.res)) & 15) return MSS_ERR_BAD_ARG;
  if (wg_stem7_tiles(p) >= (1ll << 31) / (WG_STEM7_TH * WG_STEM7_TW)) return MSS_ERR_UNSUPPORTED;
  return MSS_OK;
}

// ---- One call of mss_conv2d_wgrad_f32, resolved: its argument checks, the facts read off its pointers and the route(s) it launches.
// The launch and the plan query (mss_conv2d_wgrad_plan) both go through wgrad_resolve, so they cannot disagree. No pointer is
// dereferenced.
struct WgradCall {
  bool empty = false;           // no output pixels: nothing is launched (MSS_OK)
  MssConvArgs p;                // the arguments with M set
  WgradFacts f;
  WgradRoute route;             // the product as given; WG_TWO_PART: what is launched are the two parts below, with part_f
  MssConvArgs part[2];          // part[1]: dy advanced by wide_K floats, dwp by wide_K * Cp (the launch does that)
  WgradRoute part_route[2];
  WgradFacts part_f;
};

static inline bool wg_aligned_to(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

// the route a launch given ws_bytes of scratch takes: the split-bf16 kernel alone is skipped, not failed, on a scratch too small
// for it -- the native route's needs then decide
static inline WgradRoute wgrad_route_given(const MssConvArgs& p, int lddy, int Cp, WgradFacts f, const WgradSwitches& sw, const WgradSplitBf16& bf,
                                           long long ws_bytes) {
  const WgradRoute r = wgrad_route(p, lddy, Cp, f, sw, bf);
  return r.kernel == WG_TN_BF16X3 && ws_bytes < r.ws_bytes ? wgrad_route(p, lddy, Cp, f, sw) : r;
}

// Whether the tiles of a launch cover dwp [Kpad][Cp]: every kernel's epilogue writes rows < Kpad and columns < Cp INSIDE its own
// ktiles x ctiles tiles only (the padding there holds exact zeros), so padding beyond the last tile would stay unwritten.
// (The split-bf16 and per-image forms take an unpadded result only: checked where they are chosen.)
static inline bool wg_covers_padding(const WgradRoute& r, const MssConvArgs& p, int Cp) {
  if (r.kernel == WG_TN_BF16X3 || r.kernel == WG_TN_DIRECT_PERIMG) return true;
  long long rows = 128, cols = 128;
  switch (r.kernel) {
    case WG_CONV_32: rows = 32; break;
    case WG_CONV_64: rows = 64; break;
    case WG_NARROW: rows = p.K <= 32 ? 32 : 64; break;
    case WG_TN_WIDE: cols = 256; break;
    default: break;
  }
  return p.Kpad <= rows * r.ktiles && Cp <= cols * r.ctiles;
}

static inline int wgrad_resolve(const MssConvArgs* args, const float* dy, int lddy, const float* dwp, int Cp, long long ws_bytes,
                                const WgradSwitches& sw, const WgradSplitBf16& bf, WgradCall& c) {
  MssConvArgs& p = c.p;
  p = *args;
  if (!p.x || !dy || !dwp) return MSS_ERR_BAD_ARG;
  if (wg_stem7_form(p, Cp)) {      // the one form with R * S > 9; args->route is ignored (native fp32 MFMA)
    p.M = p.N * p.OH * p.OW;
    if (p.M <= 0) { c.empty = true; return MSS_OK; }
    if (const int rc = wg_stem7_check(p, dy, lddy)) return rc;
    c.route = wg_plan_stem7(p);
    return MSS_OK;
  }
  if (p.C % 4 || p.ldx % 4 || lddy % 4 || p.R * p.S > 9 || Cp % 4) return MSS_ERR_UNSUPPORTED;
  p.M = p.N * p.OH * p.OW;
  if (p.M <= 0) { c.empty = true; return MSS_OK; }
  if (p.batch > 1 && (p.R * p.S != 1 || p.batch > 65535)) return MSS_ERR_BAD_ARG;
  if (p.k_steps) {               // MssConvArgs.k_imgs: the LDS-free TN kernel is the only one that has the per-image form
    if (p.k_imgs < 1 || p.batch < 2 || p.batch % p.k_imgs || p.k_base < 0 || p.k_base * 16 > p.C || p.R * p.S != 1 || p.N != 1 || p.H != 1 ||
        p.K % 128 || p.C % 128 || p.K > 4096 || p.Kpad != p.K || Cp != p.C || p.ldx != p.C || lddy != p.K || p.x_bs % 4 || p.y_bs % 4 ||
        p.in_scale || p.in_shift || p.in_relu || p.route)
      return MSS_ERR_UNSUPPORTED;
  }
  c.f.dense_dy = lddy == p.K;
  c.f.dy8 = wg_aligned_to(dy, 8);
  c.f.x16 = wg_aligned_to(p.x, 16);
  c.f.affine16 = wg_aligned_to(p.in_scale, 16) && wg_aligned_to(p.in_shift, 16);      // (a null pointer counts as aligned)
  c.route = wgrad_route_given(p, lddy, Cp, c.f, sw, bf, ws_bytes);
  if (c.route.kernel != WG_TWO_PART) return wg_covers_padding(c.route, p, Cp) ? MSS_OK : MSS_ERR_UNSUPPORTED;
  // both parts one after the other on the same scratch, each writing its own rows of dwp
  c.part_f = c.f;
  c.part_f.dense_dy = false;
  for (int i = 0; i < 2; ++i) {
    c.part[i] = wgrad_part(p, c.route.wide_K, i == 1);
    c.part_route[i] = wgrad_route_given(c.part[i], lddy, Cp, c.part_f, sw, bf, ws_bytes);
    if (!wg_covers_padding(c.part_route[i], c.part[i], Cp)) return MSS_ERR_UNSUPPORTED;
  }
  return MSS_OK;
}
