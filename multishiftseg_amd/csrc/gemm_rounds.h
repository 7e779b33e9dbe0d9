// Round arithmetic of gemm_nt_kernel's dense launches (gemm.hip; fwd_route.h asks it): one text for the launch rule and a host test
// (tests/gemm_rounds_check.cpp).
//
// A product of mtiles row tiles (128 rows) and K output channels runs on 128 x 128 ("narrow", K / 128 column tiles, up to 3 workgroups
// per CU = 768 slots) or on 128 x 256 tiles ("wide", K / 256 column tiles, 2 per CU = 512 slots). Tiles are numbered n-fastest, so
// narrow tiles 2w and 2w + 1 are the left and right half of wide tile w: a launch may run wide tiles [0, full) and finish on narrow
// tiles [2 * full, 2 * tiles256) -- the hybrid -- and still write every output element once, by the same sum in the same order.
#pragma once

enum { MSS_GEMM_NARROW = 0, MSS_GEMM_WIDE = 1, MSS_GEMM_HYBRID = 2 };

#define MSS_GEMM_WIDE_SLOTS 512
#define MSS_GEMM_NARROW_SLOTS 768
#define MSS_GEMM_TAIL_MAX 384            // wide tiles a hybrid's narrow launch may stand for: 768 narrow tiles, one round

struct MssGemmRounds {
  int mode;
  long long tiles256;                    // wide tiles of the whole product (0: K is no multiple of 256)
  long long full, rem;                   // hybrid: wide tiles [0, full), then narrow tiles [2 * full, 2 * (full + rem)); else 0
};

// share of the slots of all rounds that hold a tile
static inline double mss_gemm_round_fill(long long total, long long slots) {
  const long long rounds = (total + slots - 1) / slots;
  return (double)total / (double)(rounds * slots);
}

// tail_mode = MSS_GEMM_TAIL: -1 the default rules, 0 no hybrid anywhere, 1 a hybrid wherever the last wide round is at most 3/4 full
static inline MssGemmRounds mss_gemm_rounds(int mtiles, int K, int C, int batch, int tail_mode) {
  MssGemmRounds r = {MSS_GEMM_NARROW, 0, 0, 0};
  if (K <= 0 || K % 256 || C < 256) return r;
  const long long tiles256 = (long long)mtiles * (K / 256) * (batch > 1 ? batch : 1);
  r.tiles256 = tiles256;
  // 256-wide tiles when there is work for two rounds of the 512 slots ...
  bool wide = tiles256 >= 2 * MSS_GEMM_WIDE_SLOTS;
  // ... unless the last round of wide tiles is mostly idle while the narrow tiles fill theirs: 64 x 18 x 1 wide tiles (ASPP
  // dilation 12 / 24 through F(6x6): 2304 tiles x 4096 -> 256) are 2.25 rounds of the 512 slots but exactly 3 rounds of the
  // 768 narrow slots -- measured 119.5 (wide) against 133.4 TFLOP/s (narrow)
  if (wide) {
    const double ew = mss_gemm_round_fill(tiles256, MSS_GEMM_WIDE_SLOTS), en = mss_gemm_round_fill(2 * tiles256, MSS_GEMM_NARROW_SLOTS);
    if (ew < 0.8 && en > ew + 0.15) wide = false;
  }
  const long long full = (tiles256 / MSS_GEMM_WIDE_SLOTS) * MSS_GEMM_WIDE_SLOTS, rem = tiles256 - full;
  if (wide) {
    // the last wide round at most 3/4 full: always with MSS_GEMM_TAIL=1; by default for single-position products of at most four
    // whole rounds, where the idle part of the last round is a visible share of the launch (fwd_route.h, FwdSwitches::tail, has the measurements)
    const long long rem_max = tail_mode == 1 ? MSS_GEMM_TAIL_MAX : (tail_mode == -1 && batch <= 1 && full <= 4 * MSS_GEMM_WIDE_SLOTS) ? MSS_GEMM_TAIL_MAX : 0;
    r.mode = MSS_GEMM_WIDE;
    if (full > 0 && rem > 0 && rem <= rem_max) { r.mode = MSS_GEMM_HYBRID; r.full = full; r.rem = rem; }
    return r;
  }
  // between one and two wide rounds (single-position products): all narrow, such a product is 2.0 ... 2.7 rounds of 768 slots and
  // its workgroups walk uneven tile chains; one whole wide round and at most one narrow round fill every slot once. The composed
  // ASPP head's two weight-sized products (56 x 16 = 896 wide tiles = 512 + 384) are exactly that. MSS_GEMM_TAIL=0: all narrow.
  if (tail_mode != 0 && batch <= 1 && tiles256 > MSS_GEMM_WIDE_SLOTS && tiles256 < 2 * MSS_GEMM_WIDE_SLOTS && rem <= MSS_GEMM_TAIL_MAX) {
    r.mode = MSS_GEMM_HYBRID; r.full = full; r.rem = rem;
  }
  return r;
}

// The width rule alone (no hybrid): what the launches without a second kernel ask -- the k_imgs form of the per-image products and
// the split-bf16 GEMM route (fwd_route.h).
static inline bool mss_gemm_wide(int mtiles, int K, int C, int batch) { return mss_gemm_rounds(mtiles, K, C, batch, 0).mode == MSS_GEMM_WIDE; }

// Two launches keep a rule of their own (unifying them would change which kernel their products get, and nothing is measured for that):
// the one-batch per-image products (MssConvArgs.k_steps, k_imgs == 0) take the rule above WITHOUT its last-round fill test: the
// per-image step counts make the rounds uneven anyway
static inline bool mss_gemm_wide_perimg(int mtiles, int K, int C) { return K % 256 == 0 && (long long)mtiles * (K / 256) >= 2 * MSS_GEMM_WIDE_SLOTS && C >= 256; }
// the implicit-GEMM layers of the split-bf16 route take the tile count ALONE, neither the fill test nor C >= 256: their reduction
// is taps * C long (16 input channels of a 3x3 layer are 9 K-steps per tile), and the fill test was measured on the GEMM products only
static inline bool mss_gemm_wide_split_conv(int mtiles, int K) { return K % 256 == 0 && (long long)mtiles * (K / 256) >= 2 * MSS_GEMM_WIDE_SLOTS; }

// Workgroups of a launch of `total` tiles: every workgroup walks ceil(total / grid) tiles, so of the residencies per_cu_max and one
// less the one whose last round is fuller by more than `margin` (the caller's measurement), e.g. 4608 tiles = 6 full rounds of 768 but 4.5 of 1024.
static inline int mss_gemm_grid(long long total, int per_cu_max, int cus, double margin) {
  int grid = 0;
  double best = -1.0;
  for (int per_cu = per_cu_max; per_cu >= (per_cu_max > 1 ? per_cu_max - 1 : 1); --per_cu) {
    const long long slots = (long long)per_cu * cus;
    const long long g = total < slots ? total : slots;
    const double eff = mss_gemm_round_fill(total, g);
    if (eff > best + margin) { best = eff; grid = (int)g; }
  }
  return grid;
}
