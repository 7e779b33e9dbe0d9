// Job plan of gemm_tn_direct_kernel's per-image form: one text for the kernel, its tail reduce kernel and a host test.
//
// Batch entry (position, image n) holds the rows of image n alone, of which only the first 16 * (k_base + k_steps[n]) columns exist:
// L[n] = ceil(that / 128) live c tiles (clamped to ctiles). The live 128 x 128 tiles of all entries are numbered densely --
// position, then image, then k tile, c tile fastest -- so that no wave slot is spent on a tile behind an extent, and when they do not
// fill whole rounds of `slots` one-wave jobs the last, partial round (`tail` tiles) is cut into `splits` row ranges of `tps` rows each
// by wg_plan_tn_direct's rule (wgrad_route.h): the round is then 1 / splits as long. Job numbers: [0, full) whole tiles, then split-major
// full + sp * tail + tail tile. k_steps lives on the device: every wave evaluates the plan from scalar loads, the host only sizes
// the grid for the worst case (tn_perimg_worst_jobs) and the waves at or behind `total` return.
#pragma once

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define TN_PERIMG_MAX_IMGS 64            // above it the unpacked plan runs (the plan is a loop over the images in every wave)
#define TN_PERIMG_MAX_SLOTS 1024         // one wave per SIMD of 256 CUs; MSS_WGRAD_PERIMG_TAIL_BYTES (include/mss_hip.h) is sized by it

struct TnPerimgPlan {
  int ktiles, ctiles, k_imgs, k_base, rows;
  int S;                  // live tiles per position: ktiles * sum of L[n]
  long long live;         // P * S
  long long full;         // whole-tile jobs (== live without a tail)
  long long total;        // full + tail * splits
  int tail;               // tiles of the cut round (0: none)
  int splits, tps;        // row ranges per tail tile, rows per range
};

struct TnPerimgJob {
  int pos, img, kt, ct;
  int sp;                 // row range (0 for a whole tile)
  int tail_tile;          // -1: whole tile, written straight to the result
  int r0, r1;             // rows [r0, r1) of the image
};

__host__ __device__ static inline int tn_perimg_ctiles(int k_base, int k_steps_n, int ctiles) {
  const int cols = 16 * (k_base + k_steps_n);
  int L = cols > 0 ? (cols + 127) / 128 : 0;
  return L < ctiles ? L : ctiles;
}

__host__ __device__ static inline TnPerimgPlan tn_perimg_plan(int P, int k_imgs, int ktiles, int ctiles, int k_base, const int* k_steps,
                                                              int slots, int rows, int want_tail) {
  TnPerimgPlan pl;
  pl.ktiles = ktiles; pl.ctiles = ctiles; pl.k_imgs = k_imgs; pl.k_base = k_base; pl.rows = rows;
  int sum = 0;
  for (int n = 0; n < k_imgs; ++n) sum += tn_perimg_ctiles(k_base, k_steps[n], ctiles);
  pl.S = ktiles * sum;
  pl.live = (long long)P * pl.S;
  pl.full = pl.live; pl.total = pl.live; pl.tail = 0; pl.splits = 1; pl.tps = rows;
  if (!want_tail || pl.live <= slots || pl.live % slots == 0) return pl;
  const long long rounds = (pl.live + slots - 1) / slots * slots;
  if (pl.live * 20 >= rounds * 19) return pl;                     // the last round is at least 0.95 full
  const int tail = (int)(pl.live % slots);
  int ts = slots / tail;
  const int max_splits = (rows + 255) / 256;
  if (ts > max_splits) ts = max_splits;
  if (ts > 16) ts = 16;
  if (ts < 2) return pl;
  pl.tail = tail;
  pl.full = pl.live - tail;
  pl.tps = ((rows + ts - 1) / ts + 1) / 2 * 2;
  pl.splits = (rows + pl.tps - 1) / pl.tps;
  pl.total = pl.full + (long long)tail * pl.splits;               // tail * splits <= slots
  return pl;
}

// false: `job` is at or behind the plan's total (nothing to do)
__host__ __device__ static inline bool tn_perimg_decode(const TnPerimgPlan& pl, const int* k_steps, long long job, TnPerimgJob& j) {
  if (job < 0 || job >= pl.total) return false;
  long long t = job;
  j.sp = 0; j.tail_tile = -1;
  if (job >= pl.full) {
    j.sp = (int)((job - pl.full) / pl.tail);
    j.tail_tile = (int)((job - pl.full) - (long long)j.sp * pl.tail);
    t = pl.full + j.tail_tile;
  }
  j.pos = (int)(t / pl.S);
  int rem = (int)(t - (long long)j.pos * pl.S);
  j.img = 0; j.kt = 0; j.ct = 0;
  for (int n = 0; n < pl.k_imgs; ++n) {
    const int L = tn_perimg_ctiles(pl.k_base, k_steps[n], pl.ctiles);
    const int g = pl.ktiles * L;
    if (rem < g) { j.img = n; j.kt = rem / L; j.ct = rem - j.kt * L; break; }
    rem -= g;
  }
  j.r0 = j.tail_tile >= 0 ? j.sp * pl.tps : 0;
  j.r1 = j.tail_tile >= 0 && j.r0 + pl.tps < pl.rows ? j.r0 + pl.tps : pl.rows;
  return true;
}

// grid size on the host, which never reads k_steps: every column kept, plus the tail jobs of the worst case (tail * splits <= slots)
__host__ __device__ static inline long long tn_perimg_worst_jobs(int P, int k_imgs, int ktiles, int ctiles, int slots, int want_tail) {
  const long long worst = (long long)P * k_imgs * ktiles * ctiles;
  return worst + (want_tail && worst > slots ? slots : 0);
}
