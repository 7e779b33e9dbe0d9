// Stand-alone host check of csrc/tn_perimg_plan.h (tests/test_tn_perimg_plan_cpu.py compiles and runs it, with the host compiler's
// address and undefined-behaviour sanitizers). One case per line of stdin:
//   P k_imgs ktiles ctiles k_base slots rows want_tail k_steps[0] ... k_steps[k_imgs - 1]
// For every case every job number of the worst-case grid (and a margin behind it) is decoded. Prints one line per case:
//   plan S live full tail splits tps total worst
// and exits non-zero with a message at the first violated property.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "tn_perimg_plan.h"

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::fprintf(stderr, "case %d: %s: ", line, #cond);  \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      return 1;                                            \
    }                                                      \
  } while (0)

int main() {
  int line = 0;
  int P, k_imgs, ktiles, ctiles, k_base, slots, rows, want_tail;
  while (std::scanf("%d %d %d %d %d %d %d %d", &P, &k_imgs, &ktiles, &ctiles, &k_base, &slots, &rows, &want_tail) == 8) {
    ++line;
    std::vector<int> ks(k_imgs);                           // exactly k_imgs ints: a read behind them is a sanitizer report
    for (int n = 0; n < k_imgs; ++n)
      if (std::scanf("%d", &ks[n]) != 1) return 2;
    const TnPerimgPlan pl = tn_perimg_plan(P, k_imgs, ktiles, ctiles, k_base, ks.data(), slots, rows, want_tail);
    const long long worst = tn_perimg_worst_jobs(P, k_imgs, ktiles, ctiles, slots, want_tail);
    std::vector<int> L(k_imgs);
    long long sum = 0;
    for (int n = 0; n < k_imgs; ++n) {
      L[n] = tn_perimg_ctiles(k_base, ks[n], ctiles);
      CHECK(L[n] >= 0 && L[n] <= ctiles && (L[n] == ctiles || L[n] * 128 >= 16 * (k_base + ks[n])), "L[%d] = %d", n, L[n]);
      CHECK(L[n] == 0 || (L[n] - 1) * 128 < 16 * (k_base + ks[n]), "L[%d] = %d has an empty tile", n, L[n]);
      sum += L[n];
    }
    CHECK(pl.S == ktiles * sum && pl.live == (long long)P * pl.S, "S %d live %lld", pl.S, pl.live);
    CHECK(pl.total <= worst, "total %lld above the worst-case grid %lld", pl.total, worst);
    CHECK(pl.full + (long long)pl.tail * pl.splits == pl.total && pl.full + pl.tail == pl.live, "full %lld tail %d", pl.full, pl.tail);
    if (pl.tail) {
      CHECK(want_tail && pl.full > 0 && pl.full % slots == 0 && pl.splits >= 2 && pl.splits <= 16, "full %lld splits %d", pl.full, pl.splits);
      CHECK((long long)pl.tail * pl.splits <= slots, "tail %d x splits %d above %d slots", pl.tail, pl.splits, slots);
      CHECK(pl.tps % 2 == 0 && (long long)pl.tps * pl.splits >= rows && (long long)pl.tps * (pl.splits - 1) < rows, "tps %d", pl.tps);
    } else {
      CHECK(pl.splits == 1 && pl.tps == rows, "splits %d tps %d without a tail", pl.splits, pl.tps);
    }
    typedef std::tuple<int, int, int, int> Key;
    std::map<Key, int> whole;
    std::map<Key, std::vector<std::pair<int, int>>> parts;       // per split: its row range
    TnPerimgJob prev{};
    bool have_prev = false;
    for (long long job = 0; job < worst + 2 * slots + 7; ++job) {
      TnPerimgJob j;
      const bool ok = tn_perimg_decode(pl, ks.data(), job, j);
      CHECK(ok == (job < pl.total), "job %lld of %lld", job, pl.total);
      if (!ok) continue;
      CHECK(j.pos >= 0 && j.pos < P && j.img >= 0 && j.img < k_imgs && j.kt >= 0 && j.kt < ktiles && j.ct >= 0 && j.ct < L[j.img],
            "job %lld -> (%d, %d, %d, %d)", job, j.pos, j.img, j.kt, j.ct);
      const Key key(j.pos, j.img, j.kt, j.ct);
      if (j.tail_tile < 0) {
        CHECK(job < pl.full && j.sp == 0 && j.r0 == 0 && j.r1 == rows, "whole job %lld rows [%d, %d)", job, j.r0, j.r1);
        CHECK(++whole[key] == 1, "job %lld: tile covered twice", job);
        // c tile fastest: the next job of the same (position, image, k tile) is the next c tile
        if (have_prev && prev.pos == j.pos && prev.img == j.img && prev.kt == j.kt) CHECK(j.ct == prev.ct + 1, "job %lld: c tile order", job);
        else CHECK(j.ct == 0 || job == 0, "job %lld: a group starts at c tile %d", job, j.ct);
        prev = j; have_prev = true;
      } else {
        CHECK(job >= pl.full && j.tail_tile < pl.tail && j.sp >= 0 && j.sp < pl.splits, "tail job %lld", job);
        CHECK(job == pl.full + (long long)j.sp * pl.tail + j.tail_tile, "tail job %lld: split-major numbering", job);
        CHECK(j.r0 == j.sp * pl.tps && j.r0 < j.r1 && j.r1 <= rows, "tail job %lld rows [%d, %d)", job, j.r0, j.r1);
        std::vector<std::pair<int, int>>& v = parts[key];
        if (v.empty()) v.assign(pl.splits, std::make_pair(-1, -1));
        CHECK(v[j.sp].first < 0, "tail job %lld: split %d of its tile twice", job, j.sp);
        v[j.sp] = std::make_pair(j.r0, j.r1);
      }
    }
    // every live tile once as a whole or once per split, never both; nothing else
    long long covered = 0;
    for (int pos = 0; pos < P; ++pos)
      for (int n = 0; n < k_imgs; ++n)
        for (int kt = 0; kt < ktiles; ++kt)
          for (int ct = 0; ct < L[n]; ++ct) {
            const Key key(pos, n, kt, ct);
            const bool w = whole.count(key) != 0, t = parts.count(key) != 0;
            CHECK(w != t, "tile (%d, %d, %d, %d): whole %d, split %d", pos, n, kt, ct, (int)w, (int)t);
            if (t) {
              int at = 0;
              for (const std::pair<int, int>& r : parts[key]) {
                CHECK(r.first == at, "tile (%d, %d, %d, %d): row ranges do not partition", pos, n, kt, ct);
                at = r.second;
              }
              CHECK(at == rows, "tile (%d, %d, %d, %d): rows end at %d", pos, n, kt, ct, at);
            }
            ++covered;
          }
    CHECK(covered == pl.live && (long long)(whole.size() + parts.size()) == pl.live && (long long)whole.size() == pl.full &&
              (long long)parts.size() == pl.tail, "covered %lld whole %zu split %zu", covered, whole.size(), parts.size());
    std::printf("plan %d %lld %lld %d %d %d %lld %lld\n", pl.S, pl.live, pl.full, pl.tail, pl.splits, pl.tps, pl.total, worst);
  }
  return 0;
}
