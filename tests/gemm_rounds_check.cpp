// Stand-alone host check of csrc/gemm_rounds.h (tests/test_gemm_rounds_cpu.py compiles and runs it, with the host compiler's address
// and undefined-behaviour sanitizers). One case per line of stdin:
//   mtiles K C batch tail_mode
// For every case the tile ranges of the plan are walked as gemm.hip launches them -- wide tiles [0, full), narrow tiles
// [2 * full, 2 * tiles256) for a hybrid, every wide or every narrow tile otherwise -- and every 128 x 128 output tile of the product
// must be covered exactly once. Prints one line per case:
//   plan mode tiles256 full rem grid_first grid_second
// (the grids at 2 wide / 3 narrow workgroups per CU on 256 CUs; grid_second 0 without a second launch) and exits non-zero with a
// message at the first violated property.
// `gemm_rounds_check width` reads `mtiles K C batch` per line and prints the three width rules: `wide wide_perimg wide_split_conv`
// (tests/test_fwd_route_cpu.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "gemm_rounds.h"

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::fprintf(stderr, "case %d: %s: ", line, #cond);  \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      return 1;                                            \
    }                                                      \
  } while (0)

int main(int argc, char** argv) {
  int line = 0;
  int mtiles, K, C, batch, tail_mode;
  // the split-bf16 launcher's margin (gemm_bf16x3.hip) on its documented case: 2304 tiles at 2 workgroups per CU on 256 CUs are 4.5
  // rounds of 512 or 9 whole rounds of 256 -- 10 % more of the slots filled, which 0.15 leaves at two per CU and gemm.hip's 0.02 does not
  CHECK(mss_gemm_grid(2304, 2, 256, 0.15) == 512 && mss_gemm_grid(2304, 2, 256, 0.02) == 256, "grids %d %d",
        mss_gemm_grid(2304, 2, 256, 0.15), mss_gemm_grid(2304, 2, 256, 0.02));
  if (argc == 2 && !std::strcmp(argv[1], "width")) {
    while (std::scanf("%d %d %d %d", &mtiles, &K, &C, &batch) == 4)
      std::printf("%d %d %d\n", (int)mss_gemm_wide(mtiles, K, C, batch), (int)mss_gemm_wide_perimg(mtiles, K, C), (int)mss_gemm_wide_split_conv(mtiles, K));
    return 0;
  }
  while (std::scanf("%d %d %d %d %d", &mtiles, &K, &C, &batch, &tail_mode) == 5) {
    ++line;
    const MssGemmRounds r = mss_gemm_rounds(mtiles, K, C, batch, tail_mode);
    const long long nb = batch > 1 ? batch : 1;
    const long long narrow = (long long)mtiles * ((K + 127) / 128) * nb;      // 128 x 128 tiles of the whole product
    std::vector<int> hits(narrow, 0);                                       // exactly `narrow` ints: a tile behind them is a sanitizer report
    long long first = 0, second = 0;
    if (r.mode == MSS_GEMM_NARROW) {
      CHECK(r.full == 0 && r.rem == 0, "full %lld rem %lld on a narrow plan", r.full, r.rem);
      for (long long t = 0; t < narrow; ++t) ++hits[t];
      first = narrow;
    } else {
      CHECK(K % 256 == 0 && C >= 256 && r.tiles256 == (long long)mtiles * (K / 256) * nb && 2 * r.tiles256 == narrow,
            "tiles256 %lld of %lld narrow tiles", r.tiles256, narrow);
      long long wide_end = r.tiles256;
      if (r.mode == MSS_GEMM_HYBRID) {
        CHECK(r.full > 0 && r.full % MSS_GEMM_WIDE_SLOTS == 0 && r.rem > 0 && r.rem <= MSS_GEMM_TAIL_MAX && r.full + r.rem == r.tiles256,
              "full %lld rem %lld", r.full, r.rem);
        wide_end = r.full;
        for (long long t = 2 * r.full; t < 2 * r.tiles256; ++t) ++hits[t];
        second = 2 * r.rem;
      } else {
        CHECK(r.mode == MSS_GEMM_WIDE && r.full == 0 && r.rem == 0, "mode %d full %lld rem %lld", r.mode, r.full, r.rem);
      }
      for (long long w = 0; w < wide_end; ++w) { ++hits[2 * w]; ++hits[2 * w + 1]; }      // wide tile w = narrow tiles 2w and 2w + 1
      first = wide_end;
    }
    for (long long t = 0; t < narrow; ++t) CHECK(hits[t] == 1, "narrow tile %lld covered %d times", t, hits[t]);
    const int g1 = mss_gemm_grid(first, r.mode == MSS_GEMM_NARROW ? 3 : 2, 256, 0.02);      // gemm.hip's margin
    const int g2 = second ? mss_gemm_grid(second, 3, 256, 0.02) : 0;
    CHECK(g1 >= 1 && g1 <= first && g1 <= 768 && (second == 0 || (g2 >= 1 && g2 <= second && g2 <= 768)), "grids %d %d", g1, g2);
    std::printf("plan %d %lld %lld %lld %d %d\n", r.mode, r.tiles256, r.full, r.rem, g1, g2);
  }
  return 0;
}
