// Stand-alone host check of csrc/fwd_route.h (tests/test_fwd_route_cpu.py compiles and runs it, with the host compiler's address
// and undefined-behaviour sanitizers). One call per line of stdin -- the columns of
// tests/golden/fwd_route_parent.json without the name, the environment written out as the four switches:
//   N H W C ldx K Kpad ldy R stride dil batch x_bs w_bs affine in_ss_stride epilogue res stats w_split y_off k_steps k_imgs k_base
//   w_img_stride  gemm variant tail split_mfma
// For every call the route is checked against what the kernels assume (their comments), and one line is printed:
//   code status kernel M BM BN BK variant affine per_sample mfma mode tiles256 full rem mtiles ntiles rows_per_group
// The program exits non-zero with a message at the first violated property.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fwd_route.h"

static const char* const NAMES[FWD_KERNELS] = {"conv_igemm", "dgrad_s2", "stem7", "few_rows", "gemm_nt", "gemm_nt_perimg", "gemm_nt_bf16x3", "conv_bf16x3", "rowaff_bf16x3"};
static int line = 0;

#define CHECK(cond, ...)                                                           \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "case %d (%s): %s: ", line, NAMES[r.kernel], #cond);    \
      std::fprintf(stderr, __VA_ARGS__);                                           \
      std::fprintf(stderr, "\n");                                                  \
      return false;                                                                \
    }                                                                              \
  } while (0)

// every 128 x 128 output tile of the product exactly once: the walk of gemm_rounds_check.cpp on this route's launches
static bool check_cover(const FwdRoute& r, const MssConvArgs& p) {
  const long long nb = p.batch > 1 ? p.batch : 1;
  const long long narrow = (long long)r.mtiles * ((p.K + 127) / 128) * nb;
  std::vector<int> hits(narrow, 0);                                         // exactly `narrow` ints: a tile behind them is a sanitizer report
  if (r.BN != 256) {
    CHECK(r.rounds.mode == MSS_GEMM_NARROW && (long long)r.mtiles * r.ntiles * nb == narrow, "%d x %d tiles", r.mtiles, r.ntiles);
    for (long long t = 0; t < narrow; ++t) ++hits[t];
  } else {
    const long long tiles256 = (long long)r.mtiles * r.ntiles * nb;
    CHECK(p.K % 256 == 0 && r.ntiles == p.K / 256 && 2 * tiles256 == narrow, "%lld wide tiles of %lld narrow", tiles256, narrow);
    long long wide_end = tiles256;
    if (r.rounds.mode == MSS_GEMM_HYBRID) {
      CHECK(r.kernel == FWD_GEMM_NT && r.rounds.full > 0 && r.rounds.rem > 0 && r.rounds.full + r.rounds.rem == tiles256 && r.rounds.tiles256 == tiles256,
            "full %lld rem %lld", r.rounds.full, r.rounds.rem);
      wide_end = r.rounds.full;
      for (long long t = 2 * r.rounds.full; t < 2 * tiles256; ++t) ++hits[t];       // the second launch: ntiles doubled
    } else {
      CHECK(r.rounds.mode == MSS_GEMM_WIDE, "mode %d on 256-wide tiles", r.rounds.mode);
    }
    for (long long w = 0; w < wide_end; ++w) { ++hits[2 * w]; ++hits[2 * w + 1]; }
  }
  for (long long t = 0; t < narrow; ++t) CHECK(hits[t] == 1, "narrow tile %lld covered %d times", t, hits[t]);
  return true;
}

static bool check(const FwdRoute& r, const MssConvArgs& p, const FwdSwitches& sw) {
  auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const long long nb = p.batch > 1 ? p.batch : 1;
  const long long M = (long long)p.N * p.OH * p.OW;
  const bool one_by_one = p.R * p.S == 1 && p.stride == 1 && p.pad == 0 && p.H == p.OH && p.W == p.OW;
  const bool gemm_family = r.kernel == FWD_GEMM_NT || r.kernel == FWD_GEMM_NT_PERIMG || r.kernel == FWD_GEMM_NT_BF16X3 || r.kernel == FWD_CONV_BF16X3 || r.kernel == FWD_ROWAFF_BF16X3;
  CHECK(r.status == MSS_OK && r.M == M && M > 0, "status %d M %d", r.status, r.M);
  CHECK(r.affine == (p.in_scale != nullptr) || r.kernel == FWD_STEM7 || r.kernel == FWD_FEW_ROWS, "affine %d", (int)r.affine);
  if (r.kernel != FWD_FEW_ROWS) CHECK(p.Kpad >= r.ntiles * r.BN && r.ntiles >= 1, "Kpad %d < %d x %d", p.Kpad, r.ntiles, r.BN);
  // 32-bit offsets, written out independently of fwd_span32
  const unsigned __int128 span_x = ((unsigned __int128)(nb - 1) * (unsigned long long)p.x_bs + (unsigned __int128)M * p.ldx) * 4;
  const unsigned __int128 span_w = ((unsigned __int128)(nb - 1) * (unsigned long long)p.w_bs + (unsigned __int128)p.Kpad * p.C) * 4;
  switch (r.kernel) {
    case FWD_DGRAD_S2:
      CHECK(p.stride == -2 && r.BK == 16 && (p.K <= 64 ? r.BM == 256 && r.BN == 64 : r.BM == 128 && r.BN == 128) && !r.per_sample, "tile %d x %d x %d", r.BM, r.BN, r.BK);
      break;
    case FWD_STEM7:
      CHECK(p.R == 7 && p.C == 4 && p.K == MSS_STEM7_K && r.BN == MSS_STEM7_K, "stem shape");
      break;
    case FWD_FEW_ROWS:
      CHECK(one_by_one && M <= r.BM && (r.BM == 8 || r.BM == 16 || r.BM == 32) && (r.BM == 8 || M > r.BM / 2) && p.batch <= 1 && (sw.gemm || p.k_steps), "bucket %d for %lld rows", r.BM, M);
      CHECK(!p.in_scale && !p.in_relu && !p.out_scale && !p.out_relu && !p.res && !p.stats && p.C % 4 == 0 && p.ldx % 4 == 0 && al(p.x) && al(p.w), "nothing fused, 16-byte rows");
      break;
    case FWD_CONV_IGEMM:
      CHECK((r.BM == 256 && r.BN == 64 && r.BK == 16 && p.K <= 64) || (r.BM == 128 && r.BN == 128 && (r.BK == 16 || r.BK == 32) && p.K > 64), "tile %d x %d x %d", r.BM, r.BN, r.BK);
      CHECK(p.C % r.BK == 0 && r.mtiles == (M + r.BM - 1) / r.BM && r.ntiles == (p.K + r.BN - 1) / r.BN && !p.k_steps, "tiles %d x %d", r.mtiles, r.ntiles);
      CHECK(r.per_sample == (p.in_scale && p.in_ss_stride && (p.OH * p.OW) % r.BM != 0), "per_sample %d", (int)r.per_sample);
      CHECK(r.rows_per_group == 0, "p.H is the image's height");
      break;
    default:
      CHECK(gemm_family, "kernel %d", (int)r.kernel);
      CHECK(r.mtiles == (M + MSS_GEMM_BM - 1) / MSS_GEMM_BM && (r.BN == 64 || r.BN == 128 || r.BN == 256), "mtiles %d BN %d", r.mtiles, r.BN);
      CHECK(p.C % MSS_GEMM_BK == 0, "C %d", p.C);
      if (!check_cover(r, p)) return false;
      break;
  }
  if (r.kernel == FWD_GEMM_NT || r.kernel == FWD_GEMM_NT_PERIMG) {
    CHECK(one_by_one && (sw.gemm || p.k_steps) && p.C / MSS_GEMM_BK >= 2 && (r.variant == 2 || r.variant == 3), "variant %d", r.variant);
    CHECK(r.variant != 3 || (p.C / MSS_GEMM_BK >= 3 && (r.kernel == FWD_GEMM_NT_PERIMG || (span_x < 0xffffffffull && span_w < 0xffffffffull))), "variant 3 beyond its offsets");
    CHECK(r.variant == 3 || sw.variant != 3 || p.C / MSS_GEMM_BK < 3 || span_x >= 0xffffffffull || span_w >= 0xffffffffull, "variant 2 without a reason");
    CHECK((r.BN == 64) == (p.K <= 64) && (r.BN != 64 || (r.variant == 3 && p.K >= 32 && M >= 16384)), "BN %d for K %d", r.BN, p.K);
    CHECK(!r.per_sample && r.mfma == 0 && (!p.w_split || r.kernel == FWD_GEMM_NT), "fields of another family");
    // rows that share an affine: tiles must not straddle them
    CHECK(r.rows_per_group > 0 && (!(p.in_scale && p.in_ss_stride) || (r.rows_per_group == p.OH * p.OW && r.rows_per_group % MSS_GEMM_BM == 0)), "rows per group %d", r.rows_per_group);
  }
  if (r.kernel == FWD_GEMM_NT_PERIMG) {
    CHECK(p.k_steps && r.variant == 3 && !r.affine && r.BN != 64 && r.rounds.mode != MSS_GEMM_HYBRID, "per-image instantiation");
    CHECK(p.k_imgs > 0 ? r.rows_per_group == M : (r.rows_per_group == p.OH * p.OW && r.rows_per_group % MSS_GEMM_BM == 0), "rows per image %d", r.rows_per_group);
  } else {
    CHECK(!p.k_steps || r.kernel == FWD_FEW_ROWS, "k_steps on another kernel");
  }
  if (r.kernel == FWD_GEMM_NT_BF16X3 || r.kernel == FWD_CONV_BF16X3 || r.kernel == FWD_ROWAFF_BF16X3) {
    CHECK(p.w_split && al(p.w_split) && p.K > 64 && p.Kpad % 128 == 0 && r.BN != 64 && r.rounds.mode != MSS_GEMM_HYBRID && r.variant == 0, "split route");
    CHECK(r.mfma == 16 || r.mfma == 32, "mfma %d", r.mfma);
    CHECK(r.mfma != 16 || (split_mf16_ok(p) && r.kernel == FWD_GEMM_NT_BF16X3 && !r.affine && sw.split_mfma != 32), "the 16x16x32 form");
    CHECK(r.mfma != 16 || (p.K % 4 == 0 && p.ldy % 4 == 0 && al(p.y) && (!p.res || (al(p.res) && p.ldres % 4 == 0)) && (!p.stats || al(p.stats))), "16-byte stores");
    CHECK(r.per_sample == (r.kernel == FWD_ROWAFF_BF16X3), "per_sample %d", (int)r.per_sample);
    CHECK((r.kernel == FWD_CONV_BF16X3) == !one_by_one && (r.kernel == FWD_CONV_BF16X3 ? r.rows_per_group == 0 : r.rows_per_group > 0), "rows per group %d", r.rows_per_group);
    CHECK(r.kernel != FWD_GEMM_NT_BF16X3 || sw.gemm, "MSS_GEMM=0 gave the NT GEMM");
  }
  if (r.per_sample) CHECK(p.in_scale && p.in_ss_stride && (p.OH * p.OW) % (r.kernel == FWD_CONV_IGEMM ? r.BM : MSS_GEMM_BM) != 0, "per_sample without straddling tiles");
  return true;
}

int main() {
  alignas(16) static float fake[64];                       // pointer fields are only compared with null and read for their alignment
  alignas(16) static int fake_steps[4];
  int N, H, W, C, ldx, K, Kpad, ldy, R, stride, dil, batch, affine, ss, epilogue, res, stats, w_split, y_off, k_steps, k_imgs, k_base;
  long long x_bs, w_bs, w_img_stride;
  FwdSwitches sw;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %d %d %d %d %d %d %d %d %d %d %lld %d %d %d %d", &N, &H, &W, &C, &ldx, &K, &Kpad, &ldy, &R,
                    &stride, &dil, &batch, &x_bs, &w_bs, &affine, &ss, &epilogue, &res, &stats, &w_split, &y_off, &k_steps, &k_imgs, &k_base,
                    &w_img_stride, &sw.gemm, &sw.variant, &sw.tail, &sw.split_mfma) == 29) {
    ++line;
    MssConvArgs p;
    std::memset(&p, 0, sizeof p);
    p.pad = dil * (R / 2);
    p.N = N; p.H = H; p.W = W; p.C = C; p.ldx = ldx; p.K = K; p.Kpad = Kpad; p.ldy = ldy;
    p.R = p.S = R; p.stride = stride; p.dil = dil;
    if (stride == -2) { p.OH = 2 * H; p.OW = 2 * W; }
    else { p.OH = (H + 2 * p.pad - dil * (R - 1) - 1) / stride + 1; p.OW = (W + 2 * p.pad - dil * (R - 1) - 1) / stride + 1; }
    p.x = p.w = fake; p.y = fake + y_off / 4;
    if (affine == 1) p.in_scale = p.in_shift = fake;
    p.in_relu = affine != 0; p.in_ss_stride = ss;
    if (epilogue) { p.out_scale = p.out_shift = fake; p.out_relu = 1; }
    if (res) { p.res = fake + (res == 2 ? 1 : 0); p.ldres = ldy; }
    if (stats) p.stats = fake;
    if (w_split) p.w_split = fake + (w_split == 2 ? 1 : 0);
    if (k_steps) p.k_steps = fake_steps;
    p.batch = batch;
    if (batch > 1) {
      p.x_bs = x_bs ? x_bs : (long long)N * H * W * ldx;
      p.w_bs = w_bs ? w_bs : (long long)Kpad * C;
      p.y_bs = (long long)N * p.OH * p.OW * ldy;
    }
    p.k_imgs = k_imgs; p.k_base = k_base; p.w_img_stride = w_img_stride;
    const FwdRoute r = fwd_route(p, sw);
    if (!check(r, p, sw)) return 1;
    std::printf("%d %d %s %d %d %d %d %d %d %d %d %d %lld %lld %lld %d %d %d\n", fwd_route_code(r), r.status, NAMES[r.kernel], r.M, r.BM, r.BN, r.BK, r.variant,
                (int)r.affine, (int)r.per_sample, r.mfma, r.rounds.mode, r.rounds.tiles256, r.rounds.full, r.rounds.rem, r.mtiles, r.ntiles, r.rows_per_group);
  }
  return 0;
}
