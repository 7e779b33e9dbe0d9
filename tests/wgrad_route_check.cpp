// Stand-alone host check of csrc/wgrad_route.h (tests/test_wgrad_route_cpu.py compiles and runs it, with the host compiler's address
// and undefined-behaviour sanitizers). `wgrad_route_check split CAP` prints split_search(base, slots, CAP) for base 1..5000 and slots
// 512, 768, 1024; `wgrad_route_check reduce` prints wg_reduce_group(slab4, splits) for every slab4 of REDUCE_SLAB4 (below) and splits
// 1..600, slab4 outermost. Otherwise one case per line of stdin (the columns of tests/golden/wgrad_route_parent.json with the switches written out):
//   M C K Kpad Cp lddy ldx R stride dil batch affine in_ss_stride route k_imgs  tn narrow tn_affine tn_tail
// For every case and every combination of WgradFacts the chosen route (for the two-part route: both parts) is checked against the
// kernels' preconditions as their comments state them, the job counts their decodes assume and the scratch formulas, and against the
// workspace query. The split-bf16 route is not offered (its rule lives in gemm_bf16x3.hip). Prints one line per case, for aligned pointers:
//   kernel splits rows_per_split total full ws_bytes wide_K query_bytes [first-part kernel, second-part kernel]
// and exits non-zero with a message at the first violated property.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "wgrad_route.h"

static const char* const NAMES[] = {"conv32", "conv64", "conv128", "narrow", "tn_lds", "tn_wide", "tn_direct", "tn_direct_tail", "tn_direct_perimg", "tn_bf16x3", "two_part"};
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

static long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// around every threshold of the rule (65536 / G float4s) and far from them; tests/test_wgrad_route_cpu.py has the same list
static const long long REDUCE_SLAB4[] = {1, 304, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769,
                                         65535, 65536, 65537, 73728, 1048576, 1ll << 33};

// one launched product: r is what wgrad_route chose for p
static bool check_launch(const WgradRoute& r, const MssConvArgs& p, int lddy, int Cp, WgradFacts f, const WgradSwitches& sw, long long query) {
  const bool prologue = p.in_scale || p.in_shift || p.in_relu, vectors = p.in_scale || p.in_shift, one_by_one = p.R * p.S == 1;
  const bool plain = p.stride == 1 && p.pad == 0 && p.OH == p.H && p.OW == p.W;
  const int P = p.batch > 1 ? p.batch : 1;
  CHECK(r.ws_bytes <= query, "%lld > %lld", r.ws_bytes, query);
  CHECK(f.dense_dy == (lddy == p.K) && lddy >= p.K, "lddy %d", lddy);
  if (r.kernel == WG_TN_DIRECT_PERIMG) {
    CHECK(p.k_steps && r.ws_bytes == 0 && r.splits == 1 && r.rows_per_split == p.M && r.full == -1, "per-image form");
    CHECK(r.positions == p.batch && r.total == (long long)p.batch * (p.K / 128) * (p.C / 128), "total %lld", r.total);
    return true;
  }
  CHECK(!p.k_steps, "k_steps on another kernel");
  int granule = 0;
  long long tiles = 0;
  switch (r.kernel) {
    case WG_CONV_32: case WG_CONV_64: case WG_CONV_128: {
      const int bko = r.kernel == WG_CONV_32 ? 32 : r.kernel == WG_CONV_64 ? 64 : 128;
      CHECK(p.K <= bko || bko == 128, "K %d on the %d-row tile", p.K, bko);
      CHECK(r.positions == (p.batch > 1 ? p.batch : p.R * p.S), "positions %d", r.positions);
      granule = 16; tiles = cdiv(p.K, bko) * cdiv(p.C, 128) * r.positions;
      break;
    }
    case WG_NARROW:
      // a streaming 1x1 kernel over dense rows: <= 64 output channels in float2 pairs above 32, whole 128-column tiles of an unpadded
      // result, float4 loads of x and of one affine for all rows, at least 16 384 rows
      CHECK(sw.narrow != 0 && one_by_one && plain && p.batch <= 1 && p.K <= 64 && p.C % 128 == 0 && Cp == p.C && p.ldx % 4 == 0, "shape");
      CHECK(f.x16 && (!vectors || (f.affine16 && p.in_ss_stride == 0)), "x / affine");
      CHECK(p.K <= 32 || (p.K % 2 == 0 && lddy % 2 == 0 && f.dy8), "float2 loads of dy");
      CHECK(p.M >= 16384 && r.positions == 1, "rows %d", p.M);
      granule = 2; tiles = p.C / 128;
      break;
    case WG_TN_LDS: case WG_TN_WIDE:
      // dense [rows][K] x [rows][C] operands per position, float4 staging, no prologue
      CHECK(sw.tn != 0 && one_by_one && p.K % 4 == 0 && p.C % 4 == 0 && p.ldx == p.C && f.dense_dy && !prologue, "operands");
      CHECK(p.batch > 1 ? (p.x_bs % 4 == 0 && p.y_bs % 4 == 0 && p.N == 1 && p.H == 1) : (plain && p.K >= 128 && p.C >= 128), "positions");
      CHECK(r.kernel != WG_TN_WIDE || p.C % 256 == 0, "C %d on 256-wide tiles", p.C);
      CHECK(r.kernel == WG_TN_LDS || sw.tn >= 4, "MSS_WGRAD_TN=%d gave the wide kernel", sw.tn);
      CHECK(r.positions == P, "positions %d", r.positions);
      granule = 16; tiles = cdiv(p.K, 128) * cdiv(p.C, r.kernel == WG_TN_WIDE ? 256 : 128) * P;
      break;
    case WG_TN_DIRECT: case WG_TN_DIRECT_TAIL:
      // whole 128 x 128 tiles, 16-byte loads, a row stride for dy (one position only), one aligned affine for all rows (one position only)
      CHECK((sw.tn == 5 || sw.tn == 7) && one_by_one && p.K % 128 == 0 && p.C % 128 == 0 && p.K <= 4096 && p.ldx == p.C && lddy % 4 == 0, "operands");
      CHECK(f.dense_dy || p.batch <= 1, "a row stride with positions");
      CHECK(!prologue || (p.batch <= 1 && p.in_ss_stride == 0 && sw.tn_affine != 0 && (!vectors || f.affine16)), "prologue");
      CHECK(p.batch > 1 ? (p.x_bs % 4 == 0 && p.y_bs % 4 == 0 && p.N == 1 && p.H == 1) : plain, "positions");
      CHECK(r.positions == P && (r.kernel == WG_TN_DIRECT_TAIL) == (r.full >= 0), "full %lld", r.full);
      CHECK(r.full < 0 || sw.tn_tail != 0, "MSS_WGRAD_TN_TAIL=0 gave the tail plan");
      granule = 2; tiles = (long long)(p.K / 128) * (p.C / 128) * P;
      break;
    default:
      CHECK(false, "not a launch");
  }
  CHECK(r.splits >= 1 && (long long)(r.splits - 1) * r.rows_per_split < p.M && p.M <= (long long)r.splits * r.rows_per_split, "splits %d x %d rows for %d", r.splits, r.rows_per_split, p.M);
  CHECK(r.rows_per_split % granule == 0, "rows per split %d", r.rows_per_split);
  if (r.full >= 0) {
    CHECK(r.full < r.total && r.full % 1024 == 0 && (r.total - r.full) % r.splits == 0 && r.full + (r.total - r.full) / r.splits == tiles, "tail plan %lld + %lld", r.full, r.total - r.full);
    CHECK(r.splits >= 2 && r.ws_bytes == (r.total - r.full) * 128ll * 128 * 4, "tail scratch %lld", r.ws_bytes);
  } else {
    CHECK(r.total == tiles * r.splits, "total %lld, %lld tiles", r.total, tiles);
    CHECK(r.ws_bytes == (r.splits > 1 ? (long long)r.splits * r.positions * p.Kpad * Cp * 4 : 0), "scratch %lld", r.ws_bytes);
  }
  // the reduce launch: none for one split and for the tail plan (its own reducer), else the group of the slab's float4 count
  CHECK(r.reduce_group == (r.splits > 1 && r.full < 0 ? wg_reduce_group((long long)r.positions * p.Kpad * Cp / 4, r.splits) : 0), "reduce group %d", r.reduce_group);
  return true;
}

static bool check_route(const MssConvArgs& p, int lddy, int Cp, WgradFacts f, const WgradSwitches& sw, long long query) {
  const WgradRoute r = wgrad_route(p, lddy, Cp, f, sw);
  if (r.kernel != WG_TWO_PART) return check_launch(r, p, lddy, Cp, f, sw, query);
  CHECK(r.wide_K > 0 && r.wide_K % 128 == 0 && p.K - r.wide_K > 0 && p.K - r.wide_K <= 64 && p.Kpad >= p.K && sw.narrow != 0, "wide part %d of %d", r.wide_K, p.K);
  f.dense_dy = false;
  const MssConvArgs a = wgrad_part(p, r.wide_K, false), b = wgrad_part(p, r.wide_K, true);
  const WgradRoute ra = wgrad_route(a, lddy, Cp, f, sw), rb = wgrad_route(b, lddy, Cp, f, sw);
  CHECK(rb.kernel == WG_NARROW && ra.kernel != WG_TWO_PART, "parts %s, %s", NAMES[ra.kernel], NAMES[rb.kernel]);
  CHECK(r.ws_bytes >= ra.ws_bytes && r.ws_bytes >= rb.ws_bytes && r.ws_bytes <= query, "scratch %lld of %lld", r.ws_bytes, query);
  CHECK(a.K + b.K == p.K && a.Kpad + b.Kpad == p.Kpad && a.Kpad == a.K, "rows of dwp");
  return check_launch(ra, a, lddy, Cp, f, sw, query) && check_launch(rb, b, lddy, Cp, f, sw, query);
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "split")) {
    const int slots[3] = {512, 768, 1024};
    for (int s = 0; s < 3; ++s)
      for (int base = 1; base <= 5000; ++base) std::printf("%d\n", split_search(base, slots[s], std::atoi(argv[2])));
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "reduce")) {
    for (long long slab4 : REDUCE_SLAB4)
      for (int splits = 1; splits <= 600; ++splits) std::printf("%d\n", wg_reduce_group(slab4, splits));
    return 0;
  }
  static float fake[64];                       // pointer fields are only compared with null
  static int fake_steps[1];
  int M, C, K, Kpad, Cp, lddy, ldx, R, stride, dil, batch, affine, ss, route, k_imgs;
  WgradSwitches sw;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &M, &C, &K, &Kpad, &Cp, &lddy, &ldx, &R, &stride, &dil, &batch,
                    &affine, &ss, &route, &k_imgs, &sw.tn, &sw.narrow, &sw.tn_affine, &sw.tn_tail) == 19) {
    ++line;
    MssConvArgs p;
    std::memset(&p, 0, sizeof p);
    p.x = p.w = fake; p.y = fake;
    if (affine == 1) p.in_scale = p.in_shift = fake;
    p.in_relu = affine != 0; p.in_ss_stride = ss;
    p.N = 1; p.C = C; p.ldx = ldx; p.K = K; p.Kpad = Kpad; p.ldy = lddy;
    p.R = p.S = R; p.stride = stride; p.dil = dil; p.pad = dil * (R / 2);
    p.H = R == 1 ? 1 : (M + 63) / 64; p.W = R == 1 ? M : 64;
    p.OH = (p.H - 1) / stride + 1; p.OW = (p.W - 1) / stride + 1;
    p.M = p.N * p.OH * p.OW;
    p.batch = batch; p.route = route;
    if (batch > 1) { p.x_bs = (long long)p.H * p.W * C; p.y_bs = (long long)p.M * K; }
    if (k_imgs) { p.k_imgs = k_imgs; p.k_base = 8; p.k_steps = fake_steps; }
    const long long query = wgrad_workspace_bytes(p, Cp, sw);
    for (int m = 0; m < 16; ++m) {
      WgradFacts f;
      f.dense_dy = !(m & 1); f.dy8 = !(m & 2); f.x16 = !(m & 4); f.affine16 = !(m & 8);
      if (!f.dense_dy && batch > 1) continue;            // Winograd-domain products always have a dense dy
      const int ld = f.dense_dy ? K : lddy != K ? lddy : K + 4;
      if (!check_route(p, ld, Cp, f, sw, query)) return 1;
    }
    WgradFacts f;
    f.dense_dy = lddy == K;
    const WgradRoute r = wgrad_route(p, lddy, Cp, f, sw);
    std::printf("%s %d %d %lld %lld %lld %d %lld", NAMES[r.kernel], r.splits, r.rows_per_split, r.total, r.full, r.ws_bytes, r.wide_K, query);
    if (r.kernel == WG_TWO_PART) {
      f.dense_dy = false;
      std::printf(" %s %s", NAMES[wgrad_route(wgrad_part(p, r.wide_K, false), lddy, Cp, f, sw).kernel],
                  NAMES[wgrad_route(wgrad_part(p, r.wide_K, true), lddy, Cp, f, sw).kernel]);
    }
    std::printf("\n");
  }
  return 0;
}
