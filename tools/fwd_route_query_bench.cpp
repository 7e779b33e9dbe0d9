// Host cost of mss_conv2d_forward_route: 100 000 calls, five repeats, on three rows of tests/golden/fwd_route_parent.json --
// dl_1x512x1024_aspp_3x3_d12 (conv_igemm_kernel), aspp_compose (the dense hybrid GEMM), dropped_f6_aspp (the k_imgs per-image GEMM).
// No GPU, no Python: the library is loaded with dlopen, the pointers are fake and never read.
//   g++ -O2 tools/fwd_route_query_bench.cpp -o /tmp/fwd_route_query_bench -ldl && /tmp/fwd_route_query_bench path/to/libmss_hip.so
// Run it on two builds alternately; profiles/fwd_route/README.md has the recorded numbers.
#include <dlfcn.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include "../include/mss_hip.h"
int main(int argc, char** argv) {
  void* h = dlopen(argv[1], RTLD_NOW); if (!h) { puts(dlerror()); return 1; }
  auto fn = (int (*)(const MssConvArgs*))dlsym(h, "mss_conv2d_forward_route");
  alignas(16) static float fake[64]; static int st[4];
  MssConvArgs a[3]; memset(a, 0, sizeof a);
  for (auto& p : a) { p.x = p.w = fake; p.y = fake; p.N = 1; p.R = p.S = 1; p.stride = 1; p.dil = 1; }
  // igemm: 1x64x128 4096->256 3x3 d12 affine
  a[0].H = a[0].OH = 64; a[0].W = a[0].OW = 128; a[0].C = a[0].ldx = 4096; a[0].K = a[0].Kpad = a[0].ldy = 256; a[0].R = a[0].S = 3; a[0].dil = a[0].pad = 12; a[0].in_scale = a[0].in_shift = fake; a[0].in_relu = 1;
  // hybrid: 7168 x 4096 -> 4096
  a[1].H = a[1].OH = 1; a[1].W = a[1].OW = 7168; a[1].C = a[1].ldx = 4096; a[1].K = a[1].Kpad = a[1].ldy = 4096;
  // k_imgs: 72 x 2592 x 4096 -> 256
  a[2].H = a[2].OH = 1; a[2].W = a[2].OW = 2592; a[2].C = a[2].ldx = 4096; a[2].K = a[2].Kpad = a[2].ldy = 256; a[2].batch = 72; a[2].x_bs = 2592ll * 4096; a[2].w_bs = 256 * 4096; a[2].y_bs = 2592 * 256; a[2].k_steps = st; a[2].k_imgs = 2; a[2].k_base = 8;
  for (int c = 0; c < 3; ++c) {
    double reps[5]; int code = 0;
    for (int r = 0; r < 5; ++r) {
      auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < 100000; ++i) code += fn(&a[c]);
      reps[r] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / 1e5;
    }
    std::sort(reps, reps + 5);
    printf("row %d code %d: ns/call min %.1f median %.1f max %.1f\n", c, fn(&a[c]), reps[0], reps[2], reps[4]);
  }
}
