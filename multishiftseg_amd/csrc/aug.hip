// libmss_aug.so, part 1 (include/mss_aug_hip.h): the point-wise and reducing stages of the Mask2Former input pipeline --
// load (mixup + ToTensor), image statistics, the fused colour run (ColorJitter's four ops, autocontrast) and equalize.
// Everything streams once over <= 50 MB; the kernels are plain, coalesced and bit-reproducible (no float atomics).
// Nothing here uses MSS_ENV_INT or any symbol of libmss_hip.so.
#include "mss_common.h"
#include "../../include/mss_aug_hip.h"

namespace {

__device__ __forceinline__ double pin(double v) { asm volatile("" : "+v"(v)); return v; }   // forbid fma contraction
__device__ __forceinline__ float pinf(float v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

inline int common_check(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return MSS_ERR_BAD_ARG;
  if (N > MSS_AUG_MAX_IMAGES || (long long)H * W > MSS_AUG_MAX_PIXELS) return MSS_ERR_UNSUPPORTED;
  return MSS_OK;
}

// ---- load: grid ceil(HW / 256) ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void load_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ gen,
                                                   const uint8_t* __restrict__ tgt, const uint8_t* __restrict__ gen_tgt, int HW,
                                                   int use_mix, double p, float* __restrict__ x, uint8_t* __restrict__ m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint8_t a = img[(long long)i * 3 + c];
    uint8_t g = gen[(long long)i * 3 + c];
    if (use_mix) {      // cityscapes.py:161-164: (p * image + (1 - p) * gen_image).astype(np.uint8), float64
      const double t1 = pin(p * (double)a), t2 = pin((1.0 - p) * (double)g);
      g = (uint8_t)(int)(t1 + t2);
    }
    x[(long long)c * HW + i] = (float)a / 255.0f;
    x[(long long)(3 + c) * HW + i] = (float)g / 255.0f;
  }
  m[i] = tgt[i];
  m[(long long)HW + i] = gen_tgt[i];
}

// ---- stats -----------------------------------------------------------------------------------------------------------------------
constexpr int STAT_BLOCKS_MAX = 256;      // partial workgroups per image
constexpr int STAT_VALS = 8;              // gray sum, (min, max) x 3, unused
inline int stat_blocks(long long HW) { return (int)((HW + 4095) / 4096 < STAT_BLOCKS_MAX ? (HW + 4095) / 4096 : STAT_BLOCKS_MAX); }

struct Stat { double sum; float lo[3], hi[3]; };
__device__ __forceinline__ void stat_fold(Stat& a, const Stat& b) {
  a.sum += b.sum;
#pragma unroll
  for (int c = 0; c < 3; ++c) { a.lo[c] = fminf(a.lo[c], b.lo[c]); a.hi[c] = fmaxf(a.hi[c], b.hi[c]); }
}
// fixed tree over the 256 threads of a workgroup; the result is in thread 0
__device__ __forceinline__ void stat_block_reduce(Stat& s, Stat* lds) {
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { Stat t = lds[threadIdx.x]; stat_fold(t, lds[threadIdx.x + o]); lds[threadIdx.x] = t; }
    __syncthreads();
  }
  s = lds[0];
}
__device__ __forceinline__ Stat stat_empty() {
  Stat s; s.sum = 0.0;
  for (int c = 0; c < 3; ++c) { s.lo[c] = INFINITY; s.hi[c] = -INFINITY; }
  return s;
}

// grid (nb, N): workgroup j of image n takes pixels j*256 + t, + nb*256, ...
__global__ __launch_bounds__(256) void stats_partial_kernel(const float* __restrict__ x, int HW, int nb, double* __restrict__ ws) {
  __shared__ Stat lds[256];
  const int n = blockIdx.y;
  const float* xr = x + (long long)n * 3 * HW;
  Stat s = stat_empty();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)nb * 256) {
    const float r = xr[i], g = xr[(long long)HW + i], b = xr[2ll * HW + i];
    s.sum += (double)gray_of(r, g, b);
    s.lo[0] = fminf(s.lo[0], r); s.hi[0] = fmaxf(s.hi[0], r);
    s.lo[1] = fminf(s.lo[1], g); s.hi[1] = fmaxf(s.hi[1], g);
    s.lo[2] = fminf(s.lo[2], b); s.hi[2] = fmaxf(s.hi[2], b);
  }
  stat_block_reduce(s, lds);
  if (threadIdx.x == 0) {
    double* o = ws + ((long long)n * nb + blockIdx.x) * STAT_VALS;
    o[0] = s.sum;
    for (int c = 0; c < 3; ++c) { o[1 + 2 * c] = (double)s.lo[c]; o[2 + 2 * c] = (double)s.hi[c]; }
    o[7] = 0.0;
  }
}
// grid N: thread t folds partials t, t + 256, ... in index order (nb <= 256: one each), then the same fixed tree
__global__ __launch_bounds__(256) void stats_final_kernel(const double* __restrict__ ws, int HW, int nb, float* __restrict__ stats) {
  __shared__ Stat lds[256];
  const int n = blockIdx.x;
  Stat s = stat_empty();
  for (int j = threadIdx.x; j < nb; j += 256) {
    const double* o = ws + ((long long)n * nb + j) * STAT_VALS;
    Stat t; t.sum = o[0];
    for (int c = 0; c < 3; ++c) { t.lo[c] = (float)o[1 + 2 * c]; t.hi[c] = (float)o[2 + 2 * c]; }
    stat_fold(s, t);
  }
  stat_block_reduce(s, lds);
  if (threadIdx.x == 0) {
    float* o = stats + (long long)n * STAT_VALS;
    o[0] = (float)(s.sum / (double)HW);
    for (int c = 0; c < 3; ++c) { o[1 + 2 * c] = s.lo[c]; o[2 + 2 * c] = s.hi[c]; }
    o[7] = 0.f;
  }
}

// ---- point-wise run ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float blend(float a, float b, float r) { return clamp01(r * a + (1.f - r) * b); }

// torchvision's _rgb2hsv -> (h + f) mod 1 -> _hsv2rgb
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float f) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float div = eqc ? 1.f : cr;
  const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
  const float hr = maxc == r ? bc - gc : 0.f;
  const float hg = (maxc == g && maxc != r) ? 2.f + rc - bc : 0.f;
  const float hb = (maxc != g && maxc != r) ? 4.f + gc - rc : 0.f;
  float h = fmodf((hr + hg + hb) / 6.f + 1.f, 1.f);
  h = h + f;
  h = h - floorf(h);                                  // Python's % 1.0 (may round up to exactly 1: sextant 6 = sextant 0 below)
  const float v = maxc;
  const float h6 = h * 6.f;
  const float fl = floorf(h6);
  const float fr = h6 - fl;
  int i = (int)fl % 6;
  if (i < 0) i += 6;
  const float p = clamp01(v * (1.f - s)), q = clamp01(v * (1.f - fr * s)), t = clamp01(v * (1.f - (1.f - fr) * s));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

struct ImgStats { float mean, lo[3], sc[3]; };
__device__ __forceinline__ ImgStats read_stats(const float* stats, int n) {
  ImgStats st;
  st.mean = 0.f;
  for (int c = 0; c < 3; ++c) { st.lo[c] = 0.f; st.sc[c] = 1.f; }
  if (stats) {
    const float* o = stats + (long long)n * STAT_VALS;
    st.mean = o[0];
    for (int c = 0; c < 3; ++c) {
      const float lo = o[1 + 2 * c], sc = 1.f / (o[2 + 2 * c] - lo);
      const bool fin = isfinite(sc);
      st.lo[c] = fin ? lo : 0.f;
      st.sc[c] = fin ? sc : 1.f;
    }
  }
  return st;
}
__device__ __forceinline__ void apply_ops(const MssAugPointOps& ops, const ImgStats& st, float& r, float& g, float& b) {
  for (int k = 0; k < ops.n; ++k) {
    const float f = ops.factor[k];
    switch (ops.kind[k]) {
      case MSS_AUG_OP_BRIGHTNESS: r = blend(r, 0.f, f); g = blend(g, 0.f, f); b = blend(b, 0.f, f); break;
      case MSS_AUG_OP_CONTRAST: r = blend(r, st.mean, f); g = blend(g, st.mean, f); b = blend(b, st.mean, f); break;
      case MSS_AUG_OP_SATURATION: { const float y = gray_of(r, g, b); r = blend(r, y, f); g = blend(g, y, f); b = blend(b, y, f); break; }
      case MSS_AUG_OP_HUE: hue_shift(r, g, b, f); break;
      default:      // MSS_AUG_OP_AUTOCONTRAST (the launcher admits no other kind)
        r = clamp01((r - st.lo[0]) * st.sc[0]); g = clamp01((g - st.lo[1]) * st.sc[1]); b = clamp01((b - st.lo[2]) * st.sc[2]);
        break;
    }
  }
}
// grid (ceil(HW / V / 256), N); V = 4: float4 accesses (HW % 4 == 0), V = 1: scalar
template <int V>
__global__ __launch_bounds__(256) void pointwise_kernel(float* __restrict__ x, int HW, MssAugPointOps ops, const float* __restrict__ stats) {
  const int n = blockIdx.y;
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (i >= HW) return;
  const ImgStats st = read_stats(stats, n);
  float* pr = x + (long long)n * 3 * HW + i;
  float* pg = pr + HW;
  float* pb = pg + HW;
  if constexpr (V == 4) {
    f32x4 r = *reinterpret_cast<const f32x4*>(pr), g = *reinterpret_cast<const f32x4*>(pg), b = *reinterpret_cast<const f32x4*>(pb);
#pragma unroll
    for (int k = 0; k < 4; ++k) { float rr = r[k], gg = g[k], bb = b[k]; apply_ops(ops, st, rr, gg, bb); r[k] = rr; g[k] = gg; b[k] = bb; }
    *reinterpret_cast<f32x4*>(pr) = r; *reinterpret_cast<f32x4*>(pg) = g; *reinterpret_cast<f32x4*>(pb) = b;
  } else {
    float r = *pr, g = *pg, b = *pb;
    apply_ops(ops, st, r, g, b);
    *pr = r; *pg = g; *pb = b;
  }
}

// ---- equalize ----------------------------------------------------------------------------------------------------------------------
constexpr int EQ_BLOCKS_MAX = 128;
__device__ __forceinline__ int quantise(float v) {       // (x * 255).to(uint8): truncation; clamped so that it is always a valid bin
  int u = (int)(v * 255.0f);
  return u < 0 ? 0 : (u > 255 ? 255 : u);
}
// grid (nb, 3N): LDS histogram of the workgroup's pixels, flushed with integer global atomics
__global__ __launch_bounds__(256) void eq_hist_kernel(const float* __restrict__ x, int HW, int nb, int* __restrict__ hist) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const float* xp = x + (long long)blockIdx.y * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)nb * 256) atomicAdd(&h[quantise(xp[i])], 1);
  __syncthreads();
  const int v = h[threadIdx.x];
  if (v) atomicAdd(&hist[blockIdx.y * 256 + threadIdx.x], v);
}
// ONE workgroup of 256 threads, thread k = bin k; loops over the 3N planes
__global__ __launch_bounds__(256) void eq_lut_kernel(const int* __restrict__ hist, int planes, int* __restrict__ lut) {
  __shared__ int cum[256];
  __shared__ int last_nz;
  const int k = threadIdx.x;
  for (int pl = 0; pl < planes; ++pl) {
    const int hk = hist[pl * 256 + k];
    if (k == 0) last_nz = -1;
    cum[k] = hk;
    __syncthreads();
    if (hk) atomicMax(&last_nz, k);
    for (int o = 1; o < 256; o <<= 1) {               // inclusive scan (integers: any order gives the same sums)
      const int add = k >= o ? cum[k - o] : 0;
      __syncthreads();
      cum[k] += add;
      __syncthreads();
    }
    const int total = cum[255];
    const int last = last_nz;
    const int step = last >= 0 ? (total - hist[pl * 256 + last]) / 255 : 0;
    int v = k;
    if (step != 0) {
      v = k == 0 ? 0 : (cum[k - 1] + step / 2) / step;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
    lut[pl * 256 + k] = v;
    __syncthreads();
  }
}
// grid (ceil(HW / 256), 3N)
__global__ __launch_bounds__(256) void eq_apply_kernel(float* __restrict__ x, int HW, const int* __restrict__ lut) {
  __shared__ int l[256];
  l[threadIdx.x] = lut[blockIdx.y * 256 + threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  float* xp = x + (long long)blockIdx.y * HW + i;
  *xp = (float)l[quantise(*xp)] / 255.0f;
}

}  // namespace

extern "C" {

int mss_aug_abi_version(void) { return MSS_AUG_ABI_VERSION; }

int mss_aug_load_f32(const uint8_t* img, const uint8_t* gen, const uint8_t* tgt, const uint8_t* gen_tgt, int H, int W, int use_mix,
                     double p, float* x, uint8_t* m, void* stream) {
  if (!img || !gen || !tgt || !gen_tgt || !x || !m) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(2, H, W)) return rc;
  if (use_mix && !(p >= 0.0 && p <= 1.0)) return MSS_ERR_BAD_ARG;
  const int HW = H * W;
  hipLaunchKernelGGL(load_kernel, dim3(mss_cdiv(HW, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), img, gen, tgt, gen_tgt, HW,
                     use_mix, p, x, m);
  return mss_launch_status();
}

long long mss_aug_stats_ws_doubles(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return (long long)stat_blocks((long long)H * W) * STAT_VALS;
}

int mss_aug_stats_f32(const float* x, int N, int H, int W, double* ws, float* stats, void* stream) {
  if (!x || !ws || !stats) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  const int HW = H * W, nb = stat_blocks(HW);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(stats_partial_kernel, dim3(nb, N), dim3(256), 0, st, x, HW, nb, ws);
  hipLaunchKernelGGL(stats_final_kernel, dim3(N), dim3(256), 0, st, ws, HW, nb, stats);
  return mss_launch_status();
}

int mss_aug_pointwise_f32(float* x, int N, int H, int W, const MssAugPointOps* ops, const float* stats, void* stream) {
  if (!x) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  if (!ops || ops->n < 1 || ops->n > MSS_AUG_MAX_OPS) return MSS_ERR_BAD_ARG;
  for (int k = 0; k < ops->n; ++k) {
    const int kind = ops->kind[k];
    if (kind < MSS_AUG_OP_BRIGHTNESS || kind > MSS_AUG_OP_AUTOCONTRAST) return MSS_ERR_BAD_ARG;
    if ((kind == MSS_AUG_OP_CONTRAST || kind == MSS_AUG_OP_AUTOCONTRAST) && !stats) return MSS_ERR_BAD_ARG;
  }
  const int HW = H * W;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
    hipLaunchKernelGGL(pointwise_kernel<4>, dim3(mss_cdiv(HW / 4, 256), N), dim3(256), 0, st, x, HW, *ops, stats);
  else
    hipLaunchKernelGGL(pointwise_kernel<1>, dim3(mss_cdiv(HW, 256), N), dim3(256), 0, st, x, HW, *ops, stats);
  return mss_launch_status();
}

int mss_aug_equalize_f32(float* x, int N, int H, int W, int* ws, void* stream) {
  if (!x || !ws) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  const int HW = H * W, planes = 3 * N;
  const int nb = mss_cdiv(HW, 256 * 16) < EQ_BLOCKS_MAX ? mss_cdiv(HW, 256 * 16) : EQ_BLOCKS_MAX;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* hist = ws;
  int* lut = ws + (long long)planes * 256;
  if (hipError_t e = hipMemsetAsync(hist, 0, sizeof(int) * 256 * planes, st)) return (int)e;
  hipLaunchKernelGGL(eq_hist_kernel, dim3(nb, planes), dim3(256), 0, st, x, HW, nb, hist);
  hipLaunchKernelGGL(eq_lut_kernel, dim3(1), dim3(256), 0, st, hist, planes, lut);
  hipLaunchKernelGGL(eq_apply_kernel, dim3(mss_cdiv(HW, 256), planes), dim3(256), 0, st, x, HW, lut);
  return mss_launch_status();
}

}  // extern "C"
