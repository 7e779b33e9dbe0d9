// libmss_aug.so, part 2 (include/mss_aug_hip.h): the stages of the Mask2Former input pipeline that look at a pixel's neighbours or
// move pixels -- the 9x9 Gaussian blur and the 3x3 sharpness filter (LDS tile with halo), resize and rotate (bilinear images,
// nearest label maps), the flip / crop window, and the finishing kernel that normalises, pastes the COCO object and writes the
// trainer's batch slots. Nothing here uses MSS_ENV_INT or any symbol of libmss_hip.so.
#include "mss_common.h"
#include "mss_bilinear.h"
#include "../../include/mss_aug_hip.h"

namespace {

__device__ __forceinline__ double pin(double v) { asm volatile("" : "+v"(v)); return v; }   // forbid fma contraction
__device__ __forceinline__ float pinf(float v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

inline int common_check(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return MSS_ERR_BAD_ARG;
  if (N > MSS_AUG_MAX_IMAGES || (long long)H * W > MSS_AUG_MAX_PIXELS) return MSS_ERR_UNSUPPORTED;
  return MSS_OK;
}

// ---- filters: one workgroup = a 16 x 64 output tile of one plane; grid (ceil(W / 64), ceil(H / 16), 3N) ------------------------------
constexpr int TH = 16, TW = 64;
struct Blur9 { float k[9]; };

__device__ __forceinline__ int reflect(int i, int n) {     // torch's reflect padding, pad < n: one reflection is enough
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);                  // unreachable for pad < n; keeps every index in bounds regardless
}

// LDS: the (16 + 8) x (64 + 8) input tile (6912 B) and its row-filtered 24 x 64 intermediate (6144 B)
__global__ __launch_bounds__(256) void blur9_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, Blur9 kw) {
  __shared__ float tile[TH + 8][TW + 8];
  __shared__ float rows[TH + 8][TW];
  const float* xp = x + (long long)blockIdx.z * H * W;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  for (int e = threadIdx.x; e < (TH + 8) * (TW + 8); e += 256) {
    const int ty = e / (TW + 8), tx = e % (TW + 8);
    tile[ty][tx] = xp[(long long)reflect(y0 + ty - 4, H) * W + reflect(x0 + tx - 4, W)];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < (TH + 8) * TW; e += 256) {
    const int ty = e / TW, tx = e % TW;
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) a += kw.k[k] * tile[ty][tx + k];
    rows[ty][tx] = a;
  }
  __syncthreads();
  const int tx = threadIdx.x % TW, ox = x0 + tx;
  if (ox >= W) return;
  float* yp = y + (long long)blockIdx.z * H * W;
#pragma unroll
  for (int r = 0; r < TH / 4; ++r) {
    const int ty = threadIdx.x / TW + 4 * r, oy = y0 + ty;
    if (oy >= H) continue;
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) a += kw.k[k] * rows[ty + k][tx];
    yp[(long long)oy * W + ox] = a;
  }
}

// LDS: the (16 + 2) x (64 + 2) input tile (4752 B). pass != 0: y = x (torchvision returns images of H <= 2 or W <= 2 unchanged)
__global__ __launch_bounds__(256) void sharp3_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, float f, int pass) {
  __shared__ float tile[TH + 2][TW + 2];
  const float* xp = x + (long long)blockIdx.z * H * W;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  for (int e = threadIdx.x; e < (TH + 2) * (TW + 2); e += 256) {
    const int ty = e / (TW + 2), tx = e % (TW + 2);
    int sy = y0 + ty - 1, sx = x0 + tx - 1;                 // the halo outside the image is never used: clamped to stay in bounds
    sy = sy < 0 ? 0 : (sy >= H ? H - 1 : sy);
    sx = sx < 0 ? 0 : (sx >= W ? W - 1 : sx);
    tile[ty][tx] = xp[(long long)sy * W + sx];
  }
  __syncthreads();
  const int tx = threadIdx.x % TW, ox = x0 + tx;
  if (ox >= W) return;
  float* yp = y + (long long)blockIdx.z * H * W;
#pragma unroll
  for (int r = 0; r < TH / 4; ++r) {
    const int ty = threadIdx.x / TW + 4 * r, oy = y0 + ty;
    if (oy >= H) continue;
    const float c = tile[ty + 1][tx + 1];
    float out = c;
    if (!pass) {
      float d = c;
      if (oy >= 1 && oy <= H - 2 && ox >= 1 && ox <= W - 2) {
        const float k1 = 1.f / 13.f, k5 = 5.f / 13.f;
        d = k1 * tile[ty][tx] + k1 * tile[ty][tx + 1] + k1 * tile[ty][tx + 2] + k1 * tile[ty + 1][tx] + k5 * c + k1 * tile[ty + 1][tx + 2] +
            k1 * tile[ty + 2][tx] + k1 * tile[ty + 2][tx + 1] + k1 * tile[ty + 2][tx + 2];
      }
      out = clamp01(f * c + (1.f - f) * d);
    }
    yp[(long long)oy * W + ox] = out;
  }
}

// ---- warps: block (64, 4), grid (ceil(OW / 64), ceil(OH / 4), N); a thread does the three channels and the label of one pixel ------
__global__ __launch_bounds__(256) void resize_kernel(const float* __restrict__ x, const uint8_t* __restrict__ m, int H, int W, int OH,
                                                     int OW, float sh, float sw, float* __restrict__ y, uint8_t* __restrict__ mo) {
  const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (ox >= OW || oy >= OH) return;
  const SrcCoord cy = src_coord(oy, sh, H), cx = src_coord(ox, sw, W);
  const float ly0 = 1.f - cy.l, lx0 = 1.f - cx.l;
  const long long HW = (long long)H * W, OHW = (long long)OH * OW;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* xp = x + ((long long)n * 3 + c) * HW;
    const float v00 = xp[(long long)cy.i0 * W + cx.i0], v01 = xp[(long long)cy.i0 * W + cx.i1];
    const float v10 = xp[(long long)cy.i1 * W + cx.i0], v11 = xp[(long long)cy.i1 * W + cx.i1];
    y[((long long)n * 3 + c) * OHW + (long long)oy * OW + ox] = ly0 * (lx0 * v00 + cx.l * v01) + cy.l * (lx0 * v10 + cx.l * v11);
  }
  // nearest: src = min(floor(dst * scale), in - 1) with the float32 scale in / out
  int ny = (int)floorf((float)oy * sh), nx = (int)floorf((float)ox * sw);
  ny = ny > H - 1 ? H - 1 : ny;
  nx = nx > W - 1 ? W - 1 : nx;
  mo[(long long)n * OHW + (long long)oy * OW + ox] = m[(long long)n * HW + (long long)ny * W + nx];
}

__global__ __launch_bounds__(256) void rotate_kernel(const float* __restrict__ x, const uint8_t* __restrict__ m, int H, int W, float t00,
                                                     float t01, float t10, float t11, float* __restrict__ y, uint8_t* __restrict__ mo) {
  const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (ox >= W || oy >= H) return;
  const float xg = (float)ox - 0.5f * (float)(W - 1), yg = (float)oy - 0.5f * (float)(H - 1);
  const float gx = xg * t00 + yg * t01, gy = xg * t10 + yg * t11;
  const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  // |ix|, |iy| stay far inside the int range for finite theta entries of magnitude <= 1 (checked by the launcher)
  const int x0 = (int)fx, y0 = (int)fy;
  const float lx = ix - fx, ly = iy - fy;
  const bool inx0 = x0 >= 0 && x0 < W, inx1 = x0 + 1 >= 0 && x0 + 1 < W, iny0 = y0 >= 0 && y0 < H, iny1 = y0 + 1 >= 0 && y0 + 1 < H;
  const long long HW = (long long)H * W, o = (long long)oy * W + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* xp = x + ((long long)n * 3 + c) * HW;
    const float v00 = (iny0 && inx0) ? xp[(long long)y0 * W + x0] : 0.f;
    const float v01 = (iny0 && inx1) ? xp[(long long)y0 * W + x0 + 1] : 0.f;
    const float v10 = (iny1 && inx0) ? xp[(long long)(y0 + 1) * W + x0] : 0.f;
    const float v11 = (iny1 && inx1) ? xp[(long long)(y0 + 1) * W + x0 + 1] : 0.f;
    y[((long long)n * 3 + c) * HW + o] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  }
  const float rx = rintf(ix), ry = rintf(iy);              // round half to even, as grid_sample's nearest mode
  const int nx = (int)rx, ny = (int)ry;
  const bool in = nx >= 0 && nx < W && ny >= 0 && ny < H;
  mo[(long long)n * HW + o] = in ? m[(long long)n * HW + (long long)ny * W + nx] : (uint8_t)0;
}

// ---- window: grid (ceil(w / 256), h, N) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_kernel(const float* __restrict__ x, const uint8_t* __restrict__ m, int H, int W, int hflip,
                                                     int vflip, int top, int left, int h, int w, float* __restrict__ y,
                                                     uint8_t* __restrict__ mo) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, n = blockIdx.z;
  if (j >= w) return;
  const int si = vflip ? H - 1 - (top + i) : top + i, sj = hflip ? W - 1 - (left + j) : left + j;
  const long long HW = (long long)H * W, hw = (long long)h * w, s = (long long)si * W + sj, o = (long long)i * w + j;
#pragma unroll
  for (int c = 0; c < 3; ++c) y[((long long)n * 3 + c) * hw + o] = x[((long long)n * 3 + c) * HW + s];
  mo[(long long)n * hw + o] = m[(long long)n * HW + s];
}

// ---- finish: grid (ceil(w / 256), h, 2) ------------------------------------------------------------------------------------------------
struct FinishArgs {
  const float* x; const uint8_t* m;
  int H, W, hflip, vflip, top, left, h, w;
  float mean[3], stdv[3];          // float32(mean), float32(std): what torchvision's Normalize subtracts / divides by
  double mean_d[3], std_d[3];      // the Python floats themselves: what img_utils.normalize() uses on the pasted object
  const float* obj_img; const uint8_t* obj_mask; int OH, OW, paste, g[6];
  int B, b; float* out_img; long long* out_tgt;
};
__global__ __launch_bounds__(256) void finish_kernel(FinishArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, n = blockIdx.z;
  if (j >= a.w) return;
  const int si = a.vflip ? a.H - 1 - (a.top + i) : a.top + i, sj = a.hflip ? a.W - 1 - (a.left + j) : a.left + j;
  const long long HW = (long long)a.H * a.W, hw = (long long)a.h * a.w, s = (long long)si * a.W + sj, o = (long long)i * a.w + j;
  const long long slot = n == 0 ? a.b : a.B + a.b;
  bool pasted = false;
  float pv[3] = {0.f, 0.f, 0.f};
  uint8_t pm = 0;
  if (a.paste && n == 0) {
    // object region rows [y1, y1 + bh) x cols [x1, x1 + bw) of the object, placed at (h0, w0) of the crop (the arithmetic of csrc/data.hip)
    const int y1 = a.g[0], x1 = a.g[1], bh = a.g[2], bw = a.g[3], h0 = a.g[4], w0 = a.g[5];
    const int oy = i - h0, ox = j - w0;
    if (bh > 0 && oy >= 0 && oy < bh && ox >= 0 && ox < bw) {
      const long long oi = (long long)(y1 + oy) * a.OW + x1 + ox;
      pm = a.obj_mask[oi];
      if (pm != 0 && pm != 255) {
        pasted = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          // normalize() of img_utils.py:355-361: float32 / 255.0 stays float32, "- mean" and "/ std" promote to float64
          const float v = pinf(a.obj_img[oi * 3 + c] / 255.0f);
          pv[c] = (float)(pin((double)v - a.mean_d[c]) / a.std_d[c]);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = a.x[((long long)n * 3 + c) * HW + s];
    const float nv = pinf(v - a.mean[c]) / a.stdv[c];      // sub_(mean).div_(std): separately rounded float32 operations
    a.out_img[(slot * 3 + c) * hw + o] = pasted ? pv[c] : nv;
  }
  a.out_tgt[slot * hw + o] = pasted ? (long long)pm : (long long)a.m[(long long)n * HW + s];
}

inline bool window_ok(int H, int W, int top, int left, int h, int w) {
  return top >= 0 && left >= 0 && h <= H && w <= W && top <= H - h && left <= W - w;
}

}  // namespace

extern "C" {

int mss_aug_blur9_f32(const float* x, float* y, int N, int H, int W, const float* k9, void* stream) {
  if (!x || !y) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  if (!k9 || x == y) return MSS_ERR_BAD_ARG;
  if (H < 5 || W < 5 || H > 65535 * TH) return MSS_ERR_UNSUPPORTED;
  Blur9 kw;
  for (int k = 0; k < 9; ++k) kw.k[k] = k9[k];
  hipLaunchKernelGGL(blur9_kernel, dim3(mss_cdiv(W, TW), mss_cdiv(H, TH), 3 * N), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, H,
                     W, kw);
  return mss_launch_status();
}

int mss_aug_sharpness_f32(const float* x, float* y, int N, int H, int W, float factor, void* stream) {
  if (!x || !y) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  if (x == y) return MSS_ERR_BAD_ARG;
  if (H > 65535 * TH) return MSS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sharp3_kernel, dim3(mss_cdiv(W, TW), mss_cdiv(H, TH), 3 * N), dim3(256), 0, static_cast<hipStream_t>(stream), x, y,
                     H, W, factor, (H <= 2 || W <= 2) ? 1 : 0);
  return mss_launch_status();
}

int mss_aug_resize_f32(const float* x, const uint8_t* m, int N, int H, int W, int OH, int OW, float* y, uint8_t* mo, void* stream) {
  if (!x || !m || !y || !mo) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  if (OH <= 0 || OW <= 0) return MSS_ERR_BAD_ARG;
  if ((long long)OH * OW > MSS_AUG_MAX_PIXELS || OH > 65535 * 4) return MSS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(resize_kernel, dim3(mss_cdiv(OW, 64), mss_cdiv(OH, 4), N), dim3(64, 4), 0, static_cast<hipStream_t>(stream), x, m, H,
                     W, OH, OW, mss_bilinear_scale(H, OH), mss_bilinear_scale(W, OW), y, mo);
  return mss_launch_status();
}

int mss_aug_rotate_f32(const float* x, const uint8_t* m, int N, int H, int W, float c, float s, float* y, uint8_t* mo, void* stream) {
  if (!x || !m || !y || !mo) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  if (!(c >= -1.f && c <= 1.f) || !(s >= -1.f && s <= 1.f)) return MSS_ERR_BAD_ARG;      // also refuses NaN
  if (H > 65535 * 4) return MSS_ERR_UNSUPPORTED;
  // rescaled theta of torchvision's _gen_affine_grid: theta^T / (0.5 W, 0.5 H), in float32
  const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
  hipLaunchKernelGGL(rotate_kernel, dim3(mss_cdiv(W, 64), mss_cdiv(H, 4), N), dim3(64, 4), 0, static_cast<hipStream_t>(stream), x, m, H, W,
                     c / hw, s / hw, -s / hh, c / hh, y, mo);
  return mss_launch_status();
}

int mss_aug_window_f32(const float* x, const uint8_t* m, int N, int H, int W, int hflip, int vflip, int top, int left, int h, int w,
                       float* y, uint8_t* mo, void* stream) {
  if (!x || !m || !y || !mo) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(N, H, W)) return rc;
  if (h <= 0 || w <= 0 || !window_ok(H, W, top, left, h, w)) return MSS_ERR_BAD_ARG;
  if (h > 65535) return MSS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(window_kernel, dim3(mss_cdiv(w, 256), h, N), dim3(256), 0, static_cast<hipStream_t>(stream), x, m, H, W, hflip, vflip,
                     top, left, h, w, y, mo);
  return mss_launch_status();
}

int mss_aug_finish_f32(const float* x, const uint8_t* m, int H, int W, int hflip, int vflip, int top, int left, int h, int w,
                       const double* mean3, const double* std3, const float* obj_img, const uint8_t* obj_mask, int OH, int OW,
                       const int* geom6, int B, int b, float* out_img, long long* out_tgt, void* stream) {
  if (!x || !m || !out_img || !out_tgt) return MSS_ERR_BAD_ARG;
  if (const int rc = common_check(2, H, W)) return rc;
  if (!mean3 || !std3) return MSS_ERR_BAD_ARG;
  if (h <= 0 || w <= 0 || !window_ok(H, W, top, left, h, w)) return MSS_ERR_BAD_ARG;
  if (B <= 0 || b < 0 || b >= B) return MSS_ERR_BAD_ARG;
  if (geom6) {
    if (!obj_img || !obj_mask || OH <= 0 || OW <= 0) return MSS_ERR_BAD_ARG;
    for (int k = 0; k < 6; ++k) if (geom6[k] < 0) return MSS_ERR_BAD_ARG;
    if (geom6[2] > OH - geom6[0] || geom6[3] > OW - geom6[1]) return MSS_ERR_BAD_ARG;
  }
  if (h > 65535) return MSS_ERR_UNSUPPORTED;
  FinishArgs a;
  a.x = x; a.m = m; a.H = H; a.W = W; a.hflip = hflip; a.vflip = vflip; a.top = top; a.left = left; a.h = h; a.w = w;
  for (int c = 0; c < 3; ++c) {
    a.mean_d[c] = mean3[c]; a.std_d[c] = std3[c];
    a.mean[c] = (float)mean3[c]; a.stdv[c] = (float)std3[c];
  }
  a.obj_img = obj_img; a.obj_mask = obj_mask; a.OH = OH; a.OW = OW; a.paste = geom6 ? 1 : 0;
  for (int k = 0; k < 6; ++k) a.g[k] = geom6 ? geom6[k] : 0;
  a.B = B; a.b = b; a.out_img = out_img; a.out_tgt = out_tgt;
  hipLaunchKernelGGL(finish_kernel, dim3(mss_cdiv(w, 256), h, 2), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return mss_launch_status();
}

}  // extern "C"
