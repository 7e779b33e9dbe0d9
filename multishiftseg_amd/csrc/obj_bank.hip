// The resident COCO-object bank of the anomaly mix (include/mss_obj_hip.h): what random_scale and the bounding-box
// cut of mix_func do per sample on the host (lib/utils/img_utils.py:345-352, :379-406), over objects that stay in HBM as uint8.
//   obj_bbox_kernel      one workgroup per (object, scaled size): every thread walks destination pixels of the NEAREST-resized mask,
//                        keeps integer min / max of the rows and columns whose source byte is valid (neither 0 nor 255); wave
//                        shuffles, four LDS words per bound, thread 0 writes (y1, x1, y2, x2). Integer reductions only.
//   obj_rescale_kernel   grid (tiles of 64 columns, tiles of 16 rows, B): a workgroup whose tile lies outside its sample's window
//                        leaves at once. 64 + 16 threads compute the (index, index, fraction, nearest index) of the tile's columns
//                        and rows in double (csrc/mss_cv_resize.h) into LDS; then waves 0-2 own ONE OUTPUT FLOAT per lane (192
//                        consecutive floats of a row = 768 contiguous bytes per row and workgroup, dword stores) and walk the 16
//                        rows: four uint8 taps, horizontal pass, vertical pass, every product and sum rounded to float32 on its
//                        own (no fused multiply-add); wave 3 owns one mask byte per lane (64 contiguous bytes per row).
// HBM per window pixel: 12 B + 1 B written; the taps (12 image bytes, 1 mask byte) come from the caches for every scale <= 1.
// No float atomics, no memset, no scratch, no device-to-host copy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mss_cv_resize.h"
#include "../../include/mss_obj_hip.h"

namespace {

constexpr int OB_T = 256;              // threads of every workgroup here
constexpr int OB_TPX = 64;             // columns of one rescale tile: 192 floats = waves 0-2, 64 mask bytes = wave 3
constexpr int OB_TH = 16;              // rows of one rescale tile

inline int ob_launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MSS_OK : (int)e;
}

// a rounded float32 that the compiler may not fuse into the operation that follows
__device__ __forceinline__ float ob_fl(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// what both kernels require of (off, H, W, sh, sw) before they touch the bank
__device__ __forceinline__ bool ob_source_ok(int off, int H, int W, int sh, int sw, long long bank_pixels) {
  return off >= 0 && H >= 1 && W >= 1 && sh >= 1 && sw >= 1 && (long long)off + (long long)H * W <= bank_pixels &&
         (long long)sh * sw <= MSS_OBJ_MAX_PIXELS;
}

__device__ __forceinline__ int ob_wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ int ob_wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// grid n
__global__ __launch_bounds__(OB_T) void obj_bbox_kernel(const uint8_t* __restrict__ bank_mask, long long bank_pixels, const int* __restrict__ jobs,
                                                        int* __restrict__ boxes) {
  __shared__ int red[4][OB_T / 64];
  const int* j = jobs + (size_t)blockIdx.x * MSS_OBJ_BBOX_JOB_INTS;
  const int off = j[0], H = j[1], W = j[2], sh = j[3], sw = j[4];
  int* box = boxes + (size_t)blockIdx.x * 4;
  if (!ob_source_ok(off, H, W, sh, sw, bank_pixels)) {          // the same in every thread
    if (threadIdx.x < 4) box[threadIdx.x] = 0;
    return;
  }
  const double scale_y = cv_scale(H, sh), scale_x = cv_scale(W, sw);
  const uint8_t* m = bank_mask + off;
  const unsigned n = (unsigned)sh * (unsigned)sw;               // <= 2^31 - 1
  int y_lo = 0x7fffffff, x_lo = 0x7fffffff, y_hi = -1, x_hi = -1;
  for (unsigned e = threadIdx.x; e < n; e += OB_T) {
    const int dy = (int)(e / (unsigned)sw), dx = (int)(e - (unsigned)dy * (unsigned)sw);
    const uint8_t v = m[(size_t)cv_nearest(dy, scale_y, H) * W + cv_nearest(dx, scale_x, W)];
    if (v != 0 && v != 255) {
      y_lo = min(y_lo, dy);
      y_hi = max(y_hi, dy);
      x_lo = min(x_lo, dx);
      x_hi = max(x_hi, dx);
    }
  }
  y_lo = ob_wave_min(y_lo);
  x_lo = ob_wave_min(x_lo);
  y_hi = ob_wave_max(y_hi);
  x_hi = ob_wave_max(x_hi);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = y_lo;
    red[1][wave] = x_lo;
    red[2][wave] = y_hi;
    red[3][wave] = x_hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < OB_T / 64; ++w) {
      y_lo = min(y_lo, red[0][w]);
      x_lo = min(x_lo, red[1][w]);
      y_hi = max(y_hi, red[2][w]);
      x_hi = max(x_hi, red[3][w]);
    }
    const bool any = y_hi >= 0;
    box[0] = any ? y_lo : 0;
    box[1] = any ? x_lo : 0;
    box[2] = any ? y_hi + 1 : 0;
    box[3] = any ? x_hi + 1 : 0;
  }
}

// grid (ceil(OWmax / OB_TPX), ceil(OHmax / OB_TH), B)
__global__ __launch_bounds__(OB_T) void obj_rescale_kernel(const uint8_t* __restrict__ bank_img, const uint8_t* __restrict__ bank_mask,
                                                           long long bank_pixels, const int* __restrict__ jobs, int OHmax, int OWmax,
                                                           float* __restrict__ out_img, uint8_t* __restrict__ out_mask) {
  __shared__ int col_i0[OB_TPX], col_i1[OB_TPX], col_n[OB_TPX];
  __shared__ float col_f[OB_TPX];
  __shared__ int row_i0[OB_TH], row_i1[OB_TH], row_n[OB_TH];
  __shared__ float row_f[OB_TH];
  const int b = blockIdx.z;
  const int* j = jobs + (size_t)b * MSS_OBJ_RESCALE_JOB_INTS;
  const int off = j[0], H = j[1], W = j[2], sh = j[3], sw = j[4], y1 = j[5], x1 = j[6], bh = j[7], bw = j[8];
  const int tx0 = blockIdx.x * OB_TPX, ty0 = blockIdx.y * OB_TH;
  // every condition here is the same in all threads of the workgroup: nobody waits at the barrier below for one that left
  if (bh <= 0 || bw <= 0 || tx0 >= bw || ty0 >= bh) return;
  if (!ob_source_ok(off, H, W, sh, sw, bank_pixels) || y1 < 0 || x1 < 0 || bh > sh - y1 || bw > sw - x1 || bh > OHmax || bw > OWmax) return;
  const int t = threadIdx.x;
  const int ncols = min(OB_TPX, bw - tx0), nrows = min(OB_TH, bh - ty0);
  if (t < ncols) {
    const double scale = cv_scale(W, sw);
    const CvTap tap = cv_linear(x1 + tx0 + t, scale, W);
    col_i0[t] = tap.i0;
    col_i1[t] = tap.i1;
    col_f[t] = tap.f;
    col_n[t] = cv_nearest(x1 + tx0 + t, scale, W);
  } else if (t >= OB_TPX && t - OB_TPX < nrows) {
    const int r = t - OB_TPX;
    const double scale = cv_scale(H, sh);
    const CvTap tap = cv_linear(y1 + ty0 + r, scale, H);
    row_i0[r] = tap.i0;
    row_i1[r] = tap.i1;
    row_f[r] = tap.f;
    row_n[r] = cv_nearest(y1 + ty0 + r, scale, H);
  }
  __syncthreads();
  const size_t slot_px = ((size_t)b * OHmax + ty0) * OWmax + tx0;        // pixel (ty0, tx0) of slot b
  if (t < 3 * OB_TPX) {
    const int px = t / 3, c = t - 3 * px;
    if (px >= ncols) return;
    const float a1 = col_f[px], a0 = 1.0f - a1;
    const uint8_t* src = bank_img + (size_t)off * 3 + c;
    const size_t c0 = (size_t)col_i0[px] * 3, c1 = (size_t)col_i1[px] * 3, row_bytes = (size_t)W * 3;
    float* dst = out_img + slot_px * 3 + t;
    for (int r = 0; r < nrows; ++r) {
      const float b1 = row_f[r], b0 = 1.0f - b1;
      const uint8_t* p0 = src + (size_t)row_i0[r] * row_bytes;
      const uint8_t* p1 = src + (size_t)row_i1[r] * row_bytes;
      const float s00 = (float)p0[c0], s01 = (float)p0[c1], s10 = (float)p1[c0], s11 = (float)p1[c1];
      const float h0 = ob_fl(ob_fl(s00 * a0) + ob_fl(s01 * a1));
      const float h1 = ob_fl(ob_fl(s10 * a0) + ob_fl(s11 * a1));
      dst[(size_t)r * OWmax * 3] = ob_fl(h0 * b0) + ob_fl(h1 * b1);
    }
  } else {
    const int px = t - 3 * OB_TPX;
    if (px >= ncols) return;
    const uint8_t* src = bank_mask + (size_t)off + col_n[px];
    uint8_t* dst = out_mask + slot_px + px;
    for (int r = 0; r < nrows; ++r) dst[(size_t)r * OWmax] = src[(size_t)row_n[r] * W];
  }
}

inline int ob_cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

extern "C" {

int mss_obj_abi_version(void) { return MSS_OBJ_ABI_VERSION; }

int mss_obj_bbox_u8(const uint8_t* bank_mask, long long bank_pixels, const int* jobs, int n, int* boxes, void* stream) {
  if (!bank_mask || !jobs || !boxes) return MSS_ERR_BAD_ARG;
  if (bank_pixels < 1 || n < 1) return MSS_ERR_BAD_ARG;
  if (bank_pixels > MSS_OBJ_MAX_PIXELS || n > MSS_OBJ_MAX_BBOX_JOBS) return MSS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(obj_bbox_kernel, dim3(n), dim3(OB_T), 0, static_cast<hipStream_t>(stream), bank_mask, bank_pixels, jobs, boxes);
  return ob_launch_status();
}

int mss_obj_rescale_f32(const uint8_t* bank_img, const uint8_t* bank_mask, long long bank_pixels, const int* jobs, int B, int OHmax,
                        int OWmax, float* out_img, uint8_t* out_mask, void* stream) {
  if (!bank_img || !bank_mask || !jobs || !out_img || !out_mask) return MSS_ERR_BAD_ARG;
  if (bank_pixels < 1 || B < 1 || OHmax < 1 || OWmax < 1) return MSS_ERR_BAD_ARG;
  if (bank_pixels > MSS_OBJ_MAX_PIXELS || B > MSS_OBJ_MAX_BATCH || OHmax > MSS_OBJ_MAX_ROWS ||
      (long long)B * OHmax > MSS_OBJ_MAX_PIXELS / OWmax)          // B OHmax OWmax > MSS_OBJ_MAX_PIXELS, without overflow
    return MSS_ERR_UNSUPPORTED;
  const dim3 grid(ob_cdiv(OWmax, OB_TPX), ob_cdiv(OHmax, OB_TH), B);
  hipLaunchKernelGGL(obj_rescale_kernel, grid, dim3(OB_T), 0, static_cast<hipStream_t>(stream), bank_img, bank_mask, bank_pixels, jobs,
                     OHmax, OWmax, out_img, out_mask);
  return ob_launch_status();
}

}  // extern "C"
