// The stem of the Mask2Former ResNet-50 backbone: conv 7x7, stride 2, padding 3, 3 -> 64 channels, bias-free, with the folded
// eval-mode norm and the ReLU in the epilogue (detectron2 BasicStem: conv1 -> norm -> relu; the max-pool behind it stays
// mss_maxpool3s2_nhwc_f32). Reached through mss_conv2d_forward_f32 (conv_igemm.hip), route label 5.
//
// The image arrives as NHWC with the three colour channels plus ONE ZERO channel (mss_nchw_to_nhwc_pad_f32, Cp = 4), so a pixel is
// one 16-byte vector and one filter tap (r, s) is exactly one K = 4 step of v_mfma_f32_16x16x4_f32: 49 MFMAs per 16 output pixels x
// 16 output channels, a quarter of the multiplies spent on the zero channel (2 * 196 * 64 instead of 2 * 147 * 64 FLOP per pixel).
//
//  * The WEIGHTS are the MFMA's first operand (A[i = channel][k = input channel]), the pixels the second (B[k][j = pixel]): the
//    accumulator of lane l then holds pixel l & 15 and the four CONSECUTIVE channels 4 (l >> 4) .. + 3 -- one 16-byte store per lane.
//  * A workgroup (4 waves) owns a tile of 8 x 32 output pixels; wave v owns output channels 16 v .. 16 v + 15 of the whole tile and
//    keeps its 49 taps x 16 channels x 4 input channels in 49 registers per lane for the life of the workgroup: the 50 KB of weights
//    never touch LDS.
//  * The input patch of the tile, (2 * 8 + 5) x (2 * 32 + 5) pixels of 16 bytes, zero outside the image, is staged in LDS once
//    (23 520 B), its columns split by parity: a wave's B operand of tap (r, s) for 16 neighbouring output pixels (input columns
//    2 j + s) is then 64 consecutive floats -- every ds_read_b32 is conflict-free and its address is the lane's base plus an
//    immediate.
//  * Four 16-pixel groups (two output rows x two column halves) run as four independent accumulators, which covers the 40-cycle
//    dependent latency of the instruction; a group whose pixels all lie outside the output is still multiplied (the patch is
//    zero-filled, never out of bounds) but not stored, except that trailing row pairs past the output are skipped.
//  * The reduction order per output value is tap 0 .. 48, input channel 0 .. 3 inside a tap: a plain fmaf chain.
#include "mss_common.h"
#include "../../include/mss_hip.h"

int mss_stem7_launch(MssConvArgs p, void* stream);

namespace {

constexpr int S7_TH = 8, S7_TW = 32;                        // output pixels per workgroup
constexpr int S7_PH = 2 * S7_TH + 5, S7_PW = 2 * S7_TW + 5; // input patch: 21 x 69 pixels
constexpr int S7_HC = (S7_PW + 1) / 2;                      // 35 columns per parity
constexpr int S7_TAPS = 49;
static_assert(MSS_STEM7_K == 4 * 16, "four waves of 16 output channels each (fwd_route.h asks for K == MSS_STEM7_K)");

__global__ __launch_bounds__(256, 2) void stem7_conv_kernel(MssConvArgs p, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) float patch[S7_PH * 2 * S7_HC * 4];   // [row][column parity][column / 2][4 channels]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int cb = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave's block of 16 output channels
  const int j = lane & 15, q = lane >> 4;                   // pixel of a group / input channel (operands), channel quad (accumulator)

  const int v = mss_xcd_remap(blockIdx.x, gridDim.x);
  const int tx = v % tiles_x, ty = (v / tiles_x) % tiles_y, n = v / (tiles_x * tiles_y);
  const int oy0 = ty * S7_TH, ox0 = tx * S7_TW;

  // ---- A operand: w[tap][channel 16 cb + j][input channel q], 49 registers
  float wreg[S7_TAPS];
  {
    const float* wp = p.w + (size_t)(cb * 16 + j) * 4 + q;
#pragma unroll
    for (int t = 0; t < S7_TAPS; ++t) wreg[t] = wp[(size_t)t * p.Kpad * 4];
  }

  // ---- the input patch -> LDS, zero outside the image
  {
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
    const float* img = p.x + (size_t)n * p.H * p.W * 4;
    for (int i = tid; i < S7_PH * S7_PW; i += 256) {
      const int py = i / S7_PW, px = i - py * S7_PW;
      const int iy = iy0 + py, ix = ix0 + px;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
        val = *reinterpret_cast<const f32x4*>(img + ((size_t)iy * p.W + ix) * 4);
      *reinterpret_cast<f32x4*>(&patch[((py * 2 + (px & 1)) * S7_HC + (px >> 1)) * 4]) = val;
    }
  }
  __syncthreads();

  // ---- epilogue constants of this lane's four channels
  const int ch = cb * 16 + q * 4;
  f32x4 osc = {1.f, 1.f, 1.f, 1.f}, osh = {0.f, 0.f, 0.f, 0.f};
  if (p.out_scale) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { osc[r] = p.out_scale[ch + r]; osh[r] = p.out_shift[ch + r]; }
  }
  const float floor_v = p.out_relu ? 0.f : -__builtin_huge_valf();
  float* yimg = p.y + (size_t)n * p.OH * p.OW * p.ldy + ch;

  // ---- two output rows x two column halves per pass
  const float* bbase = &patch[j * 4 + q];
  for (int rp = 0; rp < S7_TH / 2; ++rp) {
    const int oy = oy0 + 2 * rp;
    if (oy >= p.OH) break;                                  // workgroup-uniform
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int g = 0; g < 2; ++g) acc[a][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* brow = bbase + (size_t)(4 * rp) * (2 * S7_HC * 4);   // patch row 2 * (2 rp) of output row 2 rp
#pragma unroll
    for (int t = 0; t < S7_TAPS; ++t) {
      const int r = t / 7, s = t % 7;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const float b = brow[(((2 * a + r) * 2 + (s & 1)) * S7_HC + 16 * g + (s >> 1)) * 4];
          acc[a][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[t], b, acc[a][g], 0, 0, 0);
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int yy = oy + a, xx = ox0 + 16 * g + j;
        f32x4 val = acc[a][g] * osc + osh;
#pragma unroll
        for (int r = 0; r < 4; ++r) val[r] = fmaxf(val[r], floor_v);
        if (yy < p.OH && xx < p.OW) *reinterpret_cast<f32x4*>(yimg + ((size_t)yy * p.OW + xx) * p.ldy) = val;
      }
  }
}

}  // namespace

// Which calls get here: mss_stem7_eligible (fwd_route.h).
int mss_stem7_launch(MssConvArgs p, void* stream) {
  if (p.N == 0) return MSS_OK;
  const int tiles_x = mss_cdiv(p.OW, S7_TW), tiles_y = mss_cdiv(p.OH, S7_TH);
  const long long grid = (long long)tiles_x * tiles_y * p.N;
  if (grid >= (1ll << 31)) return MSS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(stem7_conv_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), p, tiles_x, tiles_y);
  return mss_launch_status();
}
