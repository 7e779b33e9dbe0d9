// Masked cross-attention of the Mask2Former GMA transformer decoder (mask2former_transformer_decoder.py:75-121, 438-542):
// few queries (<= 128), many keys (up to 128 x 256), 8 heads of 32 channels, a foreground and a background attention with
// opposite masks.
//
// The reference materialises per attention a bool mask [B*8, Q, HW] (bilinear resample + sigmoid + compare, repeated over the
// heads), an fp32 weight tensor of that shape, and un-masks fully masked rows through a host-visible torch.where. Here
//   * m2f_attn_mask_bits_kernel resamples the pixel-major low-resolution mask logits [B, hm*wm, ldq] to the level size and
//     writes, per image and key, two bit rows over the queries (neg: logit < 0, pos: logit > 0; sigmoid(x) < 0.5 <=> x < 0, no
//     sigmoid is evaluated) plus one "some key is allowed" bit per (image, attention, query) (integer atomic OR: order-free);
//   * m2f_masked_attention_kernel is a streaming softmax: a lane owns one query (its 32 q values, running maximum, denominator
//     and 32 numerators live in registers), the key / value rows of a head are wave-uniform 128-byte segments read once, the
//     bit rows are applied to the scores and a query without any allowed key ignores its mask (the reference's rescue rule);
//   * the key range is split into chunks so that 8 heads x 2 attentions x B fill the chip; a chunk leaves (numerator, maximum,
//     denominator) in a workspace and m2f_attn_merge_kernel folds the chunks in fixed order -- no float atomics, bit-reproducible.
#include "mss_common.h"
#include "mss_bilinear.h"
#include "../../include/mss_hip.h"

namespace {

constexpr int HD = 32;        // head dimension
constexpr int NH = 8;         // heads
constexpr int KB = 8;         // keys per online-softmax step (one rescale of the accumulators per KB keys)
constexpr int WSROWS = HD + 2;  // workspace rows of one (chunk, head): 32 numerators, maximum (log2 domain), denominator

// SrcCoord / src_coord: F.interpolate(mode="bilinear", align_corners=False), mss_bilinear.h

// bits [B][2][h*w][W] (W = ceil(Q/32) words; bit q of a row set = query q may NOT attend to that key), allowed [B][2][W]
// (zeroed before the launch; bit q set = query q has at least one allowed key). A wave takes one key at a time: lane = query.
__global__ __launch_bounds__(256) void m2f_attn_mask_bits_kernel(const float* __restrict__ logit, int Q, int ldq, int hm, int wm,
                                                                 int h, int w, float sy, float sx, int keys_per_block,
                                                                 uint32_t* __restrict__ bits, uint32_t* __restrict__ allowed) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = (Q + 31) >> 5;
  const int HW = h * w;
  const int k_begin = blockIdx.x * keys_per_block, k_end = min(HW, k_begin + keys_per_block);
  unsigned long long some_fg[2] = {0ull, 0ull}, some_bg[2] = {0ull, 0ull};
  for (int key = k_begin + wave; key < k_end; key += 4) {
    const int oy = key / w, ox = key - oy * w;
    const SrcCoord cy = src_coord(oy, sy, hm), cx = src_coord(ox, sx, wm);
    const float* img = logit + (long long)b * hm * wm * ldq;
    const float* r00 = img + ((long long)cy.i0 * wm + cx.i0) * ldq;
    const float* r01 = img + ((long long)cy.i0 * wm + cx.i1) * ldq;
    const float* r10 = img + ((long long)cy.i1 * wm + cx.i0) * ldq;
    const float* r11 = img + ((long long)cy.i1 * wm + cx.i1) * ldq;
    const float hy0 = 1.f - cy.l, hy1 = cy.l, wx0 = 1.f - cx.l, wx1 = cx.l;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (64 * j >= Q) break;
      const int q = lane + 64 * j;
      const bool in = q < Q;
      float v = 0.f;
      // same association as ATen's upsample_bilinear2d: h0 * (w0 v00 + w1 v01) + h1 * (w0 v10 + w1 v11)
      if (in) v = hy0 * (wx0 * r00[q] + wx1 * r01[q]) + hy1 * (wx0 * r10[q] + wx1 * r11[q]);
      const unsigned long long neg = __ballot(in && v < 0.f), pos = __ballot(in && v > 0.f);
      some_fg[j] |= ~neg;
      some_bg[j] |= ~pos;
      const int word = 2 * j + lane;
      if (lane < 2 && word < W) {
        bits[((long long)(b * 2 + 0) * HW + key) * W + word] = (uint32_t)(neg >> (32 * lane));
        bits[((long long)(b * 2 + 1) * HW + key) * W + word] = (uint32_t)(pos >> (32 * lane));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int word = 2 * j + lane;
    if (lane < 2 && word < W) {
      const uint32_t fg = (uint32_t)(some_fg[j] >> (32 * lane)), bg = (uint32_t)(some_bg[j] >> (32 * lane));
      if (fg) atomicOr(&allowed[(b * 2 + 0) * W + word], fg);
      if (bg) atomicOr(&allowed[(b * 2 + 1) * W + word], bg);
    }
  }
}

// grid (chunks, 8 * A, B), block 64 * ceil(Q / 64). q [B*Q, ldq], k / v [B*NK, ldk / ldv], out [B*Q, ldo]; attention a and head hd
// use columns a * 256 + hd * 32 ... + 31 of each. scale_log2e = softmax scale * log2(e), folded into q (the exponentials are
// exp2). DIRECT (chunks == 1): normalise and store; else leave the chunk's partial state in ws [slot][34][QS].
template <bool MASKED, bool DIRECT>
__global__ __launch_bounds__(128) void m2f_masked_attention_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                                   const float* __restrict__ v, int ldv, const uint32_t* __restrict__ bits,
                                                                   const uint32_t* __restrict__ allowed, int Q, int NK, int A,
                                                                   float scale_log2e, int keys_per_chunk, float* __restrict__ ws,
                                                                   float* __restrict__ out, int ldo) {
  const int c = blockIdx.x, a = blockIdx.y >> 3, hd = blockIdx.y & 7, b = blockIdx.z;
  const int col = a * (NH * HD) + hd * HD;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qi = wave * 64 + lane;
  const int W = (Q + 31) >> 5;
  const float NEG_INF = -__builtin_huge_valf();
  float qr[HD], acc[HD];
  {
    const float* qp = q + ((long long)b * Q + min(qi, Q - 1)) * ldq + col;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(qp + d);
      qr[d] = t.x * scale_log2e; qr[d + 1] = t.y * scale_log2e; qr[d + 2] = t.z * scale_log2e; qr[d + 3] = t.w * scale_log2e;
    }
  }
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
  float m = NEG_INF, l = 0.f;
  const int k0 = c * keys_per_chunk, k1 = min(NK, k0 + keys_per_chunk);
  const float* kb = k + (long long)b * NK * ldk + col;
  const float* vb = v + (long long)b * NK * ldv + col;
  // the two mask words that hold this wave's 64 queries (wave-uniform addresses); a lane picks its word and bit
  const int w0 = 2 * wave, w1 = min(2 * wave + 1, W - 1);
  const uint32_t* brow = nullptr;
  uint32_t live = 0u;          // this lane's "mask applies" word: a query with no allowed key ignores its mask
  const int sh = lane & 31;
  const bool hi = (lane & 32) != 0;
  if (MASKED) {
    brow = bits + (long long)(b * A + a) * NK * W;
    const uint32_t al0 = allowed[(b * A + a) * W + w0], al1 = allowed[(b * A + a) * W + w1];
    live = hi ? al1 : al0;
  }
  for (int kk = k0; kk < k1; kk += KB) {
    float s[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      const int key = min(kk + j, k1 - 1);
      const float* kr = kb + (long long)key * ldk;
      float dot = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) dot = __builtin_fmaf(qr[d], kr[d], dot);
      bool masked = kk + j >= k1;
      if (MASKED) {
        const uint32_t b0 = brow[(long long)key * W + w0], b1 = brow[(long long)key * W + w1];
        masked = masked || ((((hi ? b1 : b0) & live) >> sh) & 1u);
      }
      s[j] = masked ? NEG_INF : dot;
    }
    float bm = s[0];
#pragma unroll
    for (int j = 1; j < KB; ++j) bm = fmaxf(bm, s[j]);
    const float mn = fmaxf(m, bm);
    const float mref = mn == NEG_INF ? 0.f : mn;      // nothing allowed so far: every exponential below is exp2(-inf) = 0
    const float alpha = exp2f(m - mref);
    l *= alpha;
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] *= alpha;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      const int key = min(kk + j, k1 - 1);
      const float* vr = vb + (long long)key * ldv;
      const float p = exp2f(s[j] - mref);
      l += p;
#pragma unroll
      for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(p, vr[d], acc[d]);
    }
    m = mn;
  }
  if (qi >= Q) return;
  if (DIRECT) {
    const float inv = 1.f / l;
    float* op = out + ((long long)b * Q + qi) * ldo + col;
#pragma unroll
    for (int d = 0; d < HD; d += 4) *reinterpret_cast<f32x4*>(op + d) = f32x4{acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv};
  } else {
    const int QS = blockDim.x;
    const long long slot = ((long long)(b * A + a) * NH + hd) * gridDim.x + c;
    float* wp = ws + slot * WSROWS * QS + qi;
#pragma unroll
    for (int d = 0; d < HD; ++d) wp[d * QS] = acc[d];
    wp[HD * QS] = m;
    wp[(HD + 1) * QS] = l;
  }
}

// one thread per (image, attention, head, channel, query): folds the chunks in index order. A chunk in which the query saw no
// allowed key has maximum -inf and enters with weight 0 (its numerators and denominator are 0 as well).
__global__ __launch_bounds__(256) void m2f_attn_merge_kernel(const float* __restrict__ ws, int B, int Q, int QS, int A, int chunks,
                                                             float* __restrict__ out, int ldo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * A * NH * HD * QS;
  if (i >= total) return;
  const int qi = (int)(i % QS);
  const int d = (int)((i / QS) % HD);
  const long long bah = i / ((long long)QS * HD);
  if (qi >= Q) return;
  const int hd = (int)(bah % NH), a = (int)((bah / NH) % A), b = (int)(bah / ((long long)NH * A));
  const float NEG_INF = -__builtin_huge_valf();
  const float* base = ws + bah * chunks * WSROWS * QS + qi;
  float M = NEG_INF;
  for (int c = 0; c < chunks; ++c) M = fmaxf(M, base[((long long)c * WSROWS + HD) * QS]);
  float num = 0.f, den = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const float* p = base + (long long)c * WSROWS * QS;
    const float mc = p[HD * QS];
    const float wgt = mc == NEG_INF ? 0.f : exp2f(mc - M);
    num = __builtin_fmaf(wgt, p[d * QS], num);
    den = __builtin_fmaf(wgt, p[(HD + 1) * QS], den);
  }
  out[((long long)b * Q + qi) * ldo + a * (NH * HD) + hd * HD + d] = num / den;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the chunk geometry both the launcher and the workspace query use: keys per chunk (a multiple of KB) and the chunk count
inline void chunk_plan(int NK, int chunks, int* keys_per_chunk, int* nchunks) {
  int kpc = mss_cdiv(NK, chunks);
  kpc = (kpc + KB - 1) / KB * KB;
  *keys_per_chunk = kpc;
  *nchunks = mss_cdiv(NK, kpc);
}

}  // namespace

extern "C" {

int mss_m2f_attn_mask_bits_f32(const float* logit, int B, int Q, int ldq, int hm, int wm, int h, int w, uint32_t* bits,
                               uint32_t* allowed, void* stream) {
  if (!logit || !bits || !allowed || B < 0 || hm < 1 || wm < 1 || h < 1 || w < 1) return MSS_ERR_BAD_ARG;
  if (Q < 1 || Q > 128 || ldq < Q) return MSS_ERR_UNSUPPORTED;
  if (B == 0) return MSS_OK;
  if (B > 65535 || (long long)h * w > (1ll << 30)) return MSS_ERR_UNSUPPORTED;
  const int W = (Q + 31) >> 5;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(allowed, 0, sizeof(uint32_t) * (size_t)B * 2 * W, st);
  if (e != hipSuccess) return (int)e;
  const float sy = (float)hm / (float)h, sx = (float)wm / (float)w;       // ATen: scale = in / out when no scale_factor is given
  const int HW = h * w;
  // 4 waves per block, one key per wave and step; enough blocks to cover the chip at the small levels, <= 32 keys per wave at the large
  int kpb = HW / (1024 / (B < 1024 ? B : 1024) + 1);
  kpb = kpb < 4 ? 4 : (kpb > 128 ? 128 : kpb);
  const dim3 grid(mss_cdiv(HW, kpb), B);
  hipLaunchKernelGGL(m2f_attn_mask_bits_kernel, grid, dim3(256), 0, st, logit, Q, ldq, hm, wm, h, w, sy, sx, kpb, bits, allowed);
  return mss_launch_status();
}

long long mss_m2f_attn_workspace_bytes(int B, int Q, int A, int chunks) {
  if (B < 1 || Q < 1 || Q > 128 || A < 1 || chunks < 2) return 0;
  const int QS = 64 * ((Q + 63) / 64);
  return (long long)B * A * NH * chunks * WSROWS * QS * (long long)sizeof(float);
}

int mss_m2f_masked_attention_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint32_t* bits,
                                 const uint32_t* allowed, int B, int Q, int NK, int A, float scale, int chunks, float* ws,
                                 float* out, int ldo, void* stream) {
  if (!q || !k || !v || !out || B < 0 || NK < 1 || chunks < 1 || (bits && !allowed)) return MSS_ERR_BAD_ARG;
  if (Q < 1 || Q > 128 || A < 1 || A > 16) return MSS_ERR_UNSUPPORTED;
  const int cols = A * NH * HD;
  if (ldq < cols || ldk < cols || ldv < cols || ldo < cols || (ldq | ldk | ldv | ldo) % 4) return MSS_ERR_UNSUPPORTED;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out)) return MSS_ERR_UNSUPPORTED;
  if (B == 0) return MSS_OK;
  if (B > 65535) return MSS_ERR_UNSUPPORTED;
  int kpc, nchunks;
  chunk_plan(NK, chunks, &kpc, &nchunks);
  if (nchunks > 1 && !ws) return MSS_ERR_BAD_ARG;
  const int QS = 64 * ((Q + 63) / 64);
  const float sl2 = scale * 1.4426950408889634f;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(nchunks, NH * A, B), block(QS);
#define MSS_ATTN_LAUNCH(MASKED, DIRECT)                                                                                          \
  hipLaunchKernelGGL((m2f_masked_attention_kernel<MASKED, DIRECT>), grid, block, 0, st, q, ldq, k, ldk, v, ldv, bits, allowed, Q, NK, \
                     A, sl2, kpc, ws, out, ldo)
  if (nchunks == 1) {
    if (bits) MSS_ATTN_LAUNCH(true, true); else MSS_ATTN_LAUNCH(false, true);
    return mss_launch_status();
  }
  if (bits) MSS_ATTN_LAUNCH(true, false); else MSS_ATTN_LAUNCH(false, false);
#undef MSS_ATTN_LAUNCH
  int rc = mss_launch_status();
  if (rc != MSS_OK) return rc;
  const long long total = (long long)B * A * NH * HD * QS;
  hipLaunchKernelGGL(m2f_attn_merge_kernel, dim3(mss_cdiv(total, 256)), dim3(256), 0, st, ws, B, Q, QS, A, nchunks, out, ldo);
  return mss_launch_status();
}

}  // extern "C"
