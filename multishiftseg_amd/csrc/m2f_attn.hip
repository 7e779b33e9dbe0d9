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
//     denominator) in a workspace and m2f_attn_merge_kernel folds the chunks in fixed order -- no float atomics, bit-reproducible;
//   * for training the same kernels also leave the log-sum-exp of every (head, query), and the backward (further down) runs as a
//     lane-per-key kernel for dK / dV and a lane-per-query kernel for dQ, again without float atomics.
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
// exp2). DIRECT (chunks == 1): normalise and store; else leave the chunk's partial state in ws [slot][34][QS]. LSE (DIRECT only, the
// training forward): `ws` is the lse output instead -- the kernel sits at the SGPR limit, a further pointer argument would spill.
template <bool MASKED, bool DIRECT, bool LSE>
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
  float* lp = nullptr;                 // LSE: this lane's lse element, pinned in vector registers so the key loop's scalar budget is the inference kernel's
  if (LSE) {
    lp = ws + ((long long)(b * A + a) * NH + hd) * Q + min(qi, Q - 1);
    asm volatile("" : "+v"(lp));
  }
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
    if (LSE) *lp = m + log2f(l);                                                   // training forward: `ws` is lse [B][A][8][Q] here
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
                                                             float* __restrict__ out, int ldo, float* __restrict__ lse) {
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
  if (lse && d == 0) lse[bah * Q + qi] = M + log2f(den);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// With s2 = scale * log2(e) * <q, k> (the forward's scores, same fma chain), P = exp2(s2 - lse) and D = <dout, out> per query:
//   dV = P^T dout,  dS = P o (dout V^T - D),  dQ = scale dS K,  dK = scale dS^T Q.
// Two kernels, each with the mapping under which ITS sum stays inside a lane (no cross-lane reduction, no float atomics):
//   * m2f_attn_bwd_dkv_kernel: lane = key (its k / v rows and 32 + 32 accumulators in registers), the queries of the head staged once in
//     LDS (scaled q and dout, 2 x 128 x 32 x 4 B = 32 KB, + lse and D) and read as broadcasts; dK / dV of a key are complete in its lane
//     and stored once;
//   * m2f_attn_bwd_dq_kernel: lane = query, wave-uniform key rows, the forward's mapping and chunking; a chunk leaves its partial dQ in
//     the workspace and m2f_attn_bwd_dq_merge_kernel adds the chunks in index order.
constexpr int BK = 128;       // keys per workgroup of the dK / dV kernel

// delta [B][A][8][QS]: D of every query (one thread each)
__global__ __launch_bounds__(256) void m2f_attn_bwd_delta_kernel(const float* __restrict__ dout, int lddo, const float* __restrict__ out, int ldo,
                                                                 int B, int Q, int QS, int A, float* __restrict__ delta) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * A * NH * QS) return;
  const int qi = (int)(i % QS);
  const long long bah = i / QS;
  if (qi >= Q) return;
  const int hd = (int)(bah % NH), a = (int)((bah / NH) % A), b = (int)(bah / ((long long)NH * A));
  const int col = a * (NH * HD) + hd * HD;
  const float* gp = dout + ((long long)b * Q + qi) * lddo + col;
  const float* op = out + ((long long)b * Q + qi) * ldo + col;
  float D = 0.f;
#pragma unroll
  for (int d = 0; d < HD; d += 4) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(gp + d), o = *reinterpret_cast<const f32x4*>(op + d);
    D = __builtin_fmaf(g.x, o.x, D); D = __builtin_fmaf(g.y, o.y, D); D = __builtin_fmaf(g.z, o.z, D); D = __builtin_fmaf(g.w, o.w, D);
  }
  delta[i] = D;
}

// grid (ceil(NK / BK), 8 * A, B), block BK. dk / dv [B*NK, A*256] dense (either may be null). A key beyond NK, a masked (key, query)
// pair and a query >= Q contribute nothing; a key masked for every query gets exact zeros.
template <bool MASKED>
__global__ __launch_bounds__(BK) void m2f_attn_bwd_dkv_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                              const float* __restrict__ v, int ldv, const uint32_t* __restrict__ bits,
                                                              const uint32_t* __restrict__ allowed, const float* __restrict__ dout, int lddo,
                                                              const float* __restrict__ lse, const float* __restrict__ delta, int Q, int QS,
                                                              int NK, int A, float scale_log2e, float ln2, float* __restrict__ dk,
                                                              float* __restrict__ dv) {
  __shared__ f32x4 qs[128 * (HD / 4)];
  __shared__ f32x4 gs[128 * (HD / 4)];
  __shared__ float ls[128];
  __shared__ float dl[128];
  const int a = blockIdx.y >> 3, hd = blockIdx.y & 7, b = blockIdx.z;
  const int col = a * (NH * HD) + hd * HD;
  const int W = (Q + 31) >> 5;
  const long long bah = (long long)(b * A + a) * NH + hd;
  for (int idx = threadIdx.x; idx < Q * (HD / 4); idx += BK) {
    const int row = idx >> 3, c4 = (idx & 7) * 4;
    const f32x4 t = *reinterpret_cast<const f32x4*>(q + ((long long)b * Q + row) * ldq + col + c4);
    qs[idx] = f32x4{t.x * scale_log2e, t.y * scale_log2e, t.z * scale_log2e, t.w * scale_log2e};
    gs[idx] = *reinterpret_cast<const f32x4*>(dout + ((long long)b * Q + row) * lddo + col + c4);
  }
  for (int i = threadIdx.x; i < Q; i += BK) {
    ls[i] = lse[bah * Q + i];
    dl[i] = delta[bah * QS + i];
  }
  __syncthreads();
  const int key = blockIdx.x * BK + threadIdx.x;
  const bool in = key < NK;
  const int kc = min(key, NK - 1);
  float kr[HD], vr[HD], dka[HD], dva[HD];
  {
    const float* kp = k + ((long long)b * NK + kc) * ldk + col;
    const float* vp = v + ((long long)b * NK + kc) * ldv + col;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(kp + d), u = *reinterpret_cast<const f32x4*>(vp + d);
      kr[d] = t.x; kr[d + 1] = t.y; kr[d + 2] = t.z; kr[d + 3] = t.w;
      vr[d] = u.x; vr[d + 1] = u.y; vr[d + 2] = u.z; vr[d + 3] = u.w;
    }
  }
#pragma unroll
  for (int d = 0; d < HD; ++d) { dka[d] = 0.f; dva[d] = 0.f; }
  const uint32_t* brow = MASKED ? bits + ((long long)(b * A + a) * NK + kc) * W : nullptr;
  for (int w = 0; w < W; ++w) {
    uint32_t mw = 0u;                                         // bit j set: query 32 w + j does not attend to this key
    if (MASKED) mw = brow[w] & allowed[(b * A + a) * W + w];   // a query with no allowed key ignores its mask
    const int qn = min(32, Q - 32 * w);
    for (int j = 0; j < qn; ++j) {
      const int qi = 32 * w + j;
      float qv[HD], gv[HD];
#pragma unroll
      for (int d = 0; d < HD; d += 4) {
        const f32x4 t = qs[qi * (HD / 4) + (d >> 2)], u = gs[qi * (HD / 4) + (d >> 2)];
        qv[d] = t.x; qv[d + 1] = t.y; qv[d + 2] = t.z; qv[d + 3] = t.w;
        gv[d] = u.x; gv[d + 1] = u.y; gv[d + 2] = u.z; gv[d + 3] = u.w;
      }
      float dot = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) dot = __builtin_fmaf(qv[d], kr[d], dot);
#pragma unroll
      for (int d = 0; d < HD; ++d) dp = __builtin_fmaf(gv[d], vr[d], dp);
      const bool dead = !in || ((mw >> j) & 1u);
      const float p = dead ? 0.f : exp2f(dot - ls[qi]);
      const float ds = p * (dp - dl[qi]);
#pragma unroll
      for (int d = 0; d < HD; ++d) {
        dva[d] = __builtin_fmaf(p, gv[d], dva[d]);
        dka[d] = __builtin_fmaf(ds, qv[d], dka[d]);
      }
    }
  }
  if (!in) return;
  if (dk) {
    float* op = dk + ((long long)b * NK + key) * (A * NH * HD) + col;
#pragma unroll
    for (int d = 0; d < HD; d += 4) *reinterpret_cast<f32x4*>(op + d) = f32x4{dka[d] * ln2, dka[d + 1] * ln2, dka[d + 2] * ln2, dka[d + 3] * ln2};
  }
  if (dv) {
    float* op = dv + ((long long)b * NK + key) * (A * NH * HD) + col;
#pragma unroll
    for (int d = 0; d < HD; d += 4) *reinterpret_cast<f32x4*>(op + d) = f32x4{dva[d], dva[d + 1], dva[d + 2], dva[d + 3]};
  }
}

// grid (chunks, 8 * A, B), block 64 * ceil(Q / 64): the forward's mapping. DIRECT (one chunk): dq [B*Q, A*256] = scale * sum; else the
// chunk's sum goes to ws [slot][32][QS].
template <bool MASKED, bool DIRECT>
__global__ __launch_bounds__(128) void m2f_attn_bwd_dq_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                              const float* __restrict__ v, int ldv, const uint32_t* __restrict__ bits,
                                                              const uint32_t* __restrict__ allowed, const float* __restrict__ dout, int lddo,
                                                              const float* __restrict__ lse, const float* __restrict__ delta, int Q, int NK,
                                                              int A, float scale_log2e, float scale, int keys_per_chunk,
                                                              float* __restrict__ ws, float* __restrict__ dq) {
  const int c = blockIdx.x, a = blockIdx.y >> 3, hd = blockIdx.y & 7, b = blockIdx.z;
  const int col = a * (NH * HD) + hd * HD;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qi = wave * 64 + lane;
  const int qc = min(qi, Q - 1);
  const int QS = blockDim.x;
  const int W = (Q + 31) >> 5;
  const long long bah = (long long)(b * A + a) * NH + hd;
  float qr[HD], gr[HD], acc[HD];
  {
    const float* qp = q + ((long long)b * Q + qc) * ldq + col;
    const float* gp = dout + ((long long)b * Q + qc) * lddo + col;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(qp + d), u = *reinterpret_cast<const f32x4*>(gp + d);
      qr[d] = t.x * scale_log2e; qr[d + 1] = t.y * scale_log2e; qr[d + 2] = t.z * scale_log2e; qr[d + 3] = t.w * scale_log2e;
      gr[d] = u.x; gr[d + 1] = u.y; gr[d + 2] = u.z; gr[d + 3] = u.w;
    }
  }
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
  const float L = lse[bah * Q + qc], D = delta[bah * QS + qc];
  const int k0 = c * keys_per_chunk, k1 = min(NK, k0 + keys_per_chunk);
  const float* kb = k + (long long)b * NK * ldk + col;
  const float* vb = v + (long long)b * NK * ldv + col;
  const int w0 = 2 * wave, w1 = min(2 * wave + 1, W - 1);
  const uint32_t* brow = nullptr;
  uint32_t live = 0u;
  const int sh = lane & 31;
  const bool hi = (lane & 32) != 0;
  if (MASKED) {
    brow = bits + (long long)(b * A + a) * NK * W;
    const uint32_t al0 = allowed[(b * A + a) * W + w0], al1 = allowed[(b * A + a) * W + w1];
    live = hi ? al1 : al0;
  }
#pragma unroll 2
  for (int key = k0; key < k1; ++key) {
    const float* kr = kb + (long long)key * ldk;
    const float* vr = vb + (long long)key * ldv;
    float dot = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) dot = __builtin_fmaf(qr[d], kr[d], dot);
#pragma unroll
    for (int d = 0; d < HD; ++d) dp = __builtin_fmaf(gr[d], vr[d], dp);
    bool masked = false;
    if (MASKED) {
      const uint32_t b0 = brow[(long long)key * W + w0], b1 = brow[(long long)key * W + w1];
      masked = (((hi ? b1 : b0) & live) >> sh) & 1u;
    }
    const float p = masked ? 0.f : exp2f(dot - L);
    const float ds = p * (dp - D);
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(ds, kr[d], acc[d]);
  }
  if (qi >= Q) return;
  if (DIRECT) {
    float* op = dq + ((long long)b * Q + qi) * (A * NH * HD) + col;
#pragma unroll
    for (int d = 0; d < HD; d += 4) *reinterpret_cast<f32x4*>(op + d) = f32x4{acc[d] * scale, acc[d + 1] * scale, acc[d + 2] * scale, acc[d + 3] * scale};
  } else {
    float* wp = ws + (bah * gridDim.x + c) * HD * QS + qi;
#pragma unroll
    for (int d = 0; d < HD; ++d) wp[d * QS] = acc[d];
  }
}

// one thread per (image, attention, head, channel, query): adds the chunks' partial dQ in index order
__global__ __launch_bounds__(256) void m2f_attn_bwd_dq_merge_kernel(const float* __restrict__ ws, int B, int Q, int QS, int A, int chunks,
                                                                    float scale, float* __restrict__ dq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * A * NH * HD * QS) return;
  const int qi = (int)(i % QS);
  const int d = (int)((i / QS) % HD);
  const long long bah = i / ((long long)QS * HD);
  if (qi >= Q) return;
  const int hd = (int)(bah % NH), a = (int)((bah / NH) % A), b = (int)(bah / ((long long)NH * A));
  const float* base = ws + (bah * chunks * HD + d) * QS + qi;
  float sum = 0.f;
  for (int c = 0; c < chunks; ++c) sum += base[(long long)c * HD * QS];
  dq[((long long)b * Q + qi) * (A * NH * HD) + a * (NH * HD) + hd * HD + d] = sum * scale;
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

int mss_m2f_masked_attention_lse_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint32_t* bits,
                                     const uint32_t* allowed, int B, int Q, int NK, int A, float scale, int chunks, float* ws,
                                     float* out, int ldo, float* lse, void* stream) {
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
  // only the DIRECT kernel writes lse itself (through its otherwise unused `ws` argument), the chunked one leaves that to the merge
#define MSS_ATTN_LAUNCH(MASKED, DIRECT, LSE)                                                                                          \
  hipLaunchKernelGGL((m2f_masked_attention_kernel<MASKED, DIRECT, LSE>), grid, block, 0, st, q, ldq, k, ldk, v, ldv, bits, allowed, Q, NK, \
                     A, sl2, kpc, LSE ? lse : ws, out, ldo)
  if (nchunks == 1) {
    if (lse) {
      if (bits) MSS_ATTN_LAUNCH(true, true, true); else MSS_ATTN_LAUNCH(false, true, true);
    } else {
      if (bits) MSS_ATTN_LAUNCH(true, true, false); else MSS_ATTN_LAUNCH(false, true, false);
    }
    return mss_launch_status();
  }
  if (bits) MSS_ATTN_LAUNCH(true, false, false); else MSS_ATTN_LAUNCH(false, false, false);
#undef MSS_ATTN_LAUNCH
  int rc = mss_launch_status();
  if (rc != MSS_OK) return rc;
  const long long total = (long long)B * A * NH * HD * QS;
  hipLaunchKernelGGL(m2f_attn_merge_kernel, dim3(mss_cdiv(total, 256)), dim3(256), 0, st, ws, B, Q, QS, A, nchunks, out, ldo, lse);
  return mss_launch_status();
}

// the inference entry point: the same kernels, no lse
int mss_m2f_masked_attention_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint32_t* bits,
                                 const uint32_t* allowed, int B, int Q, int NK, int A, float scale, int chunks, float* ws,
                                 float* out, int ldo, void* stream) {
  return mss_m2f_masked_attention_lse_f32(q, ldq, k, ldk, v, ldv, bits, allowed, B, Q, NK, A, scale, chunks, ws, out, ldo, nullptr, stream);
}

// D of every query [B][A][8][QS], then (more than one chunk) the chunks' partial dQ [B][A][8][chunks][32][QS]
long long mss_m2f_attn_bwd_workspace_bytes(int B, int Q, int A, int chunks) {
  if (B < 1 || Q < 1 || Q > 128 || A < 1 || chunks < 1) return 0;
  const int QS = 64 * ((Q + 63) / 64);
  return (long long)B * A * NH * QS * (1 + (chunks > 1 ? (long long)chunks * HD : 0)) * (long long)sizeof(float);
}

int mss_m2f_masked_attention_bwd_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint32_t* bits,
                                     const uint32_t* allowed, const float* out, int ldo, const float* lse, const float* dout, int lddo,
                                     int B, int Q, int NK, int A, float scale, int chunks, float* ws, float* dq, float* dk, float* dv,
                                     void* stream) {
  if (!q || !k || !v || !out || !lse || !dout || !ws || B < 0 || NK < 1 || chunks < 1 || (bits && !allowed)) return MSS_ERR_BAD_ARG;
  if (Q < 1 || Q > 128 || A < 1 || A > 16) return MSS_ERR_UNSUPPORTED;
  const int cols = A * NH * HD;
  if (ldq < cols || ldk < cols || ldv < cols || ldo < cols || lddo < cols || (ldq | ldk | ldv | ldo | lddo) % 4) return MSS_ERR_UNSUPPORTED;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(dout) || !aligned16(dq) || !aligned16(dk) ||
      !aligned16(dv))
    return MSS_ERR_UNSUPPORTED;
  if (B == 0) return MSS_OK;
  if (B > 65535) return MSS_ERR_UNSUPPORTED;
  const int QS = 64 * ((Q + 63) / 64);
  const float sl2 = scale * 1.4426950408889634f;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* delta = ws;
  float* parts = ws + (long long)B * A * NH * QS;
  hipLaunchKernelGGL(m2f_attn_bwd_delta_kernel, dim3(mss_cdiv((long long)B * A * NH * QS, 256)), dim3(256), 0, st, dout, lddo, out, ldo, B,
                     Q, QS, A, delta);
  int rc = mss_launch_status();
  if (rc != MSS_OK) return rc;
  if (dk || dv) {
    const dim3 grid(mss_cdiv(NK, BK), NH * A, B);
    if (bits)
      hipLaunchKernelGGL((m2f_attn_bwd_dkv_kernel<true>), grid, dim3(BK), 0, st, q, ldq, k, ldk, v, ldv, bits, allowed, dout, lddo, lse, delta,
                         Q, QS, NK, A, sl2, 0.6931471805599453f, dk, dv);
    else
      hipLaunchKernelGGL((m2f_attn_bwd_dkv_kernel<false>), grid, dim3(BK), 0, st, q, ldq, k, ldk, v, ldv, bits, allowed, dout, lddo, lse, delta,
                         Q, QS, NK, A, sl2, 0.6931471805599453f, dk, dv);
    rc = mss_launch_status();
    if (rc != MSS_OK) return rc;
  }
  if (!dq) return MSS_OK;
  int kpc, nchunks;
  chunk_plan(NK, chunks, &kpc, &nchunks);
  const dim3 grid(nchunks, NH * A, B), block(QS);
#define MSS_ATTN_BWD_LAUNCH(MASKED, DIRECT)                                                                                        \
  hipLaunchKernelGGL((m2f_attn_bwd_dq_kernel<MASKED, DIRECT>), grid, block, 0, st, q, ldq, k, ldk, v, ldv, bits, allowed, dout, lddo, lse, \
                     delta, Q, NK, A, sl2, scale, kpc, parts, dq)
  if (nchunks == 1) {
    if (bits) MSS_ATTN_BWD_LAUNCH(true, true); else MSS_ATTN_BWD_LAUNCH(false, true);
    return mss_launch_status();
  }
  if (bits) MSS_ATTN_BWD_LAUNCH(true, false); else MSS_ATTN_BWD_LAUNCH(false, false);
#undef MSS_ATTN_BWD_LAUNCH
  rc = mss_launch_status();
  if (rc != MSS_OK) return rc;
  const long long total = (long long)B * A * NH * HD * QS;
  hipLaunchKernelGGL(m2f_attn_bwd_dq_merge_kernel, dim3(mss_cdiv(total, 256)), dim3(256), 0, st, parts, B, Q, QS, A, nchunks, scale, dq);
  return mss_launch_status();
}

}  // extern "C"
