// Multi-tensor AdamW with full-model gradient clipping (Mask2Former stage 2: train_m2f.py:211-299 builds torch.optim.AdamW with one
// parameter group per tensor and wraps it in FullModelGradientClippingOptimizer, i.e. clip_grad_norm_(all_params, 0.01) before every
// step). One call = three stages over a LIST of float32 tensors, whatever its length:
//   norm    per-chunk sums of squares of every gradient -> scratch[slot(tensor, chunk)] (plain stores: no atomics, no memset)
//   coef    one workgroup folds the slots in a fixed order in double -> out[0] = total_norm, out[1] = clip coefficient
//   update  g' = g * coef, then torch's single-tensor AdamW on (p, g', m, v); g itself is never written
// The tensors' metadata rides in by-value kernel arguments (the multi_tensor_apply scheme): every launch carries up to
// MSS_ADAMW_TENSORS tensors and a block -> (tensor, chunk) map of MSS_ADAMW_BLOCKS entries, and a list needs as many launches as
// it fills. p.grad pointers change every step under zero_grad(set_to_none=True); kernel arguments are copied by the runtime at
// launch, so there is no staging buffer whose lifetime a later step could cut short.
#include "mss_common.h"
#include "../../include/mss_hip.h"
#include <math.h>

namespace {

constexpr int CHUNK = 4096;          // elements per workgroup: 256 threads x 4 x 16 bytes
constexpr int TENSORS = 36;          // tensors per launch
constexpr int BLOCKS = 320;          // workgroups per launch
constexpr int THREADS = 256;
constexpr int VEC_ITERS = CHUNK / (THREADS * 4);

struct TensorMeta {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
  float decay;         // (float)(1 - lr*wd), formed in double
  float neg_step;      // (float)(-(lr / bias1))
  float bc2_sqrt;      // (float)sqrt(bias2)
  int slot0;           // scratch slot of this tensor's chunk 0; chunk c of the tensor owns slot0 + c
};
struct LaunchArgs {
  TensorMeta t[TENSORS];
  int chunk[BLOCKS];                 // chunk index inside its tensor (a tensor may continue over several launches)
  unsigned char tensor[BLOCKS];      // index into t[]
};
static_assert(sizeof(TensorMeta) == 56, "TensorMeta layout");
// HIP's kernel-argument limit is 4096 bytes; the update kernel adds a pointer and four floats behind this struct
static_assert(sizeof(LaunchArgs) + 64 <= 4096, "LaunchArgs must stay inside the kernel-argument limit");

// four consecutive elements starting at i (i % 4 == 0 relative to the tensor start); beyond n: 0
__device__ __forceinline__ f32x4 load4(const float* __restrict__ x, long long i, long long n, bool vec) {
  if (vec && i + 4 <= n) return *reinterpret_cast<const f32x4*>(x + i);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i + k < n) r[k] = x[i + k];
  return r;
}
__device__ __forceinline__ void store4(float* __restrict__ x, long long i, long long n, bool vec, f32x4 r) {
  if (vec && i + 4 <= n) { *reinterpret_cast<f32x4*>(x + i) = r; return; }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i + k < n) x[i + k] = r[k];
}
__device__ __forceinline__ bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

// Sum of squares of one chunk, in an order fixed by the chunk alone: thread t takes elements 4*(it*256 + t) .. +3 on the vector
// and on the scalar route alike, four running sums per thread, DPP / shuffle tree per wave, the four waves in index order.
__global__ void __launch_bounds__(THREADS) adamw_norm_kernel(const LaunchArgs a, float* __restrict__ scratch) {
  __shared__ float wave_sum[THREADS / 64];
  const int ti = a.tensor[blockIdx.x];
  const int chunk = a.chunk[blockIdx.x];
  const float* __restrict__ g = a.t[ti].g;
  const long long n = a.t[ti].n;
  const bool vec = aligned16(g);
  const long long base = (long long)chunk * CHUNK;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int it = 0; it < VEC_ITERS; ++it) {
    const long long i = base + 4ll * (it * THREADS + threadIdx.x);
    if (i < n) {
      const f32x4 x = load4(g, i, n, vec);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = __fmaf_rn(x[k], x[k], acc[k]);
    }
  }
  const float s = mss_wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) scratch[a.t[ti].slot0 + chunk] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// torch/nn/utils/clip_grad.py, clip_grad_norm_(error_if_nonfinite=False), in its order of operations:
//   total_norm = vector_norm(stack([vector_norm(g) for g in grads]))          (a float32 0-d tensor)
//   clip_coef = max_norm / (total_norm + 1e-6)          a Python float over a tensor is Tensor.__rdiv__ (torch/_tensor.py):
//                                                       (total_norm + 1e-6).reciprocal() * max_norm, two float32 roundings
//   clip_coef_clamped = clamp(clip_coef, max=1.0)                             (NaN stays NaN)
//   g.mul_(clip_coef_clamped)
// Here total_norm is the float32 rounding of sqrt(sum of the slots), the sum taken in double in a fixed order: thread t folds the
// contiguous slots [t*per, (t+1)*per) in index order, thread 0 folds the 256 sums in index order.
__global__ void __launch_bounds__(THREADS) adamw_coef_kernel(const float* __restrict__ scratch, int slots, float max_norm,
                                                              float* __restrict__ out) {
  __shared__ double part[THREADS];
  const int per = (slots + THREADS - 1) / THREADS;
  const int lo = min(slots, (int)threadIdx.x * per), hi = min(slots, lo + per);
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s += (double)scratch[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < THREADS; ++i) tot += part[i];
    const float total_norm = (float)sqrt(tot);
    const float c = (1.f / (total_norm + 1e-6f)) * max_norm;      // reciprocal, then the product: not one division
    out[0] = total_norm;
    out[1] = c > 1.f ? 1.f : c;      // clamp(max=1): a NaN coefficient is kept, as torch keeps it
  }
}

// torch/optim/adam.py _single_tensor_adam with decoupled_weight_decay, operation for operation, on g' = g * coef:
//   param.mul_(1 - lr*wd) ; exp_avg.lerp_(g', 1-b1) ; exp_avg_sq.mul_(b2).addcmul_(g', g', value=1-b2) ;
//   denom = (exp_avg_sq.sqrt() / sqrt(bias2)).add_(eps) ; param.addcdiv_(exp_avg, denom, value=-lr/bias1)
// with the roundings of adam_kernel (csrc/glue.hip). Contraction is off so that g * coef is rounded before it is used, as the
// in-place mul_ of clip_grad_norm_ rounds it; the fused operations are the ones spelled out.
__global__ void __launch_bounds__(THREADS) adamw_update_kernel(const LaunchArgs a, const float* __restrict__ norm_out,
                                                                float one_minus_b1, float b2, float one_minus_b2, float eps) {
#pragma clang fp contract(off)
  const int ti = a.tensor[blockIdx.x];
  const TensorMeta& t = a.t[ti];
  float* __restrict__ p = t.p;
  const float* __restrict__ g = t.g;
  float* __restrict__ m = t.m;
  float* __restrict__ v = t.v;
  const long long n = t.n;
  const float decay = t.decay, neg_step = t.neg_step, bc2_sqrt = t.bc2_sqrt;
  const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
  const bool clip = norm_out != nullptr;
  const float coef = clip ? norm_out[1] : 1.f;
  const long long base = (long long)a.chunk[blockIdx.x] * CHUNK;
  f32x4 P[VEC_ITERS], G[VEC_ITERS], M[VEC_ITERS], V[VEC_ITERS];
#pragma unroll
  for (int it = 0; it < VEC_ITERS; ++it) {
    const long long i = base + 4ll * (it * THREADS + threadIdx.x);
    if (i < n) {
      P[it] = load4(p, i, n, vec);
      G[it] = load4(g, i, n, vec);
      M[it] = load4(m, i, n, vec);
      V[it] = load4(v, i, n, vec);
    }
  }
#pragma unroll
  for (int it = 0; it < VEC_ITERS; ++it) {
    const long long i = base + 4ll * (it * THREADS + threadIdx.x);
    if (i < n) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float grad = clip ? G[it][k] * coef : G[it][k];                    // g.mul_(clip_coef_clamped)
        const float pi = P[it][k] * decay;                                       // param.mul_(1 - lr*wd)
        const float m0 = M[it][k];
        const float mi = __fmaf_rn(one_minus_b1, grad - m0, m0);                 // exp_avg.lerp_(grad, 1-b1), weight < 0.5 branch
        const float vi = __fmaf_rn(one_minus_b2 * grad, grad, V[it][k] * b2);    // mul_(b2).addcmul_(grad, grad, value=1-b2)
        const float denom = __fsqrt_rn(vi) / bc2_sqrt + eps;
        P[it][k] = __fmaf_rn(neg_step, mi / denom, pi);                          // addcdiv_(exp_avg, denom, value=-step_size)
        M[it][k] = mi;
        V[it][k] = vi;
      }
      store4(p, i, n, vec, P[it]);
      store4(m, i, n, vec, M[it]);
      store4(v, i, n, vec, V[it]);
    }
  }
}

inline long long chunks_of(long long n) { return n <= 0 ? 0 : (n + CHUNK - 1) / CHUNK; }

// The packing rule, shared by the launcher and by mss_adamw_plan: tensors in list order, chunks in index order; a launch is
// issued when its block map is full, or when its tensor table is full and the last tensor's chunks are all placed; a tensor cut
// by a full block map continues as entry 0 of the next launch. fill(meta, i) sets the per-tensor fields of list entry i;
// emit(args, blocks, list_index) is called once per launch, list_index[e] being the list entry behind args.t[e]. Empty tensors
// take no entry, no block and no slot.
template <class Fill, class Emit>
int walk_plan(int count, const long long* numel, Fill fill, Emit emit) {
  LaunchArgs a;
  int list_index[TENSORS];
  int nt = 0, nb = 0;
  long long slot = 0;
  for (int i = 0; i < count; ++i) {
    const long long chunks = chunks_of(numel[i]);
    if (chunks == 0) continue;
    if (slot + chunks > 0x7fffffffll) return MSS_ERR_UNSUPPORTED;
    fill(a.t[nt], i);
    a.t[nt].n = numel[i];
    a.t[nt].slot0 = (int)slot;
    list_index[nt] = i;
    ++nt;
    for (long long c = 0; c < chunks; ++c) {
      a.tensor[nb] = (unsigned char)(nt - 1);
      a.chunk[nb] = (int)c;
      ++nb;
      const bool last = c == chunks - 1;
      if (nb == BLOCKS || (nt == TENSORS && last)) {
        const int rc = emit(a, nb, list_index);
        if (rc != MSS_OK) return rc;
        nb = 0;
        if (last) {
          nt = 0;
        } else {
          a.t[0] = a.t[nt - 1];
          list_index[0] = list_index[nt - 1];
          nt = 1;
        }
      }
    }
    slot += chunks;
  }
  if (nb > 0) return emit(a, nb, list_index);
  return MSS_OK;
}

}  // namespace

#define S_(x) static_cast<hipStream_t>(x)

extern "C" {

int mss_adamw_chunk_elems(void) { return CHUNK; }
int mss_adamw_tensors_per_launch(void) { return TENSORS; }
int mss_adamw_blocks_per_launch(void) { return BLOCKS; }

long long mss_adamw_scratch_floats(int count, const long long* numel) {
  long long s = 0;
  for (int i = 0; i < count && numel; ++i) s += chunks_of(numel[i]);
  return s;
}

long long mss_adamw_plan(int count, const long long* numel, long long capacity, int* launch, int* block, int* tensor,
                         long long* chunk, int* slot) {
  if (count < 0 || (count > 0 && !numel)) return -1;
  long long entries = 0;
  int launches = 0;
  const bool record = launch && block && tensor && chunk && slot;
  const int rc = walk_plan(
      count, numel, [](TensorMeta&, int) {},
      [&](const LaunchArgs& a, int nb, const int* list_index) {
        for (int b = 0; b < nb; ++b, ++entries) {
          if (!record || entries >= capacity) continue;
          launch[entries] = launches;
          block[entries] = b;
          tensor[entries] = list_index[a.tensor[b]];
          chunk[entries] = a.chunk[b];
          slot[entries] = a.t[a.tensor[b]].slot0 + a.chunk[b];
        }
        ++launches;
        return MSS_OK;
      });
  return rc == MSS_OK ? entries : -1;
}

int mss_adamw_clip_step_f32(int count, float* const* param, const float* const* grad, float* const* exp_avg,
                            float* const* exp_avg_sq, const long long* numel, const double* lr, const double* weight_decay,
                            const int* step, double beta1, double beta2, double eps, int clip, double max_norm, float* scratch,
                            long long scratch_floats, float* norm_out, int* launches, void* stream) {
  if (launches) *launches = 0;
  if (count < 0) return MSS_ERR_BAD_ARG;
  if (count == 0) return MSS_OK;
  if (!param || !grad || !exp_avg || !exp_avg_sq || !numel || !lr || !weight_decay || !step) return MSS_ERR_BAD_ARG;
  long long slots = 0;
  for (int i = 0; i < count; ++i) {
    if (numel[i] < 0 || step[i] < 1) return MSS_ERR_BAD_ARG;
    if (numel[i] > 0 && (!param[i] || !grad[i] || !exp_avg[i] || !exp_avg_sq[i])) return MSS_ERR_BAD_ARG;
    slots += chunks_of(numel[i]);
  }
  if (slots == 0) return MSS_OK;
  if (slots > 0x7fffffffll) return MSS_ERR_UNSUPPORTED;
  if (clip && (!scratch || !norm_out || scratch_floats < slots)) return MSS_ERR_BAD_ARG;
  int issued = 0;
  auto fill = [&](TensorMeta& t, int i) {
    t.p = param[i]; t.g = grad[i]; t.m = exp_avg[i]; t.v = exp_avg_sq[i];
    // as Python forms them: 1 - lr*wd, 1 - beta**step, lr / bias1, bias2 ** 0.5 in double; only the derived scalars are rounded
    const double bc1 = 1.0 - pow(beta1, (double)step[i]);
    const double bc2 = 1.0 - pow(beta2, (double)step[i]);
    t.decay = (float)(1.0 - lr[i] * weight_decay[i]);
    t.neg_step = (float)(-(lr[i] / bc1));
    t.bc2_sqrt = (float)sqrt(bc2);
  };
  int rc = MSS_OK;
  if (clip) {
    auto fill_grad = [&](TensorMeta& t, int i) { t.g = grad[i]; };       // the norm kernel reads g, n and slot0 only
    rc = walk_plan(count, numel, fill_grad, [&](const LaunchArgs& a, int nb, const int*) {
      hipLaunchKernelGGL(adamw_norm_kernel, dim3(nb), dim3(THREADS), 0, S_(stream), a, scratch);
      ++issued;
      return mss_launch_status();
    });
    if (rc != MSS_OK) return rc;
    hipLaunchKernelGGL(adamw_coef_kernel, dim3(1), dim3(THREADS), 0, S_(stream), scratch, (int)slots, (float)max_norm, norm_out);
    ++issued;
    rc = mss_launch_status();
    if (rc != MSS_OK) return rc;
  }
  rc = walk_plan(count, numel, fill, [&](const LaunchArgs& a, int nb, const int*) {
    hipLaunchKernelGGL(adamw_update_kernel, dim3(nb), dim3(THREADS), 0, S_(stream), a, clip ? norm_out : (const float*)nullptr,
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
    ++issued;
    return mss_launch_status();
  });
  if (launches) *launches = issued;
  return rc;
}

}  // extern "C"
