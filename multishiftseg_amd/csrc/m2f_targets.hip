// Mask2Former targets from label maps, on the device (include/mss_hip.h: mss_m2f_targets_from_labels).
// replaces train_m2f.py:342-385 (prepare_input: target[b].cpu().numpy(), np.unique, one `sem_seg == class_id` map per class, the OOD
// map) and lib/network/mask2former/maskformer_model.py:316-339 (prepare_targets: the zero padding) with three launches:
//   count 1: per-image class presence as a 128-bit set -- every workgroup ORs into its own set in LDS, then into the image's
//            (integer atomicOr: order-independent, so the result is exact);
//   count 2: one workgroup per image turns the sets into tstart, the packed ascending labels and rank[b][v] (the row of class v
//            inside image b, or -1);
//   fill   : a workgroup turns a stretch of one image's padded plane into row codes in LDS (rank, 0xFE for an OOD pixel, 0xFF for
//            "nothing" and for the padding); a thread owns a run of VW consecutive pixels of one padded image row and stores one
//            VW-byte vector per target row of its image and one for the OOD map: every byte of tmask and ood is written, a
//            wave's store is 64 * VW consecutive bytes of one mask.
// Integer arithmetic only, no float atomics, no scratch: two runs give the same bytes.
#include "mss_common.h"
#include "../../include/mss_hip.h"

namespace {

constexpr int TGT_MAX_CLASSES = 128;      // label_threshold <= 128: the presence set is two 64-bit words, a row code is one byte
constexpr unsigned TGT_NONE = 0xFFu;      // row code of a pixel that belongs to no target row (rank <= 127 never collides)
constexpr unsigned TGT_OOD = 0xFEu;       // ... and is an OOD pixel

// a value is a class iff 0 <= v < thr (train_m2f.py:357: `classes < label_threshold`; a negative value is NOT a class here)
template <typename T>
__device__ __forceinline__ long long tgt_value(T v) { return (long long)v; }

template <typename T>
__global__ __launch_bounds__(256) void targets_present_kernel(const T* __restrict__ sem, long long HW, int thr,
                                                              unsigned long long* __restrict__ present) {
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ unsigned long long set[2];
  if (threadIdx.x < 2) set[threadIdx.x] = 0ull;
  __syncthreads();
  const T* img = sem + (long long)blockIdx.y * HW;
  const bool aligned = (reinterpret_cast<uintptr_t>(img) & 15) == 0;
  unsigned long long lo = 0ull, hi = 0ull;
  auto mark = [&](long long v) {
    if (v >= 0 && v < thr) {
      if (v < 64) lo |= 1ull << v;
      else hi |= 1ull << (v - 64);
    }
  };
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC; i < HW; i += (long long)gridDim.x * 256 * VEC) {
    if (aligned && i + VEC <= HW) {
      alignas(16) T v[VEC];
      *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(img + i);
#pragma unroll
      for (int j = 0; j < VEC; ++j) mark(tgt_value(v[j]));
    } else {
      for (int j = 0; j < VEC && i + j < HW; ++j) mark(tgt_value(img[i + j]));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo |= __shfl_xor(lo, o);
    hi |= __shfl_xor(hi, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (lo) atomicOr(&set[0], lo);
    if (hi) atomicOr(&set[1], hi);
  }
  __syncthreads();
  if (threadIdx.x < 2 && set[threadIdx.x]) atomicOr(&present[2 * blockIdx.y + threadIdx.x], set[threadIdx.x]);
}

// one workgroup per image, thread v = class v
__global__ __launch_bounds__(TGT_MAX_CLASSES) void targets_rank_kernel(const unsigned long long* __restrict__ present, int B, int thr,
                                                                       int* __restrict__ tstart, int* __restrict__ labels,
                                                                       int* __restrict__ rank) {
  __shared__ int start_s;
  const int b = blockIdx.x, v = threadIdx.x;
  if (v == 0) start_s = 0;
  __syncthreads();
  int part = 0;
  for (int i = v; i < b; i += TGT_MAX_CLASSES) part += __popcll(present[2 * i]) + __popcll(present[2 * i + 1]);
  if (part) atomicAdd(&start_s, part);
  __syncthreads();
  const int start = start_s;
  const unsigned long long lo = present[2 * b], hi = present[2 * b + 1];
  if (v < thr) {
    const bool on = ((v < 64 ? lo >> v : hi >> (v - 64)) & 1ull) != 0;
    const int below = v < 64 ? __popcll(lo & ((1ull << v) - 1ull)) : __popcll(lo) + __popcll(hi & ((1ull << (v - 64)) - 1ull));
    rank[(long long)b * thr + v] = on ? below : -1;
    if (on) labels[start + below] = v;
  }
  if (v == 0) {
    tstart[b] = start;
    if (b == B - 1) tstart[B] = start + __popcll(lo) + __popcll(hi);
  }
}

typedef unsigned tgt_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned tgt_u32x2 __attribute__((ext_vector_type(2)));
template <int VW> struct TgtVec;
template <> struct TgtVec<16> { typedef tgt_u32x4 type; };
template <> struct TgtVec<8> { typedef tgt_u32x2 type; };
template <> struct TgtVec<4> { typedef unsigned type; };
template <> struct TgtVec<2> { typedef unsigned short type; };
template <> struct TgtVec<1> { typedef unsigned char type; };

// 0x01 in every byte of x that equals the byte c (exact: no carry crosses a byte), 0x00 elsewhere
__device__ __forceinline__ unsigned tgt_bytes_equal(unsigned x, unsigned c) {
  const unsigned d = x ^ (c * 0x01010101u);
  return (~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d | 0x7F7F7F7Fu)) >> 7;
}

// VW divides Wp and the alignment of tmask and ood, so every store of VW bytes is aligned. A workgroup owns 256 * VW consecutive
// bytes of the image's padded plane. It first turns their pixels into row codes in LDS, lane after lane along the row, so the
// label map is read coalesced whatever its element size; a thread then picks up the VW codes of its run with one LDS read.
// grid: (padded plane / (256 * VW), B)
template <typename T, int VW>
__global__ __launch_bounds__(256) void targets_fill_kernel(const T* __restrict__ sem, int H, int W, int Hp, int Wp, int thr, int ignore,
                                                           const int* __restrict__ tstart, const int* __restrict__ rank,
                                                           long long total_t, unsigned char* __restrict__ tmask,
                                                           unsigned char* __restrict__ ood) {
  typedef typename TgtVec<VW>::type vec_t;
  constexpr int NW = (VW + 3) / 4;                 // dwords that hold a run's codes
  __shared__ unsigned char code_of[TGT_MAX_CLASSES];
  __shared__ __attribute__((aligned(16))) unsigned char stage[256 * VW];
  const int b = blockIdx.y;
  if (threadIdx.x < TGT_MAX_CLASSES) {
    int r = threadIdx.x < thr ? rank[(long long)b * thr + threadIdx.x] : -1;
    code_of[threadIdx.x] = (r >= 0 && r < TGT_MAX_CLASSES) ? (unsigned char)r : (unsigned char)TGT_NONE;
  }
  __syncthreads();
  const long long plane = (long long)Hp * Wp;
  const long long chunk0 = (long long)blockIdx.x * (256 * VW);
  const int y0 = (int)(chunk0 / Wp);
  const unsigned x0 = (unsigned)(chunk0 % Wp);
  const T* img = sem + (long long)b * H * W;
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    const unsigned p = (unsigned)(k * 256) + threadIdx.x, xs = x0 + p;      // Wp <= 2^30 (checked by the launcher): no overflow
    const unsigned x = xs % (unsigned)Wp;
    const long long y = (long long)y0 + xs / (unsigned)Wp;
    unsigned c = TGT_NONE;                                                   // the padding, and rows past the plane's end
    if (y < H && x < (unsigned)W) {
      const long long v = tgt_value(img[y * W + x]);
      if (v >= 0 && v < thr) c = code_of[v];
      else if (v > thr && v != ignore) c = TGT_OOD;
    }
    stage[p] = (unsigned char)c;
  }
  __syncthreads();
  const long long at = chunk0 + (long long)threadIdx.x * VW;
  if (at >= plane) return;
  unsigned codes[NW];
  {
    const vec_t in = *reinterpret_cast<const vec_t*>(&stage[threadIdx.x * VW]);
    if constexpr (VW == 16) { codes[0] = in.x; codes[1] = in.y; codes[2] = in.z; codes[3] = in.w; }
    else if constexpr (VW == 8) { codes[0] = in.x; codes[1] = in.y; }
    else if constexpr (VW == 4) codes[0] = in;
    else codes[0] = (unsigned)in | (VW == 2 ? 0xFFFF0000u : 0xFFFFFF00u);
  }
  auto store = [&](unsigned char* dst, unsigned c) {
    unsigned w[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = tgt_bytes_equal(codes[k], c);
    vec_t out;
    if constexpr (VW == 16) out = tgt_u32x4{w[0], w[1], w[2], w[3]};
    else if constexpr (VW == 8) out = tgt_u32x2{w[0], w[1]};
    else out = (vec_t)w[0];
    *reinterpret_cast<vec_t*>(dst) = out;      // plain stores: nontemporal ones measured 15 % slower at 16 x 704 x 704
  };
  store(ood + (long long)b * plane + at, TGT_OOD);
  const int first = tstart[b];
  int count = tstart[b + 1] - first;
  if (count > TGT_MAX_CLASSES) count = TGT_MAX_CLASSES;
  for (int r = 0; r < count; ++r) {
    const long long g = (long long)first + r;
    if (g < 0 || g >= total_t) break;              // a tstart that does not fit total_t never writes outside tmask
    store(tmask + g * plane + at, (unsigned)r);
  }
}

template <typename T>
int launch_present(const void* sem, int B, long long HW, int thr, unsigned long long* present, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  long long nb = (HW + 256ll * VEC * 4 - 1) / (256ll * VEC * 4);       // about four vectors per thread
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(targets_present_kernel<T>, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, s, static_cast<const T*>(sem), HW, thr, present);
  return mss_launch_status();
}

template <typename T, int VW>
int launch_fill_vw(const void* sem, int B, int H, int W, int Hp, int Wp, int thr, int ignore, const int* tstart, const int* rank,
                   long long total_t, unsigned char* tmask, unsigned char* ood, hipStream_t s) {
  const long long runs = (long long)Hp * (Wp / VW), nb = (runs + 255) / 256;
  if (nb > 0x7fffffffll || Wp > (1 << 30)) return MSS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((targets_fill_kernel<T, VW>), dim3((unsigned)nb, (unsigned)B), dim3(256), 0, s, static_cast<const T*>(sem), H, W, Hp, Wp, thr,
                     ignore, tstart, rank, total_t, tmask, ood);
  return mss_launch_status();
}

template <typename T>
int launch_fill(int vw, const void* sem, int B, int H, int W, int Hp, int Wp, int thr, int ignore, const int* tstart, const int* rank,
                long long total_t, unsigned char* tmask, unsigned char* ood, hipStream_t s) {
  switch (vw) {
    case 16: return launch_fill_vw<T, 16>(sem, B, H, W, Hp, Wp, thr, ignore, tstart, rank, total_t, tmask, ood, s);
    case 8: return launch_fill_vw<T, 8>(sem, B, H, W, Hp, Wp, thr, ignore, tstart, rank, total_t, tmask, ood, s);
    case 4: return launch_fill_vw<T, 4>(sem, B, H, W, Hp, Wp, thr, ignore, tstart, rank, total_t, tmask, ood, s);
    case 2: return launch_fill_vw<T, 2>(sem, B, H, W, Hp, Wp, thr, ignore, tstart, rank, total_t, tmask, ood, s);
    default: return launch_fill_vw<T, 1>(sem, B, H, W, Hp, Wp, thr, ignore, tstart, rank, total_t, tmask, ood, s);
  }
}

}  // namespace

extern "C" int mss_m2f_targets_from_labels(const void* sem, int sem_bytes, int B, int H, int W, int Hp, int Wp, int label_threshold,
                                           int ignore_label, int phase, unsigned long long* present, int* tstart, int* labels, int* rank,
                                           long long total_t, unsigned char* tmask, unsigned char* ood, void* stream) {
  if (label_threshold < 1 || label_threshold > TGT_MAX_CLASSES || (sem_bytes != 1 && sem_bytes != 4 && sem_bytes != 8)) return MSS_ERR_UNSUPPORTED;
  if (B < 1 || H < 1 || W < 1 || Hp < H || Wp < W || (phase != 0 && phase != 1) || total_t < 0 || !sem || !tstart || !rank) return MSS_ERR_BAD_ARG;
  if (phase == 0 && (!present || !labels)) return MSS_ERR_BAD_ARG;
  if (phase == 1 && (!ood || (total_t > 0 && !tmask))) return MSS_ERR_BAD_ARG;
  if (B > 65535) return MSS_ERR_UNSUPPORTED;         // the image is the grid's y
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long HW = (long long)H * W;
  if (phase == 0) {
    hipError_t e = hipMemsetAsync(present, 0, (size_t)B * 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    int rc = sem_bytes == 8 ? launch_present<long long>(sem, B, HW, label_threshold, present, s)
             : sem_bytes == 4 ? launch_present<int>(sem, B, HW, label_threshold, present, s)
                              : launch_present<unsigned char>(sem, B, HW, label_threshold, present, s);
    if (rc != MSS_OK) return rc;
    hipLaunchKernelGGL(targets_rank_kernel, dim3((unsigned)B), dim3(TGT_MAX_CLASSES), 0, s, present, B, label_threshold, tstart, labels, rank);
    return mss_launch_status();
  }
  // the widest store that every row start of both outputs is aligned to
  int vw = 16;
  const uintptr_t bits = (uintptr_t)(unsigned)Wp | reinterpret_cast<uintptr_t>(ood) | reinterpret_cast<uintptr_t>(tmask);
  while (vw > 1 && (bits & (uintptr_t)(vw - 1))) vw >>= 1;
  return sem_bytes == 8 ? launch_fill<long long>(vw, sem, B, H, W, Hp, Wp, label_threshold, ignore_label, tstart, rank, total_t, tmask, ood, s)
         : sem_bytes == 4 ? launch_fill<int>(vw, sem, B, H, W, Hp, Wp, label_threshold, ignore_label, tstart, rank, total_t, tmask, ood, s)
                          : launch_fill<unsigned char>(vw, sem, B, H, W, Hp, Wp, label_threshold, ignore_label, tstart, rank, total_t, tmask, ood, s);
}
