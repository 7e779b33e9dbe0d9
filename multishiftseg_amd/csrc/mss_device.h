// What a launcher knows about the device it launches on, kept PER DEVICE (function attributes and occupancy are per device; a process
// may drive several): one once-cache for every route. The cache is plain C++ (tests/device_cache_check.cpp); the HIP side needs hipcc.
#pragma once
#include <atomic>
#include <mutex>
#include "mss_gemm_dims.h"       // MSS_OK / MSS_ERR_*

constexpr int MSS_MAX_DEVICES = 16;      // device indices 0..15; a launch on any other answers MSS_ERR_UNSUPPORTED

// One Record per device, filled by the first caller's probe under the mutex -- int probe(int dev, Record& r), MSS_OK or a status that
// is returned and NOT cached (the next call probes again). Once filled, a read is an acquire load and a copy: no lock.
template <typename Record>
class MssPerDevice {
  struct Slot { std::atomic<bool> ready{false}; Record rec{}; };
  std::mutex mu_;
  Slot slots_[MSS_MAX_DEVICES];
 public:
  template <typename Probe>
  int get(int dev, Probe&& probe, Record* out) {
    if (dev < 0 || dev >= MSS_MAX_DEVICES) return MSS_ERR_UNSUPPORTED;
    Slot& s = slots_[dev];
    if (!s.ready.load(std::memory_order_acquire)) {
      std::lock_guard<std::mutex> lock(mu_);
      if (!s.ready.load(std::memory_order_relaxed)) {
        if (const int rc = probe(dev, s.rec)) return rc;
        s.ready.store(true, std::memory_order_release);
      }
    }
    if (out) *out = s.rec;
    return MSS_OK;
  }
};

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// device_state.hip: the ticket pool of the split-bf16 kernels' dynamic tile order on the current device (who calls what, and when: there)
void mss_sched_init(hipStream_t stream);
int* mss_sched_slot(hipStream_t stream);
struct MssKernelInfo { int occ, cus; };  // resident workgroups per CU at the launch's block size and LDS; CUs of the device

inline int mss_device_cus(int dev) {     // read once per device, shared by every kernel; 256 where the query fails
  static MssPerDevice<int> cache;
  int cus = 256;
  (void)cache.get(dev, [](int d, int& r) {
    if (hipDeviceGetAttribute(&r, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess) r = 256;
    return MSS_OK;
  }, &cus);
  return cus;
}

// {occ, cus} of kernel Kern on the current device; one cache per kernel. The first call per device raises the kernel's dynamic-LDS
// limit to smem_bytes where that exceeds 48 KB (smem_bytes: the most any launch of Kern asks for) and queries the occupancy
// (fallback_occ where the query fails or answers none). Launchers that need only the raised limit pass no `out`.
template <auto Kern>
int mss_kernel_info(int threads, size_t smem_bytes, int fallback_occ = 1, MssKernelInfo* out = nullptr) {
  static MssPerDevice<MssKernelInfo> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return MSS_ERR_UNSUPPORTED;
  return cache.get(dev, [&](int d, MssKernelInfo& r) {
    if (smem_bytes > 48 * 1024)
      if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_bytes)) return (int)e;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, Kern, threads, smem_bytes) != hipSuccess || n < 1) n = fallback_occ;
    r = {n, mss_device_cus(d)};
    return MSS_OK;
  }, out);
}
#endif
