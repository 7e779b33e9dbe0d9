// Stand-alone host check of the per-device once-cache of csrc/mss_device.h (tests/test_device_cache_cpu.py compiles and runs it, once
// with the host compiler's address and undefined-behaviour sanitizers and once with its thread sanitizer). Only the cache part of the
// header is seen here (no HIP); the probe is a fake that counts its own calls. Eight threads ask for all sixteen devices many times:
//   1. the probe ran exactly once per device and every reader saw the complete record;
//   2. a probe that fails the first time is run again; its failure is returned to the one caller that met it and is not cached;
//   3. device indices -1 and 16 are refused without a probe.
// Prints "ok" and exits 0, or a message at the first violated property and exits 1.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "mss_device.h"

namespace {

constexpr int THREADS = 8, ROUNDS = 2000, FAIL_STATUS = 77;

struct Record { int a, b, c, d; };                              // complete: the four fields name the same device
bool complete(const Record& r, int dev) { return r.a == dev + 1 && r.b == 2 * (dev + 1) && r.c == 3 * (dev + 1) && r.d == 4 * (dev + 1); }

std::atomic<int> probes[MSS_MAX_DEVICES];

int fill(int dev, Record& r) {                                  // slowly, field by field: a reader let in early would see a torn record
  probes[dev].fetch_add(1);
  r.a = dev + 1; std::this_thread::yield();
  r.b = 2 * (dev + 1); std::this_thread::yield();
  r.c = 3 * (dev + 1); std::this_thread::yield();
  r.d = 4 * (dev + 1);
  return MSS_OK;
}
int fill_failing_once(int dev, Record& r) {
  if (probes[dev].load() == 0) { probes[dev].fetch_add(1); r.a = -1; return FAIL_STATUS; }      // leaves rubbish behind, as a real probe may
  return fill(dev, r);
}

// every thread asks for every device ROUNDS times (each starting at another device); per thread: calls that were refused with
// FAIL_STATUS per device, and whether anything else went wrong
struct Tally { int failed[MSS_MAX_DEVICES] = {0}; int bad = 0; };

template <typename Probe>
std::vector<Tally> hammer(MssPerDevice<Record>& cache, Probe probe) {
  std::vector<Tally> tally(THREADS);
  std::atomic<int> waiting{THREADS};
  std::vector<std::thread> pool;
  for (int t = 0; t < THREADS; ++t)
    pool.emplace_back([&, t] {
      waiting.fetch_sub(1);
      while (waiting.load() > 0) std::this_thread::yield();     // all threads make their first call together
      for (int i = 0; i < ROUNDS; ++i)
        for (int k = 0; k < MSS_MAX_DEVICES; ++k) {
          const int dev = (k + 2 * t) % MSS_MAX_DEVICES;
          Record r = {0, 0, 0, 0};
          const int rc = cache.get(dev, probe, &r);
          if (rc == FAIL_STATUS) ++tally[t].failed[dev];
          else if (rc != MSS_OK || !complete(r, dev)) ++tally[t].bad;
        }
    });
  for (auto& th : pool) th.join();
  return tally;
}

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::fprintf(stderr, "%s: ", #cond);                 \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      return 1;                                            \
    }                                                      \
  } while (0)

}  // namespace

int main() {
  {
    static MssPerDevice<Record> cache;
    const std::vector<Tally> tally = hammer(cache, fill);
    for (int t = 0; t < THREADS; ++t) {
      CHECK(tally[t].bad == 0, "thread %d: %d calls failed or saw an incomplete record", t, tally[t].bad);
      for (int d = 0; d < MSS_MAX_DEVICES; ++d) CHECK(tally[t].failed[d] == 0, "thread %d device %d", t, d);
    }
    for (int d = 0; d < MSS_MAX_DEVICES; ++d) CHECK(probes[d].load() == 1, "device %d probed %d times", d, probes[d].load());

    Record r = {0, 0, 0, 0};
    const int before = probes[0].load() + probes[MSS_MAX_DEVICES - 1].load();
    CHECK(cache.get(-1, fill, &r) == MSS_ERR_UNSUPPORTED, "index -1 accepted");
    CHECK(cache.get(MSS_MAX_DEVICES, fill, &r) == MSS_ERR_UNSUPPORTED, "index %d accepted", MSS_MAX_DEVICES);
    CHECK(MSS_MAX_DEVICES == 16 && r.a == 0 && probes[0].load() + probes[MSS_MAX_DEVICES - 1].load() == before, "a refused index probed");
  }
  {
    static MssPerDevice<Record> cache;
    for (auto& p : probes) p.store(0);
    const std::vector<Tally> tally = hammer(cache, fill_failing_once);
    for (int d = 0; d < MSS_MAX_DEVICES; ++d) {
      int failed = 0;
      for (int t = 0; t < THREADS; ++t) failed += tally[t].failed[d];
      CHECK(failed == 1, "device %d: the first probe's failure was returned to %d calls", d, failed);
      CHECK(probes[d].load() == 2, "device %d probed %d times (one failure, one success)", d, probes[d].load());
    }
    for (int t = 0; t < THREADS; ++t) CHECK(tally[t].bad == 0, "thread %d: %d calls saw a cached failure or an incomplete record", t, tally[t].bad);
  }
  std::puts("ok");
  return 0;
}
