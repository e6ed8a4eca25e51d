// Who frees what in the sensor half of the library (csrc/dev_memory.hip.h's owners and the module states built on
// them) and in the marking layers' building blocks (csrc/marking_buffers.hip.h), on the CPU.  The HIP allocation calls are replaced by counting stand-ins on malloc, each of which can be told to
// fail at the k-th call of a pass.  For every state: a clean alloc + free leaves nothing live; with the failure placed
// at every call of the clean pass in turn, alloc reports failure and nothing stays live afterwards; and no pointer is
// ever freed twice, nothing unknown is freed, no memset or copy leaves its allocation.  Then the two growing helpers
// (dev_realloc, host_mapped_reserve) the same way.  The program needs no GPU: it never reaches the HIP runtime.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (++failures <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                \
  } while (0)

struct Fake {
  std::map<void*, size_t> dev, host;   // what is live, with its size
  int calls = 0, fail_at = 0;          // the fail_at-th call of a pass fails (0: none)
  int misuse = 0;                      // frees of something not live, writes beyond an allocation
  int released = 0;                    // frees of something live
  bool fails() { return ++calls == fail_at; }
  void pass(int k) { calls = 0; fail_at = k; }
  bool holds(const void* p, size_t bytes) const {
    for (const auto* m : {&dev, &host}) {
      const auto it = m->find(const_cast<void*>(p));
      if (it != m->end()) return bytes <= it->second;
    }
    return false;
  }
} fake;

hipError_t fake_alloc(std::map<void*, size_t>& live, void** p, size_t bytes) {
  *p = nullptr;
  if (fake.fails()) return hipErrorOutOfMemory;
  *p = std::malloc(std::max<size_t>(bytes, 1));
  live[*p] = bytes;
  return hipSuccess;
}
// A free that is told to fail still releases: the library ignores the result, and must not depend on it.
hipError_t fake_release(std::map<void*, size_t>& live, void* p) {
  const bool failing = fake.fails();
  if (p) {
    if (!live.erase(p)) {
      ++fake.misuse;
      return hipErrorInvalidValue;
    }
    std::free(p);
    ++fake.released;
  }
  return failing ? hipErrorInvalidValue : hipSuccess;
}
template <class T>
hipError_t fake_hipMalloc(T** p, size_t bytes) { return fake_alloc(fake.dev, reinterpret_cast<void**>(p), bytes); }
hipError_t fake_hipFree(void* p) { return fake_release(fake.dev, p); }
hipError_t fake_hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_alloc(fake.host, p, bytes); }
hipError_t fake_hipHostFree(void* p) { return fake_release(fake.host, p); }
hipError_t fake_hipHostGetDevicePointer(void** dev, void* host, unsigned) {
  *dev = nullptr;
  if (fake.fails()) return hipErrorInvalidValue;
  if (!fake.host.count(host)) {
    ++fake.misuse;
    return hipErrorInvalidValue;
  }
  *dev = host;
  return hipSuccess;
}
hipError_t fake_hipMemset(void* p, int value, size_t bytes) {
  if (fake.fails()) return hipErrorInvalidValue;
  if (!fake.holds(p, bytes)) {
    ++fake.misuse;
    return hipErrorInvalidValue;
  }
  std::memset(p, value, bytes);
  return hipSuccess;
}
hipError_t fake_hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  if (fake.fails()) return hipErrorInvalidValue;
  if (!fake.holds(dst, bytes)) {
    ++fake.misuse;
    return hipErrorInvalidValue;
  }
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}

}  // namespace

#define hipMalloc fake_hipMalloc
#define hipFree fake_hipFree
#define hipHostMalloc fake_hipHostMalloc
#define hipHostFree fake_hipHostFree
#define hipHostGetDevicePointer fake_hipHostGetDevicePointer
#define hipMemset fake_hipMemset
#define hipMemcpy fake_hipMemcpy

#include "dev_memory.hip.h"
#include "depth_clear.hip.h"
#include "depth_image.hip.h"
#include "lidar_features.hip.h"
#include "marking_buffers.hip.h"

using namespace dddmr;

namespace {

int n_states = 0, n_clean_calls = 0, n_placements = 0;

size_t live() { return fake.dev.size() + fake.host.size(); }

// alloc(state) fills the state in and allocates it, as the library's caller does; free_it(state) is the state's *_free;
// is_reset(state): the record names nothing any more.
template <class State, class Alloc, class Free, class IsReset>
void check_state(const char* name, Alloc alloc, Free free_it, IsReset is_reset) {
  ++n_states;
  int clean_calls = 0;
  {
    State s{};
    fake.pass(0);
    CHECK(alloc(s) == 0, "%s: clean alloc", name);
    clean_calls = fake.calls;
    CHECK(live() > 0 && !is_reset(s), "%s: a clean alloc holds memory", name);
    free_it(s);
    CHECK(live() == 0 && is_reset(s), "%s: %zu live after a clean free", name, live());
    free_it(s);                                        // a second free finds nothing
    CHECK(fake.misuse == 0, "%s: %d bad frees or writes in the clean pass", name, fake.misuse);
  }
  n_clean_calls += clean_calls;
  for (int k = 1; k <= clean_calls; ++k) {
    {
      State s{};
      fake.pass(k);
      CHECK(alloc(s) != 0, "%s: alloc succeeded with call %d of %d failing", name, k, clean_calls);
      fake.pass(0);
      if (k & 1) {                                     // torn down by its *_free, or by going out of scope
        free_it(s);
        CHECK(live() == 0 && is_reset(s), "%s: %zu live after call %d failed and the state was freed", name, live(), k);
      }
    }
    CHECK(live() == 0, "%s: %zu live after call %d failed and the state died", name, live(), k);
    CHECK(fake.misuse == 0, "%s: %d bad frees or writes with call %d failing", name, fake.misuse, k);
    ++n_placements;
  }
  {                                                    // a complete state that is never freed by name frees itself
    State s{};
    fake.pass(0);
    CHECK(alloc(s) == 0, "%s: clean alloc", name);
  }
  CHECK(live() == 0 && fake.misuse == 0, "%s: %zu live after a complete state died", name, live());
}

void check_states() {
  constexpr size_t kMaxPoints = 100;
  check_state<PerceptionScratch>(
      "PerceptionScratch", [&](PerceptionScratch& s) { return perception_alloc(s, kMaxPoints); }, perception_free,
      [](const PerceptionScratch& s) { return !s.counters && !s.stage && !s.res_host && !s.table.mem && s.cap_points == 0; });
  for (const bool raw_stage : {true, false})
    check_state<DepthSource>(
        raw_stage ? "DepthSource (clouds)" : "DepthSource (images)",
        [&](DepthSource& s) {
          s.max_frame_points = 50;
          s.max_frames = 2;
          return depth_alloc(s, kMaxPoints, raw_stage);
        },
        depth_free, [](const DepthSource& s) { return !s.buf[0] && !s.buf[1] && !s.surv && !s.stage && !s.res_host && s.max_frame_points == 0; });
  check_state<DepthImage>(
      "DepthImage",
      [](DepthImage& d) {
        d.p.width = d.p.cols = d.p.rows = 4;
        d.p.step = 1;
        d.height = 4;
        return dimg_alloc(d);
      },
      dimg_free, [](const DepthImage& d) { return !d.stage && !d.cloud[0] && !d.cloud[1] && !d.counters && !d.res_host && d.height == 0; });
  check_state<DepthClear>(
      "DepthClear", [&](DepthClear& d) { return dc_alloc(d, kMaxPoints, 1000); }, dc_free,
      [](const DepthClear& d) { return !d.hdr && !d.pts && !d.temp && d.temp_bytes == 0; });
  auto sweep_shape = [](LidarSweep& s) {
    s.p.V = 4;
    s.p.H = 8;
    s.max_points = 64;
  };
  auto sweep_reset = [](const LidarSweep& s) { return !s.moved && !s.obs[1] && !s.res_host && !s.feed.counters && !s.features && s.max_points == 0; };
  check_state<LidarSweep>(
      "LidarSweep",
      [&](LidarSweep& s) {
        sweep_shape(s);
        return sweep_alloc(s);
      },
      sweep_free, sweep_reset);
  auto features_shape = [](LidarFeatures& f) {
    f.p.V = 4;
    f.p.H = 8;
  };
  check_state<LidarFeatures>(
      "LidarFeatures",
      [&](LidarFeatures& f) {
        features_shape(f);
        return features_alloc(f);
      },
      features_free, [](const LidarFeatures& f) { return !f.block_cnt && !f.feat_idx[1] && !f.res_host && f.p.V == 0; });
  check_state<LidarSweep>(                             // the features live and die with their sweep
      "LidarSweep with features",
      [&](LidarSweep& s) {
        sweep_shape(s);
        if (sweep_alloc(s) != 0) return -1;
        s.features.reset(new LidarFeatures());
        features_shape(*s.features);
        return features_alloc(*s.features);
      },
      sweep_free, sweep_reset);
  // the marking layers' building blocks, at table 8, pool 4, n_ground 1, N = 2; freed by assigning an empty state
  for (const bool depth : {false, true})               // the lidar layer's store has the fov flag, the depth layer's has heads
    check_state<StoreBuf>(
        depth ? "StoreBuf (depth layer)" : "StoreBuf (lidar layer)", [&](StoreBuf& b) { return store_alloc(b, 8, 4, 4, 1, !depth, depth); },
        [](StoreBuf& b) { b = StoreBuf(); },
        [](const StoreBuf& b) { return !b.s.keys && !b.s.fov_flag && !b.head.pc_n && !b.head_alt.pc_ofs && !b.pool_alt && !b.counters && b.table == 0; });
  check_state<ClusterScratch>(
      "ClusterScratch", [](ClusterScratch& c) { return cluster_scratch_alloc(c, 2, 4096); }, [](ClusterScratch& c) { c = ClusterScratch(); },
      [](const ClusterScratch& c) { return !c.temp && !c.parent && !c.cl.vkey && !c.n_groups && c.temp_bytes == 0; });
  struct OwnedGrid {                                   // a GridBuf allocates into its user's owner
    GridBuf b;
    Owned mem;
  };
  check_state<OwnedGrid>(
      "GridBuf", [](OwnedGrid& g) { return grid_alloc(g.mem.dev, g.b, 8, 2); }, [](OwnedGrid& g) { g = OwnedGrid(); },
      [](const OwnedGrid& g) { return !g.b.g.cell_start && !g.b.g.sorted && g.b.cap_cells == 0; });
}

// dev_realloc: grow, grow with every call of the grow failing in turn, free
void check_dev_realloc() {
  int grow_calls = 0;
  for (int k = 0; k <= grow_calls; ++k) {
    DevAllocs owner;
    float4* p = nullptr;
    float* other = nullptr;
    fake.pass(0);
    CHECK(dev_alloc(owner, &other, 3) == hipSuccess && dev_realloc(owner, &p, 10) == hipSuccess && p && owner.size() == 2, "dev_realloc: first allocation");
    void* const old = p;                               // (malloc may hand the same address out again)
    const int released = fake.released;
    fake.pass(k);
    const hipError_t e = dev_realloc(owner, &p, 100);
    if (k == 0) grow_calls = fake.calls;
    fake.pass(0);
    CHECK(fake.released == released + 1 && (p == old || (!fake.dev.count(old) && std::find(owner.begin(), owner.end(), old) == owner.end())),
          "dev_realloc: the old buffer is gone (k = %d)", k);
    if (e == hipSuccess) {
      CHECK(p && fake.dev.count(p) && fake.dev[p] == 100 * sizeof(float4) && owner.size() == 2, "dev_realloc: grown (k = %d)", k);
    } else {
      CHECK(k > 0 && p == nullptr && owner.size() == 1 && fake.dev.size() == 1, "dev_realloc: a failed grow leaves null and only the other buffer (k = %d)", k);
    }
    dev_free(owner);
    CHECK(live() == 0 && owner.empty() && fake.misuse == 0, "dev_realloc: %zu live after dev_free (k = %d)", live(), k);
    ++n_placements;
  }
  CHECK(grow_calls == 2, "dev_realloc: a grow is one free and one allocation, not %d calls", grow_calls);
}

// host_mapped_reserve: grow from nothing, no call within the capacity, grow with every call failing in turn, free
void check_host_reserve() {
  int grow_calls = 0;
  for (int k = 0; k <= grow_calls; ++k) {
    HostAllocs owner;
    void *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    fake.pass(0);
    CHECK(host_mapped_reserve(owner, &host, &dev, &cap, (size_t)100) == 0 && host && dev == host && cap == (1u << 16), "host_mapped_reserve: first");
    const int calls = fake.calls;
    CHECK(host_mapped_reserve(owner, &host, &dev, &cap, (size_t)1 << 16) == 0 && fake.calls == calls, "host_mapped_reserve: within the capacity");
    void* const old = host;                            // (malloc may hand the same address out again)
    const int released = fake.released;
    fake.pass(k);
    const int rc = host_mapped_reserve(owner, &host, &dev, &cap, (size_t)100000);
    if (k == 0) grow_calls = fake.calls;
    fake.pass(0);
    CHECK(fake.released == released + (rc == 0 || k < 3 ? 1 : 2) &&
              (host == old || (!fake.host.count(old) && std::find(owner.mem.begin(), owner.mem.end(), old) == owner.mem.end())),
          "host_mapped_reserve: the old buffer is gone (k = %d)", k);
    if (rc == 0) {
      CHECK(host && dev == host && cap == (1u << 17) && fake.host.count(host) && fake.host[host] == cap && owner.mem.size() == 1, "host_mapped_reserve: grown (k = %d)", k);
    } else {
      CHECK(k > 0 && !host && !dev && cap == 0 && owner.mem.empty() && fake.host.empty(), "host_mapped_reserve: a failed grow leaves null (k = %d)", k);
    }
    host_free(owner);
    CHECK(live() == 0 && owner.mem.empty() && fake.misuse == 0, "host_mapped_reserve: %zu live after host_free (k = %d)", live(), k);
    ++n_placements;
  }
  CHECK(grow_calls == 3, "host_mapped_reserve: a grow is a free, an allocation and a device address, not %d calls", grow_calls);
}

}  // namespace

int main() {
  check_states();
  check_dev_realloc();
  check_host_reserve();
  if (failures) {
    std::printf("source memory: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("source memory OK: %d states, %d calls in their clean passes, %d failure placements\n", n_states, n_clean_calls, n_placements);
  return 0;
}
