// dev_memory.hip.h -- who owns device and pinned host memory, and how a call waits: the owners every allocation of the
// library is recorded in, the Drain guard of the error exits, and the bounded spin on a result's sequence word behind a
// feed.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <vector>

namespace dddmr {

// Who owns device memory: the context (rollout_engine.hip), the marking store and every module state record what they
// allocate in a DevAllocs of their own, where it is made; the context's teardown walks its vector, a state's Owned (below)
// walks its own when the state dies.  (Swapping a main array with its _alt array leaves the set of pointers as it is.)
// hipMalloc / hipFree and their pinned-host kin are called here and nowhere else in the library.
using DevAllocs = std::vector<void*>;
template <class T>
inline hipError_t dev_alloc(DevAllocs& owner, T** p, size_t count) {
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
  if (e == hipSuccess) owner.push_back(*p);
  return e;
}
template <class T>
inline hipError_t dev_alloc_zeroed(DevAllocs& owner, T** p, size_t count) {
  const hipError_t e = dev_alloc(owner, p, count);
  return e != hipSuccess ? e : hipMemset(*p, 0, count * sizeof(T));
}
inline void dev_free(DevAllocs& owner) {
  for (void* q : owner) (void)hipFree(q);
  owner.clear();
}
// A buffer that grows, or comes back after its user was torn down: the owner drops and frees what *p names (nothing when
// it is null), then allocates `count` elements afresh.  On failure *p is null.
template <class T>
inline hipError_t dev_realloc(DevAllocs& owner, T** p, size_t count) {
  owner.erase(std::remove(owner.begin(), owner.end(), static_cast<void*>(*p)), owner.end());
  (void)hipFree(*p);
  *p = nullptr;
  return dev_alloc(owner, p, count);
}
// The temporaries of one call: freed on any return.  (Lives on the stack, never copied.)
struct DevScope {
  DevAllocs mem;
  ~DevScope() { dev_free(mem); }
};

// Pinned host memory has owners of the same kind (a type of its own: a host pointer never lands in a DevAllocs).
struct HostAllocs { std::vector<void*> mem; };
template <class T>
inline hipError_t host_alloc(HostAllocs& owner, T** host, size_t bytes, unsigned flags = hipHostMallocDefault) {
  const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(host), bytes, flags);
  if (e == hipSuccess) owner.mem.push_back(*host);
  return e;
}
// pinned host memory the device reads and writes in place
template <class T>
inline int host_mapped_alloc(HostAllocs& owner, T** host, T** dev, size_t bytes) {
  if (host_alloc(owner, host, bytes, hipHostMallocMapped) != hipSuccess) return -1;
  return hipHostGetDevicePointer(reinterpret_cast<void**>(dev), *host, 0) == hipSuccess ? 0 : -1;
}
inline void host_free(HostAllocs& owner) {
  for (void* q : owner.mem) (void)hipHostFree(q);
  owner.mem.clear();
}
// the owner frees what *host names, if it is one of its own, and forgets it; *host is null afterwards
template <class T>
inline void host_drop(HostAllocs& owner, T** host) {
  const auto it = std::find(owner.mem.begin(), owner.mem.end(), static_cast<void*>(*host));
  if (it != owner.mem.end()) {
    (void)hipHostFree(*it);
    owner.mem.erase(it);
  }
  *host = nullptr;
}
// A mapped staging buffer that grows: afterwards it holds at least `bytes` (*cap, doubled from 64 KiB).  dev_realloc's
// rule: the owner drops and frees the old buffer first; on failure *host and *dev are null and *cap is 0.  The device
// must be done with the old buffer: the callers' calls each end with a wait.
template <class T>
inline int host_mapped_reserve(HostAllocs& owner, T** host, T** dev, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return 0;
  size_t want = std::max<size_t>(*cap, 1u << 16);
  while (want < bytes) want <<= 1;
  host_drop(owner, host);
  *cap = 0;
  if (host_mapped_alloc(owner, host, dev, want) == 0) { *cap = want; return 0; }
  host_drop(owner, host);          // (pinned but without a device address: not kept)
  *dev = nullptr;
  return -1;
}

// What a module state owns, in both kinds of memory.  A state holds one as a member and fills it where it allocates; the
// state cannot be copied, frees what it owns when it dies, and `state = State()` frees and resets it in one go.
struct Owned {
  DevAllocs dev;
  HostAllocs host;
  Owned() = default;
  Owned& operator=(Owned&& o) noexcept { release(); dev.swap(o.dev); host.mem.swap(o.host.mem); return *this; }
  ~Owned() { release(); }
  void release() { dev_free(dev); host_free(host); }
};

// The deleter of a unique_ptr that is declared where the state's type is still incomplete (the context's module slots, a
// sweep's features, the localiser's observation): instantiated at the end of the translation unit, which must have
// included the state's header by then.
template <class T>
struct LateDelete {
  void operator()(T* p) const {
    static_assert(sizeof(T) > 0, "the state's header has to be included before the end of the translation unit");
    delete p;
  }
};

// An error return may leave work enqueued that reads a pinned cloud buffer: while armed, the guard waits for the stream
// when it goes out of scope, so that a CloudPin declared BEFORE it releases a buffer nothing reads any more and the next
// call finds the stream idle.  Disarmed where the function has waited itself or handed the pin to the pending tick.
struct Drain {
  hipStream_t st;
  bool armed = true;
  ~Drain() { if (armed) (void)hipStreamSynchronize(st); }
};

// Bounded spin on a host-mapped word that a kernel stores last with a system-scope release.  True when the word was
// seen: what the kernel wrote before it may then be read.  False: the caller falls back to its stream synchronise.
inline bool wait_seq(volatile uint32_t* word, uint32_t seq) {
  bool seen = false;
  for (uint64_t spins = 0; spins < (1ull << 26); ++spins) {
    if (*word == seq) { seen = true; break; }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return seen;
}
// the next value of a state's sequence word: never 0, which a freshly allocated result record holds
inline uint32_t next_seq(uint32_t& seq) { return ++seq ? seq : ++seq; }
// The tail of a feed, behind its last launch: -5 when a launch failed, once what was enqueued before it has drained;
// otherwise the call's one host wait, the bounded spin on the result's word and then the stream: -4 when that fails.
// *waits, when given, grows by the waits made: one, two when the spin ran out.
inline int feed_wait(hipStream_t stream, volatile uint32_t* word, uint32_t seq, uint32_t* waits = nullptr) {
  if (hipGetLastError() != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    return -5;
  }
  if (waits) ++*waits;
  if (wait_seq(word, seq)) return 0;
  if (waits) ++*waits;
  return hipStreamSynchronize(stream) != hipSuccess ? -4 : 0;
}

}  // namespace dddmr
