// voxel_table.hip.h -- the voxel-sum hash table the feeds share, and the small device and host helpers around it.
//
// The lidar feed (perception_kernels.hip.h), the depth cloud feed (depth_feed.hip.h) and the depth image path
// (depth_image.hip.h) all restate pcl::VoxelGrid the same way: a point's voxel is floor(p * inverse_leaf) per axis
// in float, the voxel's centroid is the mean of its points.  This header is the only place that knows how that is
// kept on the device:
//   layout    [keys 8B | sums 3x8B | counts 4B] x slots in one allocation, open addressing with linear probing;
//   key       bit 63 set, 21 bits per axis, offset 2^20; 0 is an empty slot;
//   protocol  an insert claims a slot with one CAS and lists it in `claimed`; the emit pass walks that list (one lane
//             per occupied voxel, not per slot) and zeroes what it reads, so a table is empty again after every call
//             and is only ever memset once, when it is allocated.
// The marking layer's persistent store (marking.hip.h) has its own table and shares the key and the hash only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <type_traits>
#include <vector>

// The reference is an x86-64 build without FMA contraction: every multiply and add below
// rounds separately, in float and in double (hipcc's default would fuse them).
#pragma clang fp contract(off)

namespace dddmr {

// ---------------------------------------------------------------------------
// key and hash
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long voxel_key(int x, int y, int z) {   // bit 63 set: 0 = empty slot
  return (1ull << 63) | ((unsigned long long)((uint32_t)(x + (1 << 20)) & 0x1FFFFFu) << 42) |
         ((unsigned long long)((uint32_t)(y + (1 << 20)) & 0x1FFFFFu) << 21) |
         (unsigned long long)((uint32_t)(z + (1 << 20)) & 0x1FFFFFu);
}
__host__ __device__ __forceinline__ void voxel_unkey(unsigned long long key, int* x, int* y, int* z) {
  *x = (int)((key >> 42) & 0x1FFFFFu) - (1 << 20);
  *y = (int)((key >> 21) & 0x1FFFFFu) - (1 << 20);
  *z = (int)(key & 0x1FFFFFu) - (1 << 20);
}
// pcl::VoxelGrid: ijk = floor(p * inverse_leaf_size), in float
__device__ __forceinline__ unsigned long long voxel_key(float x, float y, float z, float inv_leaf) {
  return voxel_key((int)floorf(x * inv_leaf), (int)floorf(y * inv_leaf), (int)floorf(z * inv_leaf));
}
__device__ __forceinline__ uint32_t voxel_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

// ---------------------------------------------------------------------------
// the table on the device
// ---------------------------------------------------------------------------
struct VoxelView {             // passed to kernels by value
  unsigned long long* keys;    // [mask + 1]
  double* sums;                // [3 x (mask + 1)]
  uint32_t* counts;            // [mask + 1]
  uint32_t* claimed;           // the slots claimed since the table was last empty, in claim order
  uint32_t* n_claimed;         // how many: an entry of the user's own counter array
  uint32_t mask;               // slots this call uses - 1
};

// Adds n points of one voxel with the sums (sx, sy, sz).  All-zero sums add the count only (x + 0.0 == x).
__device__ __forceinline__ void voxel_insert(const VoxelView& t, unsigned long long key, double sx, double sy, double sz,
                                             uint32_t n) {
  uint32_t slot = voxel_hash(key) & t.mask;
  for (uint32_t probe = 0; probe <= t.mask; ++probe) {
    const unsigned long long prev = atomicCAS(&t.keys[slot], 0ull, key);
    if (prev == 0ull || prev == key) {
      if (prev == 0ull) t.claimed[atomicAdd(t.n_claimed, 1u)] = slot;   // first of a voxel: list its slot for the emit pass
      if (!(sx == 0.0 && sy == 0.0 && sz == 0.0)) {
        atomicAdd(&t.sums[3 * (size_t)slot + 0], sx);
        atomicAdd(&t.sums[3 * (size_t)slot + 1], sy);
        atomicAdd(&t.sums[3 * (size_t)slot + 2], sz);
      }
      atomicAdd(&t.counts[slot], n);
      return;
    }
    slot = (slot + 1) & t.mask;
  }
}

// leaves a claimed slot empty for the next call (saves a memset of the whole table per call)
__device__ __forceinline__ void voxel_clean(const VoxelView& t, uint32_t slot) {
  t.keys[slot] = 0ull;
  t.sums[3 * (size_t)slot + 0] = 0.0;
  t.sums[3 * (size_t)slot + 1] = 0.0;
  t.sums[3 * (size_t)slot + 2] = 0.0;
  t.counts[slot] = 0u;
}

// the float centroid of a claimed slot; the slot is left empty
__device__ __forceinline__ float3 voxel_take(const VoxelView& t, uint32_t slot) {
  const double n = (double)t.counts[slot];
  const float3 c = make_float3((float)(t.sums[3 * (size_t)slot + 0] / n), (float)(t.sums[3 * (size_t)slot + 1] / n),
                               (float)(t.sums[3 * (size_t)slot + 2] / n));
  voxel_clean(t, slot);
  return c;
}

// ---------------------------------------------------------------------------
// wave and workgroup helpers
// ---------------------------------------------------------------------------
// Wave-aggregated append, every lane of the wave calls it: one atomic per wave, the keeping lanes stay in lane order.
// Returns the lane's output index (meaningless where !keep).
__device__ __forceinline__ uint32_t wave_append(bool keep, uint32_t* counter) {
  const unsigned long long mask = __ballot(keep);
  if (!mask) return 0u;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
  base = __shfl(base, leader, 64);
  return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// Every thread of every workgroup calls it once, after its last write.  True in thread 0 of the workgroup that
// finishes last, which then sees what all the others wrote with device-scope atomics (device-scope ticket).
__device__ __forceinline__ bool last_block(uint32_t* ticket) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x != 0) return false;
  return __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
}

// pcl::transformPointCloud(cloud, cloud, Affine3d): double multiply-add, float result
__device__ __forceinline__ float3 affine_to_float(const double R[9], const double t[3], float x, float y, float z) {
  return make_float3((float)(R[0] * x + R[1] * y + R[2] * z + t[0]), (float)(R[3] * x + R[4] * y + R[5] * z + t[1]),
                     (float)(R[6] * x + R[7] * y + R[8] * z + t[2]));
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// slots for n keys at load <= 0.5, a power of two
inline size_t voxel_slots_for(size_t n) {
  size_t slots = 1024;
  while (slots < 2 * n) slots <<= 1;
  return slots;
}

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

struct VoxelTable {
  unsigned char* mem = nullptr;   // the layout above over `slots` entries; a call may use only the first of them
  uint32_t* claimed = nullptr;    // [max_keys]
  size_t slots = 0;

  int alloc(DevAllocs& owner, size_t max_keys) {    // room for max_keys voxels; empty, and the emit passes keep it so
    slots = voxel_slots_for(max_keys);
    if (dev_alloc(owner, &claimed, max_keys) != hipSuccess) return -1;
    return dev_alloc_zeroed(owner, &mem, slots * (8 + 24 + 4) + 64) == hipSuccess ? 0 : -1;
  }
  // the first use_slots (<= slots, a power of two) entries; counter = where this user counts its claimed slots
  VoxelView view(size_t use_slots, uint32_t* counter) const {
    return VoxelView{reinterpret_cast<unsigned long long*>(mem), reinterpret_cast<double*>(mem + slots * 8),
                     reinterpret_cast<uint32_t*>(mem + slots * 32), claimed, counter, (uint32_t)(use_slots - 1)};
  }
};

// n records (stride_bytes apart, x y z first) narrowed to packed xyz
inline void pack_xyz_records(float* dst, const float* src, size_t n, size_t stride_bytes) {
  const size_t sf = stride_bytes / 4;
  for (size_t i = 0; i < n; ++i) {
    dst[3 * i + 0] = src[i * sf + 0];
    dst[3 * i + 1] = src[i * sf + 1];
    dst[3 * i + 2] = src[i * sf + 2];
  }
}

// Stages the caller's records for a kernel: 12- and 16-byte records go as they are, wider ones (PCL: 32 bytes) are
// narrowed to 12 bytes on the way.  Returns the staged records' stride in floats.
inline int stage_xyz_records(float* dst, const float* src, size_t n, size_t stride_bytes) {
  if (stride_bytes == 12 || stride_bytes == 16) {
    std::memcpy(dst, src, n * stride_bytes);
    return (int)(stride_bytes / 4);
  }
  pack_xyz_records(dst, src, n, stride_bytes);
  return 3;
}

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
