// voxel_table.hip.h -- the voxel-sum hash table the feeds share: the key, the hash, the view a kernel gets, the insert and
// emit helpers, VoxelTable on the host, and the feeds' double-precision affine transform.
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

#include "dev_memory.hip.h"   // DevAllocs, dev_alloc: VoxelTable::alloc

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

}  // namespace dddmr
