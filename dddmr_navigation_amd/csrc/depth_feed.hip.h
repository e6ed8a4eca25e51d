// depth_feed.hip.h -- local-mode feed of the depth camera layer as HIP kernels.
//
// Replaces DepthCameraObservationBuffer::bufferCloud
// (dddmr_perception_3d/plugins/depth_camera/depth_camera_observation_buffer.cpp:78-187) for the
// local planner, per frame: sensor->base transform (:105-107), the obstacle-height band on the
// float z (:109-120), only above 20000 survivors a 0.05 m VoxelGrid centroid downsample in the
// base frame (:123-131), base->global transform (:177-178).  The frustum the same function builds
// is read by the global-mode selfClear only and is not computed here.
//
// Two launches on one stream, one host wait:
//   k_depth_insert  raw records (pinned, read over PCIe once) -> base-frame survivors, compacted on the
//                   device with one counter add per wave (the survivor count is exact), and in the same
//                   pass their 0.05 m voxel sums into the hash table: the PCIe reads bound this kernel, the
//                   table updates ride behind them.  Which branch the frame ends on is not known before the
//                   last workgroup has counted, so the sums are built either way; a frame of at most 20000
//                   survivors wastes at most 20000 table updates.
//   k_depth_emit    reads the count and decides.  <= 20000: global transform, one store per survivor, the
//                   claimed slots cleaned.  > 20000: one lane per claimed voxel: centroid, global
//                   transform, append, slot cleaned.  The last workgroup hands the counts to the host.
// One table update per point, as k_feed_insert: a variant that first summed the runs of equal keys among the
// consecutive lanes of a wave (segmented shuffle reduction, one update per run) was measured beside it and
// did not win outside the spread (profiles/r04_depth_feed.json), so the simpler kernel stays.
//
// Voxel membership is PCL's floor(p * inverse_leaf) per axis in float with inverse_leaf =
// 1.0f / 0.05f (= 20.0f exactly); centroid sums are double (PCL sums in float in input order, so
// 1e-5 m is the meaningful agreement, as for the lidar feed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "perception_kernels.hip.h"

// Nothing may be fused: the reference is an x86-64 build without FMA contraction.
#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kDepthVoxelizeAbove = 20000;   // depth_camera_observation_buffer.cpp:124
constexpr unsigned kDepthEmitBlocks = 512;        // k_depth_emit's grid: 2 workgroups per CU, grid-stride

struct DepthParams {
  double Rbs[9], tbs[3];   // base <- sensor
  double Rgb[9], tgb[3];   // global <- base
  double zmin, zmax;       // min_obstacle_height_, max_obstacle_height_ (doubles in the reference)
  int n;                   // raw records of the frame
};

struct DepthResult {         // host-mapped, written by the last k_depth_emit workgroup
  uint32_t n_survivors;      // points inside the height band
  uint32_t n_out;            // points of the frame's observation
  uint32_t seq;              // stored last (system-scope release); the host polls it
  uint32_t pad;
};

struct DepthFrame {
  uint32_t n;                // points of the observation
  int64_t stamp_us;          // pcl_conversions::toPCL: whole microseconds
};

struct DepthSource {
  double zmin = 0, zmax = 0;
  int64_t persistence_ns = 0;
  uint32_t max_frame_points = 0, max_frames = 0;
  // the alive observations, oldest first, packed in buf[cur]; a frame that makes older ones leave is
  // built in buf[cur ^ 1] behind a device-to-device copy of the ones that stay, then the two swap
  float4* buf[2] = {nullptr, nullptr};
  int cur = 0;
  std::vector<DepthFrame> frames;
  // per-frame scratch
  float* stage = nullptr;              // pinned + mapped: the raw records
  float* stage_dev = nullptr;
  float4* surv = nullptr;              // base-frame survivors of the frame
  uint32_t* claimed = nullptr;
  unsigned char* table = nullptr;      // [keys 8B | sums 3x8B | counts 4B] x slots; k_depth_emit leaves it clean
  uint32_t* counters = nullptr;        // [0] survivors, [1] ticket, [2] claimed slots, [3] emitted
  DepthResult* res_host = nullptr;
  DepthResult* res_dev = nullptr;
  size_t cap_slots = 0;
  uint32_t seq = 0;
};

__device__ __forceinline__ unsigned long long depth_voxel_key(float x, float y, float z) {
  // pcl::VoxelGrid: ijk = floor(p * inverse_leaf_size); leaf 0.05f -> inverse 20.0f
  const float inv_leaf = 1.0f / 0.05f;
  const int ix = (int)floorf(x * inv_leaf), iy = (int)floorf(y * inv_leaf), iz = (int)floorf(z * inv_leaf);
  return (1ull << 63) | ((unsigned long long)((uint32_t)(ix + (1 << 20)) & 0x1FFFFFu) << 42) |
         ((unsigned long long)((uint32_t)(iy + (1 << 20)) & 0x1FFFFFu) << 21) |
         (unsigned long long)((uint32_t)(iz + (1 << 20)) & 0x1FFFFFu);
}

// One raw record per lane (valid = the lane has one), every lane of the wave calls it: bufferCloud's transform and
// height band, the wave-aggregated append of the survivors and their voxel sums.  The body of k_depth_insert; the depth
// image path (depth_image.hip.h) calls it on its stage-one centroids.
__device__ __forceinline__ void depth_insert_record(const DepthParams& f, bool valid, float sx, float sy, float sz,
                                                    float4* __restrict__ surv, unsigned long long* __restrict__ keys,
                                                    double* __restrict__ sums, uint32_t* __restrict__ counts,
                                                    uint32_t slot_mask, uint32_t* __restrict__ claimed,
                                                    uint32_t* __restrict__ counters) {
  bool keep = false;
  float x = 0.f, y = 0.f, z = 0.f;
  if (valid && isfinite(sx) && isfinite(sy) && isfinite(sz)) {
    // pcl::transformPointCloud(cloud, cloud, Affine3d): double multiply-add, float result
    x = (float)(f.Rbs[0] * sx + f.Rbs[1] * sy + f.Rbs[2] * sz + f.tbs[0]);
    y = (float)(f.Rbs[3] * sx + f.Rbs[4] * sy + f.Rbs[5] * sz + f.tbs[1]);
    z = (float)(f.Rbs[6] * sx + f.Rbs[7] * sy + f.Rbs[8] * sz + f.tbs[2]);
    keep = (double)z <= f.zmax && (double)z >= f.zmin;
  }
  // wave-aggregated append of the survivors: one atomic per wave, lanes keep their pixel order
  const unsigned long long mask = __ballot(keep);
  if (!mask) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(&counters[0], (uint32_t)__popcll(mask));
  base = __shfl(base, leader, 64);
  if (keep) surv[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = make_float4(x, y, z, 0.f);
  // the voxel sums, whichever branch the frame ends on (the count is not known before the last workgroup
  // has run; a frame of at most 20000 survivors wastes at most 20000 inserts, hidden behind the PCIe reads)
  if (!keep) return;
  const unsigned long long key = depth_voxel_key(x, y, z);
  uint32_t slot = hash_key(key) & slot_mask;
  for (uint32_t probe = 0; probe <= slot_mask; ++probe) {
    const unsigned long long prev = atomicCAS(&keys[slot], 0ull, key);
    if (prev == 0ull || prev == key) {
      if (prev == 0ull) claimed[atomicAdd(&counters[2], 1u)] = slot;   // first of a voxel: list its slot for the emit pass
      atomicAdd(&sums[3 * (size_t)slot + 0], (double)x);
      atomicAdd(&sums[3 * (size_t)slot + 1], (double)y);
      atomicAdd(&sums[3 * (size_t)slot + 2], (double)z);
      atomicAdd(&counts[slot], 1u);
      return;
    }
    slot = (slot + 1) & slot_mask;
  }
}

__global__ __launch_bounds__(256) void k_depth_insert(DepthParams f, const float* __restrict__ raw, int stride_floats,
                                                      float4* __restrict__ surv, unsigned long long* __restrict__ keys,
                                                      double* __restrict__ sums, uint32_t* __restrict__ counts,
                                                      uint32_t slot_mask, uint32_t* __restrict__ claimed,
                                                      uint32_t* __restrict__ counters) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < f.n;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (valid) {
    const float* sp = raw + (size_t)i * stride_floats;
    sx = sp[0], sy = sp[1], sz = sp[2];
  }
  depth_insert_record(f, valid, sx, sy, sz, surv, keys, sums, counts, slot_mask, claimed, counters);
}

// Grid-stride over max(survivors, claimed slots): the branch is decided here, from the device's own count.
__global__ __launch_bounds__(256) void k_depth_emit(DepthParams f, const float4* __restrict__ surv,
                                                    unsigned long long* __restrict__ keys, double* __restrict__ sums,
                                                    uint32_t* __restrict__ counts, const uint32_t* __restrict__ claimed,
                                                    float4* __restrict__ out, uint32_t* __restrict__ counters,
                                                    DepthResult* __restrict__ res, uint32_t seq) {
  const uint32_t n_surv = counters[0], n_claimed = counters[2];
  const bool voxelise = n_surv > kDepthVoxelizeAbove;
  const uint32_t work = voxelise ? n_claimed : max(n_surv, n_claimed);
  const int lane = threadIdx.x & 63;
  for (uint32_t idx0 = blockIdx.x * blockDim.x; idx0 < work; idx0 += gridDim.x * blockDim.x) {   // uniform per workgroup
    const uint32_t idx = idx0 + threadIdx.x;
    const bool occ = idx < n_claimed;
    const uint32_t slot = occ ? claimed[idx] : 0u;
    if (voxelise) {
      // one lane per occupied voxel, wave-aggregated append
      const unsigned long long mask = __ballot(occ);
      uint32_t base = 0;
      if (mask) {
        const int leader = __ffsll((long long)mask) - 1;
        if (lane == leader) base = atomicAdd(&counters[3], (uint32_t)__popcll(mask));
        base = __shfl(base, leader, 64);
      }
      if (occ) {
        const double n = (double)counts[slot];
        const float cx = (float)(sums[3 * (size_t)slot + 0] / n);
        const float cy = (float)(sums[3 * (size_t)slot + 1] / n);
        const float cz = (float)(sums[3 * (size_t)slot + 2] / n);
        out[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] =
            make_float4((float)(f.Rgb[0] * cx + f.Rgb[1] * cy + f.Rgb[2] * cz + f.tgb[0]),
                        (float)(f.Rgb[3] * cx + f.Rgb[4] * cy + f.Rgb[5] * cz + f.tgb[1]),
                        (float)(f.Rgb[6] * cx + f.Rgb[7] * cy + f.Rgb[8] * cz + f.tgb[2]), 0.f);
      }
    } else if (idx < n_surv) {
      // the points pass unchanged: base -> global
      const float4 p = surv[idx];
      out[idx] = make_float4((float)(f.Rgb[0] * p.x + f.Rgb[1] * p.y + f.Rgb[2] * p.z + f.tgb[0]),
                             (float)(f.Rgb[3] * p.x + f.Rgb[4] * p.y + f.Rgb[5] * p.z + f.tgb[1]),
                             (float)(f.Rgb[6] * p.x + f.Rgb[7] * p.y + f.Rgb[8] * p.z + f.tgb[2]), 0.f);
    }
    if (occ) {
      // leave the table empty for the next frame
      keys[slot] = 0ull;
      sums[3 * (size_t)slot + 0] = 0.0;
      sums[3 * (size_t)slot + 1] = 0.0;
      sums[3 * (size_t)slot + 2] = 0.0;
      counts[slot] = 0u;
    }
  }
  // last workgroup publishes the counts to the host (device-scope ticket; the counters are
  // only touched by device-scope atomics)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add(&counters[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == gridDim.x - 1) {
      const uint32_t emitted = __hip_atomic_load(&counters[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      res->n_survivors = n_surv;
      res->n_out = voxelise ? emitted : n_surv;
      counters[0] = 0;         // next frame
      counters[1] = 0;
      counters[2] = 0;
      counters[3] = 0;
      __threadfence_system();
      __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

inline void depth_free(DepthSource& s) {
  for (float4* b : s.buf)
    if (b) (void)hipFree(b);
  if (s.surv) (void)hipFree(s.surv);
  if (s.claimed) (void)hipFree(s.claimed);
  if (s.table) (void)hipFree(s.table);
  if (s.counters) (void)hipFree(s.counters);
  if (s.res_host) (void)hipHostFree(s.res_host);
  if (s.stage) (void)hipHostFree(s.stage);
  s = DepthSource();
}

// max_points bounds what the source may publish; a frame under construction sits behind it.  raw_stage = false: a
// source fed depth images, which stages those itself (depth_image.hip.h)
inline int depth_alloc(DepthSource& s, size_t max_points, bool raw_stage = true) {
  const size_t F = s.max_frame_points;
  size_t slots = 1024;
  while (slots < 2 * F) slots <<= 1;
  s.cap_slots = slots;
  for (float4*& b : s.buf)
    if (hipMalloc(&b, (max_points + F) * sizeof(float4)) != hipSuccess) return -1;
  if (hipMalloc(&s.surv, F * sizeof(float4)) != hipSuccess) return -1;
  if (hipMalloc(&s.claimed, F * sizeof(uint32_t)) != hipSuccess) return -1;
  if (hipMalloc(&s.table, feed_table_bytes(slots)) != hipSuccess) return -1;
  if (hipMalloc(&s.counters, 4 * sizeof(uint32_t)) != hipSuccess) return -1;
  if (hipMemset(s.table, 0, feed_table_bytes(slots)) != hipSuccess) return -1;   // k_depth_emit keeps it clean afterwards
  if (hipMemset(s.counters, 0, 4 * sizeof(uint32_t)) != hipSuccess) return -1;
  if (hipHostMalloc(&s.res_host, sizeof(DepthResult), hipHostMallocMapped) != hipSuccess) return -1;
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&s.res_dev), s.res_host, 0) != hipSuccess) return -1;
  // k_depth_transform reads the raw frame straight from this pinned, device-mapped buffer
  if (raw_stage) {
    if (hipHostMalloc(&s.stage, F * 4 * sizeof(float), hipHostMallocMapped) != hipSuccess) return -1;
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&s.stage_dev), s.stage, 0) != hipSuccess) return -1;
  }
  std::memset(s.res_host, 0, sizeof(DepthResult));
  return 0;
}

// One frame through the three kernels into out_dev (room for max_frame_points points); f.n <= max_frame_points.
inline int depth_feed(DepthSource& s, DepthParams f, const float* raw, size_t stride_bytes, float4* out_dev,
                      hipStream_t stream, uint32_t* n_out) {
  *n_out = 0;
  if (f.n == 0) return 0;
  int stride_floats;
  if (stride_bytes == 12 || stride_bytes == 16) {
    stride_floats = (int)(stride_bytes / 4);
    std::memcpy(s.stage, raw, (size_t)f.n * stride_bytes);
  } else {                                    // wider records (PCL: 32 bytes) are narrowed on the way
    stride_floats = 3;
    const size_t sf = stride_bytes / 4;
    for (size_t i = 0; i < (size_t)f.n; ++i) {
      s.stage[3 * i + 0] = raw[i * sf + 0];
      s.stage[3 * i + 1] = raw[i * sf + 1];
      s.stage[3 * i + 2] = raw[i * sf + 2];
    }
  }
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(s.table);
  double* sums = reinterpret_cast<double*>(s.table + s.cap_slots * 8);
  uint32_t* counts = reinterpret_cast<uint32_t*>(s.table + s.cap_slots * 32);
  const uint32_t seq = ++s.seq ? s.seq : ++s.seq;
  // table of this frame: the first `slots` entries, load <= 0.5 even if every record survives in a voxel of its own
  size_t slots = 1024;
  while (slots < 2 * (size_t)f.n) slots <<= 1;
  if (slots > s.cap_slots) return -2;
  const dim3 grid((unsigned)((f.n + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_depth_insert, grid, block, 0, stream, f, s.stage_dev, stride_floats, s.surv, keys, sums, counts,
                     (uint32_t)(slots - 1), s.claimed, s.counters);
  // survivors and voxels are a fraction of the raw records: a fixed grid walks them
  const dim3 emit_grid(std::min<unsigned>(grid.x, kDepthEmitBlocks));
  hipLaunchKernelGGL(k_depth_emit, emit_grid, block, 0, stream, f, s.surv, keys, sums, counts, s.claimed, out_dev, s.counters,
                     s.res_dev, seq);
  if (hipGetLastError() != hipSuccess) return -5;
  // the device chose the branch from its own count; the host waits once, for the last kernel's word
  volatile uint32_t* seq_p = &s.res_host->seq;
  bool seen = false;
  for (uint64_t spins = 0; spins < (1ull << 26); ++spins) {
    if (*seq_p == seq) { seen = true; break; }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  if (!seen && hipStreamSynchronize(stream) != hipSuccess) return -4;
  *n_out = s.res_host->n_out;
  return 0;
}

}  // namespace dddmr
