// perception_kernels.hip.h -- local-mode perception feed as a HIP voxel-hash.
//
// Replaces MultiLayerSpinningLidar::cbSensor
// (dddmr_perception_3d/plugins/multilayer_spinning_lidar.cpp:177-281) for the
// local planner: sensor->base transform (:232-233), PassThrough crop
// |x|,|y| <= window, 0 <= z <= marking_height (:240-251), VoxelGrid centroid
// downsample with a 0.1 m leaf (:253-256), base->global transform (:264-269).
// The result is written straight into the context's aggregate-observation
// buffer (StackedPerception::aggregateObservations, src/stacked_perception.cpp:128-140)
// so the scorer's binning pass reads it without a host round trip.
//
// Voxel membership is PCL's: voxel = floor(p * (1/leaf)) per axis in float.  The
// per-voxel centroid is accumulated with double atomics (PCL accumulates in
// float in an unspecified order, so only ~1e-6 agreement is meaningful).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <deque>

#include "dev_memory.hip.h"        // Owned, host_mapped_alloc, feed_wait
#include "point_grid_plan.hip.h"   // pack_xyz_records, stage_xyz_records
#include "voxel_table.hip.h"
#include "wave_ops.hip.h"          // wave_append, last_block

// The reference is an x86-64 build without FMA contraction: every multiply and add below
// rounds separately, in float and in double (hipcc's default would fuse them).
#pragma clang fp contract(off)

namespace dddmr {

struct FeedParams {
  double Rbs[9], tbs[3];  // base <- sensor
  double Rgb[9], tgb[3];  // global <- base
  int n;
  float window;           // perception_window_size_
  float height;           // marking_height_
};

struct FeedResult {          // host-mapped: written by the last k_feed_emit workgroup
  uint32_t n_out;
  uint32_t seq;              // stored last (system-scope release); the host polls it
};

struct PerceptionScratch {
  float* stage_dev = nullptr;          // device address of `stage` (raw scan records, stride_floats apart)
  VoxelTable table;                    // base-frame voxels of one scan; k_feed_emit leaves it clean
  uint32_t* counters = nullptr;        // [0] n_out, [1] ticket, [2] claimed slots
  FeedResult* res_host = nullptr;      // pinned + mapped
  FeedResult* res_dev = nullptr;
  float* stage = nullptr;              // pinned staging for the raw scan
  size_t cap_points = 0;
  uint32_t seq = 0;
  // stitcher (cbSensor :185-200): the last stitcher_num raw scans, oldest first, packed xyz in `stage`
  int stitcher_num = 0;
  std::deque<uint32_t> stitched;       // point counts of the queued scans
  Owned mem;
};

// one raw record through cbSensor's transform, crop and voxel insert
__device__ __forceinline__ void feed_insert_record(const FeedParams& f, float sx, float sy, float sz, const VoxelView& table) {
  if (!(isfinite(sx) && isfinite(sy) && isfinite(sz))) return;
  const float3 p = affine_to_float(f.Rbs, f.tbs, sx, sy, sz);
  // pcl::PassThrough keeps limit_min <= v <= limit_max
  if (p.x < -f.window || p.x > f.window || p.y < -f.window || p.y > f.window || p.z < 0.0f || p.z > f.height) return;
  // pcl::VoxelGrid with a 0.1f leaf -> inverse 10.0f
  voxel_insert(table, voxel_key(p.x, p.y, p.z, 1.0f / 0.1f), (double)p.x, (double)p.y, (double)p.z, 1u);
}

__global__ __launch_bounds__(256) void k_feed_insert(FeedParams f, const float* __restrict__ scan, int stride_floats,
                                                     VoxelView table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.n) return;
  const float* sp = scan + (size_t)i * stride_floats;
  feed_insert_record(f, sp[0], sp[1], sp[2], table);
}

__global__ __launch_bounds__(256) void k_feed_emit(FeedParams f, VoxelView table, float4* __restrict__ out,
                                                   uint32_t* __restrict__ counters, FeedResult* __restrict__ res,
                                                   uint32_t seq) {
  // one lane per occupied voxel (the slots k_feed_insert listed), not per table slot
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool occ = idx < counters[2];
  const uint32_t o = wave_append(occ, &counters[0]);
  if (occ) {
    const float3 c = voxel_take(table, table.claimed[idx]);
    const float3 g = affine_to_float(f.Rgb, f.tgb, c.x, c.y, c.z);
    out[o] = make_float4(g.x, g.y, g.z, 0.f);
  }
  // last workgroup publishes the count to the host (the count is only touched by device-scope atomics)
  if (last_block(&counters[1])) {
    res->n_out = __hip_atomic_load(&counters[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    counters[0] = 0;         // next call
    counters[1] = 0;
    counters[2] = 0;
    __threadfence_system();
    __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

inline int perception_alloc(PerceptionScratch& s, size_t max_points) {
  s.cap_points = max_points;
  if (s.table.alloc(s.mem.dev, max_points) != 0) return -1;
  if (dev_alloc_zeroed(s.mem.dev, &s.counters, 4) != hipSuccess) return -1;
  if (host_mapped_alloc(s.mem.host, &s.res_host, &s.res_dev, sizeof(FeedResult)) != 0) return -1;
  // the raw scan is read by k_feed_insert straight from this pinned, device-mapped buffer
  // (no separate H2D copy: the kernel's coalesced reads stream it over PCIe)
  if (host_mapped_alloc(s.mem.host, &s.stage, &s.stage_dev, max_points * 4 * sizeof(float)) != 0) return -1;
  s.res_host->n_out = 0;
  s.res_host->seq = 0;
  return 0;
}

inline void perception_free(PerceptionScratch& s) { s = PerceptionScratch(); }

// scan: caller's records (stride_bytes apart, x y z first).  Output: out_dev (global frame).
// With a stitcher depth N > 0 the scan joins the queue of the last N raw scans (the oldest one leaves when
// the queue is full) and the WHOLE queue, oldest first, is fed through the current transforms -- cbSensor's
// pcl_stitcher_ deque (multilayer_spinning_lidar.cpp:185-200).
inline int perception_feed(PerceptionScratch& s, FeedParams f, const float* scan, size_t stride_bytes,
                           float4* out_dev, hipStream_t stream, uint32_t* n_out) {
  *n_out = 0;
  const bool stitch = s.stitcher_num > 0;
  if (stitch) {
    if ((int)s.stitched.size() >= s.stitcher_num) {            // pop_front: the later scans move up
      const size_t drop = s.stitched.front();
      s.stitched.pop_front();
      size_t rest = 0;
      for (uint32_t c : s.stitched) rest += c;
      std::memmove(s.stage, s.stage + 3 * drop, rest * 3 * sizeof(float));
    }
    size_t have = 0;
    for (uint32_t c : s.stitched) have += c;
    if (have + (size_t)f.n > s.cap_points) return -2;
    pack_xyz_records(s.stage + 3 * have, scan, (size_t)f.n, stride_bytes);
    s.stitched.push_back((uint32_t)f.n);
    f.n = (int)(have + (size_t)f.n);
  }
  if (f.n == 0) return 0;
  // a call only uses the first `slots` entries of the full-capacity table
  const size_t slots = voxel_slots_for((size_t)f.n);
  if (slots > s.table.slots) return -2;
  // the raw records go to pinned memory (the stitcher's queue is there already, packed)
  const int stride_floats = stitch ? 3 : stage_xyz_records(s.stage, scan, (size_t)f.n, stride_bytes);
  const VoxelView table = s.table.view(slots, s.counters + 2);
  const uint32_t seq = next_seq(s.seq);
  hipLaunchKernelGGL(k_feed_insert, dim3((f.n + 255) / 256), dim3(256), 0, stream, f, s.stage_dev, stride_floats, table);
  hipLaunchKernelGGL(k_feed_emit, dim3((unsigned)((f.n + 255) / 256)), dim3(256), 0, stream, f, table, out_dev, s.counters,
                     s.res_dev, seq);
  if (const int rc = feed_wait(stream, &s.res_host->seq, seq)) return rc;
  *n_out = s.res_host->n_out;
  return 0;
}

// ---------------------------------------------------------------------------
// PathBlockedStrategy::selfMark
// (dddmr_perception_3d/plugins/path_blocked_strategy.cpp:56-100): which forward points of
// the prune-plan cloud have an observation point within check_radius.  The reference
// builds a second kd-tree on the aggregate observation for M radius searches (:68-83);
// here every cloud point is tested against the forward plan points kept in LDS (a
// bounding box of the plan, grown by the radius, rejects nearly all of them first).
// FLANN's L2_Simple float distance, strict `<` against static_cast<float>(r * r).
// ---------------------------------------------------------------------------
constexpr int kBlockedMaxPlan = 1024;   // pcl_prune_plan_ points (the nearest pose appears twice)
struct BlockedParams {
  int n_points;
  int m;            // plan points
  float r2;
  float lo[3], hi[3];
};

__global__ __launch_bounds__(256) void k_path_blocked(BlockedParams b, const float4* __restrict__ cloud,
                                                      const float4* __restrict__ plan_xyzi,
                                                      uint32_t* __restrict__ flags /* [(m + 31) / 32] */) {
  __shared__ float4 plan[kBlockedMaxPlan];
  __shared__ uint32_t hit[kBlockedMaxPlan / 32];
  for (int i = threadIdx.x; i < b.m; i += blockDim.x) plan[i] = plan_xyzi[i];
  for (int i = threadIdx.x; i < kBlockedMaxPlan / 32; i += blockDim.x) hit[i] = 0u;
  __syncthreads();
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < b.n_points; i += stride) {
    const float4 p = cloud[i];
    if (!(p.x >= b.lo[0] && p.x <= b.hi[0] && p.y >= b.lo[1] && p.y <= b.hi[1] && p.z >= b.lo[2] && p.z <= b.hi[2]))
      continue;
    for (int j = 0; j < b.m; ++j) {
      const float4 q = plan[j];
      if (q.w < 0.f) continue;                    // backward of the robot (:80-81)
      float d = q.x - p.x;
      float r = d * d;
      d = q.y - p.y;
      r = r + d * d;
      d = q.z - p.z;
      r = r + d * d;
      if (r < b.r2) atomicOr(&hit[j >> 5], 1u << (j & 31));
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (b.m + 31) / 32; i += blockDim.x)
    if (hit[i]) atomicOr(&flags[i], hit[i]);
}

}  // namespace dddmr
