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

#include "dev_memory.hip.h"           // Owned, host_mapped_alloc, feed_wait
#include "perception_kernels.hip.h"
#include "point_grid_plan.hip.h"      // stage_xyz_records
#include "wave_ops.hip.h"             // wave_append, last_block

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
  VoxelTable table;                    // base-frame voxels of one frame; k_depth_emit leaves it clean
  uint32_t* counters = nullptr;        // [0] survivors, [1] ticket, [2] claimed slots, [3] emitted
  DepthResult* res_host = nullptr;
  DepthResult* res_dev = nullptr;
  uint32_t seq = 0;
  Owned mem;
};

// One raw record per lane (valid = the lane has one), every lane of the wave calls it: bufferCloud's transform and
// height band, the wave-aggregated append of the survivors and their voxel sums.  The body of k_depth_insert; the depth
// image path (depth_image.hip.h) calls it on its stage-one centroids.
__device__ __forceinline__ void depth_insert_record(const DepthParams& f, bool valid, float sx, float sy, float sz,
                                                    float4* __restrict__ surv, const VoxelView& table,
                                                    uint32_t* __restrict__ counters) {
  bool keep = false;
  float3 p = make_float3(0.f, 0.f, 0.f);
  if (valid && isfinite(sx) && isfinite(sy) && isfinite(sz)) {
    p = affine_to_float(f.Rbs, f.tbs, sx, sy, sz);
    keep = (double)p.z <= f.zmax && (double)p.z >= f.zmin;
  }
  // the survivors keep their pixel order
  const uint32_t o = wave_append(keep, &counters[0]);
  if (!keep) return;
  surv[o] = make_float4(p.x, p.y, p.z, 0.f);
  // the voxel sums, whichever branch the frame ends on (the count is not known before the last workgroup
  // has run; a frame of at most 20000 survivors wastes at most 20000 inserts, hidden behind the PCIe reads);
  // pcl::VoxelGrid with a 0.05f leaf -> inverse 20.0f
  voxel_insert(table, voxel_key(p.x, p.y, p.z, 1.0f / 0.05f), (double)p.x, (double)p.y, (double)p.z, 1u);
}

__global__ __launch_bounds__(256) void k_depth_insert(DepthParams f, const float* __restrict__ raw, int stride_floats,
                                                      float4* __restrict__ surv, VoxelView table,
                                                      uint32_t* __restrict__ counters) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < f.n;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (valid) {
    const float* sp = raw + (size_t)i * stride_floats;
    sx = sp[0], sy = sp[1], sz = sp[2];
  }
  depth_insert_record(f, valid, sx, sy, sz, surv, table, counters);
}

// Grid-stride over max(survivors, claimed slots): the branch is decided here, from the device's own count.
__global__ __launch_bounds__(256) void k_depth_emit(DepthParams f, const float4* __restrict__ surv, VoxelView table,
                                                    float4* __restrict__ out, uint32_t* __restrict__ counters,
                                                    DepthResult* __restrict__ res, uint32_t seq) {
  const uint32_t n_surv = counters[0], n_claimed = counters[2];
  const bool voxelise = n_surv > kDepthVoxelizeAbove;
  const uint32_t work = voxelise ? n_claimed : max(n_surv, n_claimed);
  for (uint32_t idx0 = blockIdx.x * blockDim.x; idx0 < work; idx0 += gridDim.x * blockDim.x) {   // uniform per workgroup
    const uint32_t idx = idx0 + threadIdx.x;
    const bool occ = idx < n_claimed;
    const uint32_t slot = occ ? table.claimed[idx] : 0u;
    if (voxelise) {
      // one lane per occupied voxel
      const uint32_t o = wave_append(occ, &counters[3]);
      if (occ) {
        const float3 c = voxel_take(table, slot);
        const float3 g = affine_to_float(f.Rgb, f.tgb, c.x, c.y, c.z);
        out[o] = make_float4(g.x, g.y, g.z, 0.f);
      }
    } else {
      if (idx < n_surv) {
        // the points pass unchanged: base -> global
        const float4 p = surv[idx];
        const float3 g = affine_to_float(f.Rgb, f.tgb, p.x, p.y, p.z);
        out[idx] = make_float4(g.x, g.y, g.z, 0.f);
      }
      if (occ) voxel_clean(table, slot);     // sums nobody read
    }
  }
  // last workgroup publishes the counts to the host (the counters are only touched by device-scope atomics)
  if (last_block(&counters[1])) {
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

inline void depth_free(DepthSource& s) { s = DepthSource(); }

// max_points bounds what the source may publish; a frame under construction sits behind it.  raw_stage = false: a
// source fed depth images, which stages those itself (depth_image.hip.h)
inline int depth_alloc(DepthSource& s, size_t max_points, bool raw_stage = true) {
  const size_t F = s.max_frame_points;
  for (float4*& b : s.buf)
    if (dev_alloc(s.mem.dev, &b, max_points + F) != hipSuccess) return -1;
  if (dev_alloc(s.mem.dev, &s.surv, F) != hipSuccess) return -1;
  if (s.table.alloc(s.mem.dev, F) != 0) return -1;
  if (dev_alloc_zeroed(s.mem.dev, &s.counters, 4) != hipSuccess) return -1;
  if (host_mapped_alloc(s.mem.host, &s.res_host, &s.res_dev, sizeof(DepthResult)) != 0) return -1;
  // k_depth_insert reads the raw frame straight from this pinned, device-mapped buffer
  if (raw_stage && host_mapped_alloc(s.mem.host, &s.stage, &s.stage_dev, F * 4 * sizeof(float)) != 0) return -1;
  std::memset(s.res_host, 0, sizeof(DepthResult));
  return 0;
}

// One frame through the two kernels into out_dev (room for max_frame_points points); f.n <= max_frame_points.
inline int depth_feed(DepthSource& s, DepthParams f, const float* raw, size_t stride_bytes, float4* out_dev,
                      hipStream_t stream, uint32_t* n_out) {
  *n_out = 0;
  if (f.n == 0) return 0;
  const int stride_floats = stage_xyz_records(s.stage, raw, (size_t)f.n, stride_bytes);
  const uint32_t seq = next_seq(s.seq);
  // table of this frame: the first `slots` entries, load <= 0.5 even if every record survives in a voxel of its own
  const size_t slots = voxel_slots_for((size_t)f.n);
  if (slots > s.table.slots) return -2;
  const VoxelView table = s.table.view(slots, s.counters + 2);
  const dim3 grid((unsigned)((f.n + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_depth_insert, grid, block, 0, stream, f, s.stage_dev, stride_floats, s.surv, table, s.counters);
  // survivors and voxels are a fraction of the raw records: a fixed grid walks them
  const dim3 emit_grid(std::min<unsigned>(grid.x, kDepthEmitBlocks));
  hipLaunchKernelGGL(k_depth_emit, emit_grid, block, 0, stream, f, s.surv, table, out_dev, s.counters, s.res_dev, seq);
  // the device chose the branch from its own count; the host waits once, for the last kernel's word
  if (const int rc = feed_wait(stream, &s.res_host->seq, seq)) return rc;
  *n_out = s.res_host->n_out;
  return 0;
}

}  // namespace dddmr
