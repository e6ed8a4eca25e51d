// depth_image.hip.h -- the depth image as the camera delivers it, through to the local planner's aggregate.
//
// Stage one replaces the reference's own node in front of the depth camera layer,
// DepthImg2PointCloud::cbDepthImg (dddmr_perception_3d/utils/depthimg2pointcloud_node.cpp:96-157): every
// sample_step-th pixel of every sample_step-th row of a 16UC1 image, z = d * 0.001, dropped when z > max_distance,
// pinhole deprojection, pcl::VoxelGrid with leaf_size in the optical frame.  Stage two is bufferCloud as
// depth_feed.hip.h restates it, applied to stage one's centroids.  Only the sampled rows of the uint16 image cross
// PCIe (2 bytes per pixel against the 12-16 of a point record).
//
// Three launches on one stream, one host wait (on k_depth_emit's word, as for a cloud frame):
//   k_dimg_insert    one lane per sampled pixel: deprojection with the node's casts, camera-frame voxel key, sums into
//                    the source's second hash table.  Neighbouring pixels of a row mostly share a voxel (a 0.05 m voxel
//                    2 m away is 8 pixels wide at 640 columns, and a region without a return is one voxel altogether:
//                    the node keeps depth 0 as the point (0, 0, 0)), so every lane updating the table for itself
//                    would put tens of adders on one slot.  The runs of equal keys among the consecutive lanes of a
//                    wave are summed first (segmented scan over shuffles, double) and the last lane of a run makes the
//                    one update; a run of depth-0 pixels adds its count only, its sums are exactly 0.
//                    With DIMG_PX == 4 (sample_step 1, width a multiple of 4) a lane loads 4 pixels as one 8-byte
//                    word and the wave then walks its 256 consecutive pixels 64 at a time, so runs stay contiguous.
//   k_dimg_centroid  one lane per claimed camera-frame voxel: float centroid, stored as the source's stage-one cloud
//                    (what the node publishes), slot cleaned; and in the same pass stage two's insert on that centroid
//                    (depth_insert_record of depth_feed.hip.h: transform, height band, compaction, base-frame table).
//                    The number of centroids is only known on the device, hence a fixed grid that strides over it.
//   k_depth_emit     unchanged.
// Stage two as a fourth kernel that reads the stage-one cloud back was measured beside the fused pass and lost
// (profiles/r05_depth_image.json); it is in the history.
//
// Voxel membership is floor(p * (1.0f / (float)leaf)) per axis in float; centroid sums are double where PCL sums in
// float in input order, so stage-one centroids agree with PCL's to the spread of PCL's own summation orders.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "depth_feed.hip.h"
#include "dev_memory.hip.h"   // Owned, dev_alloc, feed_wait
#include "wave_ops.hip.h"     // last_block

// Nothing may be fused: the reference is an x86-64 build without FMA contraction.
#pragma clang fp contract(off)

#ifndef DDDMR_DIMG_PX
#define DDDMR_DIMG_PX 4      // pixels per lane and load at sample_step 1 (1 or 4)
#endif

namespace dddmr {

struct DimgParams {
  float cx, cy, fx, fy;        // cx, cy as floats; fx, fy = (float)(1.0 / K[0]), (float)(1.0 / K[4])
  float inv_leaf;              // 1.0f / (float)leaf_size
  uint32_t drop_zero;
  double max_distance;
  uint32_t width;              // pixels per staged row
  uint32_t cols, rows, step;   // sampled columns / rows
};

struct DimgResult {            // host-mapped, written by the last k_dimg_centroid workgroup
  uint32_t n_camera;           // stage-one points
  uint32_t pad[3];
};

struct DepthImage {
  DimgParams p;
  uint32_t height = 0;
  uint16_t* stage = nullptr;          // pinned + mapped: the sampled rows, packed
  uint16_t* stage_dev = nullptr;
  VoxelTable table;                   // camera-frame voxels; k_dimg_centroid leaves it clean
  uint32_t* counters = nullptr;       // [0] claimed slots, [1] ticket
  float* cloud[2] = {nullptr, nullptr};   // stage-one cloud, packed xyz; cloud[cur] belongs to the latest accepted image
  int cur = 0;
  uint32_t n_cloud = 0;
  DimgResult* res_host = nullptr;
  DimgResult* res_dev = nullptr;
  Owned mem;
};

__device__ __forceinline__ double dimg_shfl_up(double v, int delta) {
  return __shfl_up(v, (unsigned)delta, 64);
}

// 64 consecutive sampled pixels, one per lane (valid = the lane has one): deproject, sum the runs, update the table.
// Every lane of the wave calls it.
__device__ __forceinline__ void dimg_wave_pixels(const DimgParams& p, bool valid, uint32_t u, uint32_t v, uint32_t d,
                                                 const VoxelView& table) {
  const int lane = threadIdx.x & 63;
  // cbDepthImg:132-146.  `float z = at<unsigned short>(v, u) * 0.001`: double product, float result;
  // `z > max_distance_` compares in double; x and y in float, left to right
  const float z = (float)((double)d * 0.001);
  const bool keep = valid && !((double)z > p.max_distance) && !(p.drop_zero && d == 0u);
  const float x = ((float)u - p.cx) * z * p.fx;
  const float y = ((float)v - p.cy) * z * p.fy;
  const unsigned long long key = keep ? voxel_key(x, y, z, p.inv_leaf) : 0ull;   // 0 is no key: bit 63 marks one
  // runs of equal keys among consecutive lanes
  const unsigned long long prev_key = __shfl_up(key, 1u, 64);
  const bool head = lane == 0 || prev_key != key;
  const unsigned long long heads = __ballot(head);
  const int run_head = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));    // lane 63: 2 << 63 wraps to 0, - 1 = all ones
  double sx = (double)x, sy = (double)y, sz = (double)z;
  uint32_t cnt = 1u;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double ax = dimg_shfl_up(sx, off), ay = dimg_shfl_up(sy, off), az = dimg_shfl_up(sz, off);
    const uint32_t ac = __shfl_up(cnt, (unsigned)off, 64);
    if (lane - off >= run_head) { sx += ax; sy += ay; sz += az; cnt += ac; }
  }
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (!(tail && keep)) return;
  // A region without a return costs one counter add per run: all-zero sums are not added.  A run may mix depth 0
  // with a tiny depth of the same voxel, so that test is on the sums, not on this lane's pixel.
  voxel_insert(table, key, sx, sy, sz, cnt);
}

// PX == 1: lane i = sampled pixel i (row i / cols, column i % cols), any step.
// PX == 4: step 1, width % 4 == 0: lane i loads pixels 4 i .. 4 i + 3 as one 8-byte word; the wave's 256 consecutive
// pixels are then processed in 4 rounds of 64 consecutive ones (round j, lane L: pixel 64 j + L, held by lane
// 16 j + L / 4), so the runs of equal keys are found among neighbours exactly as for PX == 1.
template <int PX>
__global__ __launch_bounds__(256) void k_dimg_insert(DimgParams p, const uint16_t* __restrict__ img, VoxelView table) {
  const uint32_t n = p.rows * p.cols;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (PX == 1) {
    const bool valid = i < n;
    const uint32_t r = valid ? i / p.cols : 0u, c = valid ? i - r * p.cols : 0u;
    const uint32_t u = c * p.step, v = r * p.step;
    const uint32_t d = valid ? (uint32_t)img[(size_t)r * p.width + u] : 0u;
    dimg_wave_pixels(p, valid, u, v, d, table);
  } else {
    static_assert(PX == 4, "1 or 4 pixels per lane");
    const int lane = threadIdx.x & 63;
    const uint32_t wave_first = (i - (uint32_t)lane) * 4u;      // first pixel of this wave; n % 4 == 0
    uint2 w = make_uint2(0u, 0u);
    if (4u * i < n) w = *reinterpret_cast<const uint2*>(img + 4 * (size_t)i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int src = 16 * j + (lane >> 2);
      const uint32_t lo = __shfl(w.x, src, 64), hi = __shfl(w.y, src, 64);
      const uint32_t pair = (lane & 2) ? hi : lo;
      const uint32_t d = (lane & 1) ? (pair >> 16) : (pair & 0xFFFFu);
      const uint32_t px = wave_first + 64u * (uint32_t)j + (uint32_t)lane;
      const bool valid = px < n;
      const uint32_t v = px / p.width, u = px - v * p.width;    // step 1: cols == width
      dimg_wave_pixels(p, valid, u, v, valid ? d : 0u, table);
    }
  }
}

// One lane per claimed camera-frame voxel, fixed grid striding over the device's own count, stage two's insert in the
// same pass.  The last workgroup hands the count on and zeroes the counters for the next image.
__global__ __launch_bounds__(256) void k_dimg_centroid(DepthParams f, VoxelView cam, uint32_t* __restrict__ icounters,
                                                       float* __restrict__ cloud, DimgResult* __restrict__ ires,
                                                       float4* __restrict__ surv, VoxelView table,
                                                       uint32_t* __restrict__ counters) {
  const uint32_t n_claimed = icounters[0];
  for (uint32_t idx0 = blockIdx.x * blockDim.x; idx0 < n_claimed; idx0 += gridDim.x * blockDim.x) {   // uniform per workgroup
    const uint32_t idx = idx0 + threadIdx.x;
    const bool occ = idx < n_claimed;
    float3 c = make_float3(0.f, 0.f, 0.f);
    if (occ) {
      c = voxel_take(cam, cam.claimed[idx]);
      cloud[3 * (size_t)idx + 0] = c.x;
      cloud[3 * (size_t)idx + 1] = c.y;
      cloud[3 * (size_t)idx + 2] = c.z;
    }
    depth_insert_record(f, occ, c.x, c.y, c.z, surv, table, counters);
  }
  if (last_block(&icounters[1])) {                     // every workgroup has read icounters[0]
    ires->n_camera = n_claimed;                        // the host reads it after k_depth_emit's release of its own word
    icounters[0] = 0;
    icounters[1] = 0;
    __threadfence_system();
  }
}

inline void dimg_free(DepthImage& d) { d = DepthImage(); }

// d.p and d.height are set; the tables hold every sampled pixel in a voxel of its own at load <= 0.5
inline int dimg_alloc(DepthImage& d) {
  const size_t n = (size_t)d.p.rows * d.p.cols;
  if (host_mapped_alloc(d.mem.host, &d.stage, &d.stage_dev, (size_t)d.p.rows * d.p.width * sizeof(uint16_t) + 8) != 0) return -1;
  if (d.table.alloc(d.mem.dev, n) != 0) return -1;
  if (dev_alloc_zeroed(d.mem.dev, &d.counters, 4) != hipSuccess) return -1;
  for (float*& c : d.cloud)
    if (dev_alloc(d.mem.dev, &c, n * 3) != hipSuccess) return -1;
  if (host_mapped_alloc(d.mem.host, &d.res_host, &d.res_dev, sizeof(DimgResult)) != 0) return -1;
  std::memset(d.res_host, 0, sizeof(DimgResult));
  return 0;
}

// Worst-case voxel box of the frustum: every sampled pixel anywhere between depth 0 and min(max_distance, 65.535 m).
// false when it could reach 2^31 cells (where pcl::VoxelGrid gives up and returns its input) or an index leaves the
// 21 bits per axis of the key.
inline bool dimg_box_ok(const DimgParams& p, uint32_t height) {
  const double zmax = std::min(p.max_distance, 65.535);
  const double inv = (double)p.inv_leaf;
  const double xs[2] = {(0.0 - (double)p.cx) * zmax * (double)p.fx, ((double)(p.width - 1) - (double)p.cx) * zmax * (double)p.fx};
  const double ys[2] = {(0.0 - (double)p.cy) * zmax * (double)p.fy, ((double)(height - 1) - (double)p.cy) * zmax * (double)p.fy};
  double cells = 1.0;
  const double lo[3] = {std::min(0.0, std::min(xs[0], xs[1])), std::min(0.0, std::min(ys[0], ys[1])), 0.0};
  const double hi[3] = {std::max(0.0, std::max(xs[0], xs[1])), std::max(0.0, std::max(ys[0], ys[1])), zmax};
  for (int a = 0; a < 3; ++a) {
    const double i0 = std::floor(lo[a] * inv) - 1.0, i1 = std::floor(hi[a] * inv) + 1.0;   // one cell of slack for the float rounding
    if (!(i0 > -(double)(1 << 20)) || !(i1 < (double)(1 << 20))) return false;
    cells *= i1 - i0 + 1.0;
  }
  return cells < 2147483648.0;
}

// One image through stage one and two into out_dev (room for max_frame_points points).  img: height rows of
// row_stride_bytes.  The stage-one cloud goes to d.cloud[d.cur ^ 1]; the caller swaps on success.
inline int depth_image_feed(DepthSource& s, DepthImage& d, DepthParams f, const uint16_t* img, size_t row_stride_bytes,
                            float4* out_dev, hipStream_t stream, uint32_t* n_camera, uint32_t* n_out) {
  *n_out = 0;
  *n_camera = 0;
  const DimgParams& p = d.p;
  const size_t row_bytes = (size_t)p.width * sizeof(uint16_t);
  if (p.step == 1 && row_stride_bytes == row_bytes) {
    std::memcpy(d.stage, img, row_bytes * p.rows);
  } else {
    for (uint32_t r = 0; r < p.rows; ++r)               // only the sampled rows cross to the device
      std::memcpy(d.stage + (size_t)r * p.width, reinterpret_cast<const unsigned char*>(img) + (size_t)r * p.step * row_stride_bytes,
                  row_bytes);
  }
  // both tables in full: neither stage knows its voxel count before its kernel has run
  const VoxelView cam = d.table.view(d.table.slots, d.counters + 0);
  const VoxelView table = s.table.view(s.table.slots, s.counters + 2);
  const uint32_t seq = next_seq(s.seq);
  const uint32_t n = p.rows * p.cols;
  const dim3 block(256);
  if (DDDMR_DIMG_PX == 4 && p.step == 1 && p.width % 4 == 0)
    hipLaunchKernelGGL(k_dimg_insert<4>, dim3((n / 4 + 255) / 256), block, 0, stream, p, d.stage_dev, cam);
  else
    hipLaunchKernelGGL(k_dimg_insert<1>, dim3((n + 255) / 256), block, 0, stream, p, d.stage_dev, cam);
  const dim3 walk(std::min<unsigned>((n + 255) / 256, kDepthEmitBlocks));
  hipLaunchKernelGGL(k_dimg_centroid, walk, block, 0, stream, f, cam, d.counters, d.cloud[d.cur ^ 1], d.res_dev, s.surv, table,
                     s.counters);
  hipLaunchKernelGGL(k_depth_emit, walk, block, 0, stream, f, s.surv, table, out_dev, s.counters, s.res_dev, seq);
  if (const int rc = feed_wait(stream, &s.res_host->seq, seq)) return rc;
  *n_out = s.res_host->n_out;
  *n_camera = *reinterpret_cast<volatile uint32_t*>(&d.res_host->n_camera);
  return 0;
}

}  // namespace dddmr
