// lidar_sweep.hip.h -- the raw lidar sweep, through to the cloud the lidar perception plugins subscribe to.
//
// Stage one replaces the front half of the reference's own node in front of the lidar plugins,
// ImageProjection::cloudHandler (dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp:280-314): pitch removal
// (:297-303), projectPointCloud (:328-382), groundRemoval's marks (:415-473, :519-526), cloudSegmentation /
// labelComponents (:538-540, :595-679) and the segmented_cloud_pure output (:582-592).  Stage two is cbSensor as
// perception_kernels.hip.h restates it, applied to stage one's points without the cloud leaving the device.
//
// The casts follow the member types of imageProjection.h:67-107: the angular resolutions, _ang_bottom, _segment_theta
// and the detection ranges are floats computed in double; tan(theta), sin(alpha) and cos(alpha) are constants of the
// configuration, computed once on the host with the float overloads.  Nothing is fused.
//
// labelComponents is a serial BFS over a symmetric relation (d1 / d2 are the max / min of the two ranges) that never
// revisits a labelled pixel, so each BFS fills exactly one connected component of the non-ground, non-empty pixels and
// its seed is the component's first pixel in raster order.  Here: a lock-free union-find over the 2 V H neighbour
// pairs with the smaller raster index as the root (marking.hip.h's cc_find pattern, with path halving), so the root IS
// the seed.  lineCountFlag is set for pushed neighbours only, never for the seed: a root's row mask takes every member's row
// except the root's own contribution.  Valid components are numbered in the raster order of their roots by a prefix
// scan, and a second scan over the output pixels gives segmented_cloud_pure's raster order.
//
// One route for every image size, eight launches on one stream and no host wait between them:
//   k_sweep_project   one lane per raw point: pitch removal, range, pixel; atomicMax of (input index + 1) per pixel
//                     (the last point in input order wins a pixel, :364-381); the moved point is kept on the device
//   k_sweep_gather    one lane per pixel: the winner's point and range (NaN / FLT_MAX where empty); the index table
//                     is left zero for the next sweep
//   k_sweep_ground    one lane per pixel pair (i, j), (i + 1, j), i < ground_scan_index
//   k_sweep_union     one lane per neighbour pair (columns wrap, rows do not)
//   k_sweep_count     one lane per pixel: its root; the root's size and row mask (one update per wave, root and row)
//   k_sweep_blocks    one lane per pixel: per-workgroup counts of valid roots and of output pixels
//   k_sweep_number    one lane per pixel: label numbers of the roots; size and row mask left zero
//   k_sweep_output    one lane per pixel: the label image and the ordered output cloud
// A route that keeps a small image in one workgroup's LDS was not built; DESIGN 4a says why.
// When the source's features are on (lidar_features.hip.h), their launches follow k_sweep_output on the same stream.
//
// Differences from the reference, on purpose: a record with any non-finite coordinate is dropped
// (removeNaNFromPointCloud trusts is_dense); a point whose row quotient is not a number (range 0) is dropped (the
// reference converts NaN to int); an empty sweep yields an empty cloud (the reference reads points.front()).
// Left out: the patched ground cloud and its VoxelGrid (:450-514), the projected image.  (segmented_cloud and _seg_msg's
// arrays: lidar_features.hip.h; findStartEndAngle and outlier_cloud: sweep_association.hip.h; each when switched on.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

#include "dev_memory.hip.h"           // Owned, dev_alloc, feed_wait
#include "perception_kernels.hip.h"
#include "point_grid_plan.hip.h"      // stage_xyz_records
#include "wave_ops.hip.h"             // block_rank, wave_sum

// Nothing may be fused: the reference is an x86-64 build without FMA contraction.
#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kSweepNone = 0xFFFFFFFFu;     // parent of a ground or empty pixel
constexpr int32_t kSweepInvalidLabel = 999999;   // labelComponents :676
constexpr uint32_t kSweepMaxRows = 128, kSweepMaxCols = 4096, kSweepMaxPixels = 1u << 19, kSweepMaxPoints = 1u << 20;

struct SweepParams {
  double Rp[9], tp[3];         // q.setRPY(0, mount, 0) as an Affine3d (:297-302); tp = 0
  double mount;                // _sensor_mount_angle (double member)
  double ground_limit;         // 10 * DEG_TO_RAD
  uint32_t V, H, n, gsi;
  int stride_floats;
  float ang_bottom, res_x, res_y;
  float min_range, max_range;
  float sin_x, cos_x, sin_y, cos_y, tan_theta;
  uint32_t valid_points, valid_lines;
};

struct SweepResult {           // host-mapped, written by the last k_sweep_output workgroup
  uint32_t n_segmented;
  uint32_t pad[3];
};

struct LidarFeatures;           // lidar_features.hip.h
inline void features_launch(LidarFeatures& f, int b, const int32_t* label_img, const uint8_t* ground_img, const float* range_img,
                            const float4* pts, hipStream_t stream);
struct SweepParams;
inline void association_launch(LidarFeatures& f, int b, const SweepParams& sweep, const float* raw, const float4* moved,
                               const int32_t* label_img, const float4* pts, hipStream_t stream);   // sweep_association.hip.h

struct LidarSweep {
  SweepParams p;
  std::unique_ptr<LidarFeatures, LateDelete<LidarFeatures>> features;   // not null: the source's features are on
  uint32_t max_points = 0;             // raw points per sweep
  PerceptionScratch feed;              // stage two's table; its pinned staging holds the raw sweep
  float4* moved = nullptr;             // [max_points] pitch-removed point, range in w
  uint32_t* pix_idx = nullptr;         // [V H] winner's input index + 1; zero between sweeps
  float4* pts = nullptr;               // [V H] _full_cloud: NaN where empty
  uint32_t* parent = nullptr;          // [V H]
  uint32_t* size = nullptr;            // [V H] members of a root; zero between sweeps
  uint32_t* rows = nullptr;            // [V H x 4] lineCountFlag of a root; zero between sweeps
  uint32_t* num = nullptr;             // [V H] label number of a root, 0 = invalid
  uint2* block_cnt = nullptr;          // [workgroups] valid roots, output pixels
  uint32_t* n_dev = nullptr;           // [1] the output cloud's size, for stage two
  // what the getters return belongs to the latest ACCEPTED sweep: [cur]; a sweep is built in [cur ^ 1]
  float* range_img[2] = {nullptr, nullptr};
  int32_t* label_img[2] = {nullptr, nullptr};
  uint8_t* ground_img[2] = {nullptr, nullptr};
  float4* cloud[2] = {nullptr, nullptr};   // x y z label
  float4* obs[2] = {nullptr, nullptr};     // stage two's observation; the source's obs in the context aliases obs[cur]
  int cur = 0;
  uint32_t n_cloud = 0;
  bool have_sweep = false;
  SweepResult* res_host = nullptr;
  SweepResult* res_dev = nullptr;
  Owned mem;                           // (the nested scratch owns its own)
};

// :331-362 for one pitch-removed point: its pixel, or -1 when one of the three tests drops it
__device__ __forceinline__ int sweep_pixel(const SweepParams& k, float x, float y, float z, float range) {
  const float vertical = asinf(z / range);
  const float rq = (vertical + k.ang_bottom) / k.res_y;
  // int rowIdn = rq truncates toward zero: (-1, 0) lands in row 0; a NaN quotient fails both comparisons
  if (!(rq > -1.0f && rq < (float)k.V)) return -1;
  const int row = (int)rq;
  const float horizon = atan2f(x, y);
  const double cd = -(double)roundf(horizon / k.res_x) + (double)k.H * 0.5;
  int col = (int)cd;
  if (col >= (int)k.H) col -= (int)k.H;
  if (col < 0 || col >= (int)k.H) return -1;
  if (range < k.min_range || range > k.max_range) return -1;
  return row * (int)k.H + col;
}

__global__ __launch_bounds__(256) void k_sweep_project(SweepParams k, const float* __restrict__ raw, float4* __restrict__ moved,
                                                       uint32_t* __restrict__ pix_idx) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k.n) return;
  const float* sp = raw + (size_t)i * k.stride_floats;
  const float sx = sp[0], sy = sp[1], sz = sp[2];
  if (!(isfinite(sx) && isfinite(sy) && isfinite(sz))) return;
  const float3 p = affine_to_float(k.Rp, k.tp, sx, sy, sz);
  const float range = sqrtf(p.x * p.x + p.y * p.y + p.z * p.z);
  moved[i] = make_float4(p.x, p.y, p.z, range);
  const int pix = sweep_pixel(k, p.x, p.y, p.z, range);
  if (pix >= 0) atomicMax(&pix_idx[pix], i + 1u);
}

__global__ __launch_bounds__(256) void k_sweep_gather(SweepParams k, const float4* __restrict__ moved, uint32_t* __restrict__ pix_idx,
                                                      float4* __restrict__ pts, float* __restrict__ range_img,
                                                      uint8_t* __restrict__ ground_img, uint32_t* __restrict__ parent) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= k.V * k.H) return;
  const uint32_t idx = pix_idx[p];
  const float nan = __int_as_float(0x7FC00000);
  float4 m = make_float4(nan, nan, nan, FLT_MAX);
  if (idx) {
    m = moved[idx - 1u];
    pix_idx[p] = 0u;
  }
  pts[p] = make_float4(m.x, m.y, m.z, 0.f);
  range_img[p] = m.w;
  ground_img[p] = 0;
  parent[p] = idx ? p : kSweepNone;
}

// :420-443.  The intensity == -1 test never fires (PointXYZI starts at 0); an empty pixel's NaN makes the angle NaN.
__global__ __launch_bounds__(256) void k_sweep_ground(SweepParams k, const float4* __restrict__ pts, uint8_t* __restrict__ ground_img,
                                                      uint32_t* __restrict__ parent) {
  const uint32_t lower = blockIdx.x * 256 + threadIdx.x;
  if (lower >= k.gsi * k.H) return;
  const uint32_t upper = lower + k.H;
  const float4 a = pts[lower], b = pts[upper];
  const float dX = b.x - a.x, dY = b.y - a.y, dZ = b.z - a.z;
  const float angle = atan2f(dZ, sqrtf(dX * dX + dY * dY + dZ * dZ));
  if ((double)angle + k.mount <= k.ground_limit) {
    ground_img[lower] = 1;
    ground_img[upper] = 1;
    parent[lower] = kSweepNone;          // :521-524: label -1, never part of a segment
    parent[upper] = kSweepNone;
  }
}

// cc_find of marking.hip.h with path halving: a horizontal run of a wall is a chain as long as the run without it.  A
// node that has a parent never becomes a root again and a parent is always an ancestor with a smaller index, so storing
// the grandparent over the parent keeps every concurrent find and CAS right.
__device__ __forceinline__ uint32_t sweep_find(uint32_t* parent, uint32_t i) {
  uint32_t p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != i) {
    const uint32_t gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gp != p) __hip_atomic_store(&parent[i], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = p;
    p = gp;
  }
  return i;
}

// The find of the kernels after the unions: it stores nothing.  k_sweep_count leaves parent[p] = root for the kernels
// behind it, and a halving store of another lane's find, made from values read earlier, could land after that store and
// put an ancestor that is not the root back.
__device__ __forceinline__ uint32_t sweep_find_settled(const uint32_t* parent, uint32_t i) {
  uint32_t p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != i) {
    i = p;
    p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return i;
}

// hooks the larger root under the smaller one (marking_fused.hip.h's cc_union_pair)
__device__ __forceinline__ void sweep_union(uint32_t* parent, uint32_t i, uint32_t j) {
  uint32_t u = sweep_find(parent, i), v = sweep_find(parent, j);
  while (u != v) {
    if (u < v) { const uint32_t t = u; u = v; v = t; }
    const uint32_t old = atomicCAS(&parent[u], u, v);
    if (old == u) break;
    u = sweep_find(parent, old);
    v = sweep_find(parent, v);
  }
}

// :620-656 as a relation: lanes [0, V H) the pair (r, c), (r, c + 1 mod H); lanes [V H, 2 V H) the pair (r, c), (r + 1, c)
__global__ __launch_bounds__(256) void k_sweep_union(SweepParams k, const float* __restrict__ range_img, uint32_t* parent) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x, n = k.V * k.H;
  if (e >= 2u * n) return;
  const bool vertical = e >= n;
  const uint32_t p = vertical ? e - n : e;
  uint32_t q;
  if (vertical) {
    if (p + k.H >= n) return;
    q = p + k.H;
  } else {
    const uint32_t c = p % k.H;
    q = c + 1u == k.H ? p - c : p + 1u;
  }
  // a pixel is in or out of the segmentation for the whole launch: kSweepNone is neither written nor removed here
  if (__hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kSweepNone ||
      __hip_atomic_load(&parent[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kSweepNone)
    return;
  const float rp = range_img[p], rq = range_img[q];
  const float d1 = rp < rq ? rq : rp, d2 = rq < rp ? rq : rp;     // std::max / std::min
  const float sa = vertical ? k.sin_y : k.sin_x, ca = vertical ? k.cos_y : k.cos_x;
  const float tang = d2 * sa / (d1 - d2 * ca);
  if (tang > k.tan_theta) sweep_union(parent, p, q);
}

// A wall is thousands of pixels of one root, and the 64 consecutive pixels of a wave mostly share root and row: the lanes
// of a wave that agree on both make one update between them (every lane of the wave stays in the loop).
__global__ __launch_bounds__(256) void k_sweep_count(SweepParams k, uint32_t* parent, uint32_t* __restrict__ size,
                                                     uint32_t* __restrict__ rows) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = p < k.V * k.H && __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kSweepNone;
  uint32_t root = kSweepNone;
  if (live) {
    root = sweep_find_settled(parent, p);                    // no unions any more: the root is final, and only this
    __hip_atomic_store(&parent[p], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // lane stores to parent[p]
  }
  const uint32_t row = p / k.H;
  unsigned long long todo = __ballot(live);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t r = __shfl(root, leader, 64), rw = __shfl(row, leader, 64);
    const bool mine = live && root == r && row == rw;
    const unsigned long long group = __ballot(mine);
    const unsigned long long pushed = __ballot(mine && p != root);   // lineCountFlag: pushed neighbours only (:652)
    if (lane == leader) {
      atomicAdd(&size[r], (uint32_t)__popcll(group));
      if (pushed) atomicOr(&rows[4u * (size_t)r + (rw >> 5)], 1u << (rw & 31u));
    }
    todo &= ~group;
  }
}

// :660-670
__device__ __forceinline__ bool sweep_valid(const SweepParams& k, uint32_t size, const uint32_t* rows) {
  if (size >= 30u) return true;
  if (size < k.valid_points) return false;
  const uint32_t lines = __popc(rows[0]) + __popc(rows[1]) + __popc(rows[2]) + __popc(rows[3]);
  return lines >= k.valid_lines;
}

__global__ __launch_bounds__(256) void k_sweep_blocks(SweepParams k, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                      const uint32_t* __restrict__ rows, uint2* __restrict__ block_cnt) {
  __shared__ uint32_t lds[4];
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const uint32_t root = p < k.V * k.H ? parent[p] : kSweepNone;
  const bool valid = root != kSweepNone && sweep_valid(k, size[root], rows + 4u * (size_t)root);
  uint32_t n_roots, n_out;
  block_rank<4>(valid && root == p, lds, &n_roots);
  block_rank<4>(valid, lds, &n_out);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = make_uint2(n_roots, n_out);
}

// what the workgroups before this one counted
__device__ __forceinline__ uint2 sweep_blocks_before(const uint2* __restrict__ block_cnt, uint2* lds /* [4] */) {
  uint32_t a = 0, b = 0;
  for (uint32_t i = threadIdx.x; i < blockIdx.x; i += 256) {
    const uint2 c = block_cnt[i];
    a += c.x;
    b += c.y;
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = make_uint2(a, b);
  __syncthreads();
  const uint2 r = make_uint2(lds[0].x + lds[1].x + lds[2].x + lds[3].x, lds[0].y + lds[1].y + lds[2].y + lds[3].y);
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_sweep_number(SweepParams k, const uint32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                      uint32_t* __restrict__ rows, const uint2* __restrict__ block_cnt,
                                                      uint32_t* __restrict__ num) {
  __shared__ uint32_t lds[4];
  __shared__ uint2 lds2[4];
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const bool is_root = p < k.V * k.H && parent[p] == p;
  bool valid = false;
  if (is_root) {                               // only a root reads its own counts here, so it may clear them
    uint32_t* r = rows + 4u * (size_t)p;
    valid = sweep_valid(k, size[p], r);
    size[p] = 0u;
    r[0] = 0u; r[1] = 0u; r[2] = 0u; r[3] = 0u;
  }
  const uint2 before = sweep_blocks_before(block_cnt, lds2);
  uint32_t total;
  const uint32_t rank = block_rank<4>(valid, lds, &total);
  if (is_root) num[p] = valid ? before.x + rank + 1u : 0u;      // _label_count starts at 1
}

__global__ __launch_bounds__(256) void k_sweep_output(SweepParams k, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ num,
                                                      const float4* __restrict__ pts, const uint2* __restrict__ block_cnt,
                                                      int32_t* __restrict__ label_img, float4* __restrict__ cloud,
                                                      uint32_t* __restrict__ n_dev, SweepResult* __restrict__ res) {
  __shared__ uint32_t lds[4];
  __shared__ uint2 lds2[4];
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const bool in = p < k.V * k.H;
  const uint32_t root = in ? parent[p] : kSweepNone;
  int32_t label = -1;
  if (root != kSweepNone) {
    const uint32_t n = num[root];
    label = n ? (int32_t)n : kSweepInvalidLabel;
  }
  if (in) label_img[p] = label;
  const bool out = label > 0 && label != kSweepInvalidLabel;      // :585
  const uint2 before = sweep_blocks_before(block_cnt, lds2);
  uint32_t total;
  const uint32_t rank = block_rank<4>(out, lds, &total);
  if (out) {
    const float4 q = pts[p];
    cloud[before.y + rank] = make_float4(q.x, q.y, q.z, (float)label);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {           // the last workgroup in raster order knows the size
    *n_dev = before.y + total;                                     // for stage two's launch, which follows on the stream
    res->n_segmented = before.y + total;                           // the host reads it after k_feed_emit's release
    __threadfence_system();
  }
}

// Stage two's insert on a device cloud whose size only the device knows: lanes over an upper bound
__global__ __launch_bounds__(256) void k_feed_insert_device(FeedParams f, const float4* __restrict__ cloud,
                                                            const uint32_t* __restrict__ n_dev, VoxelView table) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= *n_dev) return;
  const float4 s = cloud[i];
  feed_insert_record(f, s.x, s.y, s.z, table);
}

inline void sweep_free(LidarSweep& s) { s = LidarSweep(); }   // (with its features, if they are on)

// s.p (V, H) and s.max_points are set
inline int sweep_alloc(LidarSweep& s) {
  const size_t px = (size_t)s.p.V * s.p.H, blocks = (px + 255) / 256;
  if (perception_alloc(s.feed, std::max<size_t>(px, s.max_points)) != 0) return -1;
  auto dev = [&s](auto** ptr, size_t count, bool zero = false) {
    return (zero ? dev_alloc_zeroed(s.mem.dev, ptr, count) : dev_alloc(s.mem.dev, ptr, count)) == hipSuccess;
  };
  bool ok = dev(&s.moved, std::max<size_t>(s.max_points, 1)) && dev(&s.pix_idx, px, true) && dev(&s.pts, px) && dev(&s.parent, px) &&
            dev(&s.size, px, true) && dev(&s.rows, 4 * px, true) && dev(&s.num, px) && dev(&s.block_cnt, blocks) && dev(&s.n_dev, 1, true);
  for (int b = 0; b < 2 && ok; ++b)
    ok = dev(&s.range_img[b], px) && dev(&s.label_img[b], px) && dev(&s.ground_img[b], px) && dev(&s.cloud[b], px) && dev(&s.obs[b], px);
  if (!ok) return -1;
  if (host_mapped_alloc(s.mem.host, &s.res_host, &s.res_dev, sizeof(SweepResult)) != 0) return -1;
  std::memset(s.res_host, 0, sizeof(SweepResult));
  return 0;
}

// One sweep through stage one and two.  Everything it produces goes to the [cur ^ 1] buffers; the caller swaps on
// success.  raw: n records of stride_bytes, x y z first.  *n_out: stage two's points, in s.obs[cur ^ 1].
inline int sweep_feed(LidarSweep& s, FeedParams f, const float* raw, size_t n, size_t stride_bytes, hipStream_t stream,
                      uint32_t* n_segmented, uint32_t* n_out) {
  *n_segmented = 0;
  *n_out = 0;
  SweepParams k = s.p;
  k.n = (uint32_t)n;
  k.stride_floats = n ? stage_xyz_records(s.feed.stage, raw, n, stride_bytes) : 3;
  const int b = s.cur ^ 1;
  const uint32_t px = k.V * k.H;
  const dim3 block(256), per_pixel((px + 255) / 256);
  if (n) hipLaunchKernelGGL(k_sweep_project, dim3((k.n + 255) / 256), block, 0, stream, k, s.feed.stage_dev, s.moved, s.pix_idx);
  hipLaunchKernelGGL(k_sweep_gather, per_pixel, block, 0, stream, k, s.moved, s.pix_idx, s.pts, s.range_img[b], s.ground_img[b], s.parent);
  if (k.gsi) hipLaunchKernelGGL(k_sweep_ground, dim3((k.gsi * k.H + 255) / 256), block, 0, stream, k, s.pts, s.ground_img[b], s.parent);
  hipLaunchKernelGGL(k_sweep_union, dim3((2 * px + 255) / 256), block, 0, stream, k, s.range_img[b], s.parent);
  hipLaunchKernelGGL(k_sweep_count, per_pixel, block, 0, stream, k, s.parent, s.size, s.rows);
  hipLaunchKernelGGL(k_sweep_blocks, per_pixel, block, 0, stream, k, s.parent, s.size, s.rows, s.block_cnt);
  hipLaunchKernelGGL(k_sweep_number, per_pixel, block, 0, stream, k, s.parent, s.size, s.rows, s.block_cnt, s.num);
  hipLaunchKernelGGL(k_sweep_output, per_pixel, block, 0, stream, k, s.parent, s.num, s.pts, s.block_cnt, s.label_img[b], s.cloud[b],
                     s.n_dev, s.res_dev);
  if (s.features) {
    features_launch(*s.features, b, s.label_img[b], s.ground_img[b], s.range_img[b], s.pts, stream);
    association_launch(*s.features, b, k, s.feed.stage_dev, s.moved, s.label_img[b], s.pts, stream);   // (nothing unless it is on)
  }
  // stage two: cbSensor on the device cloud; at most one point per pixel reaches it
  PerceptionScratch& ps = s.feed;
  const VoxelView table = ps.table.view(voxel_slots_for(px), ps.counters + 2);
  const uint32_t seq = next_seq(ps.seq);
  hipLaunchKernelGGL(k_feed_insert_device, per_pixel, block, 0, stream, f, s.cloud[b], s.n_dev, table);
  hipLaunchKernelGGL(k_feed_emit, per_pixel, block, 0, stream, f, table, s.obs[b], ps.counters, ps.res_dev, seq);
  if (const int rc = feed_wait(stream, &ps.res_host->seq, seq)) return rc;
  *n_out = ps.res_host->n_out;
  *n_segmented = *reinterpret_cast<volatile uint32_t*>(&s.res_host->n_segmented);
  return 0;
}

}  // namespace dddmr
