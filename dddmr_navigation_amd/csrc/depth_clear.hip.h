// depth_clear.hip.h -- the depth camera's frustums and selfClear's clearing verdicts as HIP kernels.
//
// Restates, for the global-mode DepthCameraLayer (citations relative to dddmr_perception_3d/plugins/depth_camera/):
//   the frustum half of DepthCameraObservationBuffer::bufferCloud   depth_camera_observation_buffer.cpp:134-174
//     findFrustumVertex / findFrustumNormal / findFrustumPlane      depth_camera_observation.cpp:85-239   -> frustum_build (host)
//   FrustumUtils::isinFrustumsObservations / isAttachFRUSTUMs / isInsideFRUSTUMwoAttach
//                                                                   frustum_utils.cpp:124-290              -> dc_in_frustums, dc_attach
//   the decision tree of DepthCameraLayer::selfClear                depth_camera_layer.cpp:252-264, :324-422 -> k_dc_verdicts
//
// The observation selfClear searches (aggregatePointCloudFromObservations: every depth buffer's alive frames) already
// lives on the device, one packed run per depth source.  The runs are copied behind one another and binned into a
// uniform grid by a counting sort -- k_dc_bounds (box of the points), k_dc_shape (one lane: cell size and dimensions,
// written to a header in device memory so that the host never has to read the box back), k_dc_count, an exclusive scan,
// k_dc_scatter -- only when a depth source has published since the grid was last built.  k_dc_verdicts then takes one
// wave per marking: the wave-uniform frustum tests choose the branch, the lanes stride over the marking's stored
// cluster points, each probing the cells its 0.01 m ball touches, and the hits are counted with one ballot per round.
// The grid answers pcl::KdTreeFLANN::radiusSearch's "is there a point within r" exactly: FLANN's L2_Simple distance in
// float, kept iff dist^2 < static_cast<float>(r * r), strictly (oracle/ASSUMPTIONS.md row 1), over the cells of the ball
// widened by 0.1 mm and formed relative to the grid's origin (grid_cx(g, q, d), DESIGN section 5 on kilometre-scale
// coordinates).
//
// Arithmetic is the reference's own mix, nothing contracted: plane distances, normals and the six `test` dot products
// are float expressions (every operand is a float; `test` is only widened to double for its `< 0`), fabs / sqrt on
// floats are the float overloads (oracle/ASSUMPTIONS.md row 18: <math.h> is in scope), hypot takes (float - double)
// arguments and is the double one, dis2rej is (float)0.12.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "dev_memory.hip.h"   // Owned, dev_alloc
#include "point_grid.hip.h"   // the observation grid and its walks; rocPRIM
#include "wave_ops.hip.h"     // wave_min, wave_max

#pragma clang fp contract(off)

namespace dddmr {

constexpr int kDcMaxSources = 4;                 // == DDDMR_MAX_SOURCES
constexpr uint32_t kDcCapCells = 1u << 21;       // cells of the observation grid; the cell grows from 0.05 m until the box fits
constexpr float kDcCell = 0.05f;
// The search boxes are widened by 0.1 mm, as the marking layer's are.  That covers half an ulp of extent + r_box, which is
// all a neighbour can be lost to, while that sum is below 2048 m: static_grids_upload refuses a ground or map cloud wider
// than kSmallPadMaxExtent (point_grid_plan.hip.h has the argument, the counter-example past the limit and the search).
constexpr float kDcPad = 1e-4f;
constexpr uint8_t kDcEmptyCluster = 0x80;        // verdict flag: a ratio branch met an empty cluster (1.0 * n / 0)

// One camera's frustum in the global frame, as DepthCameraObservation holds it after bufferCloud.
struct DcFrustum {
  float vtx[8][3];      // frustum_: TLNear TRNear BLNear BRNear TLFar TRFar BLFar BRFar
  float nrm[6][3];      // frustum_normal_: near, right, bottom, left, far, top
  float pl[6][4];       // frustum_plane_equation_
  double origin[3];     // origin_ (geometry_msgs Point: doubles)
  double max_d;         // max_detect_distance_
};
struct DcFrustums {
  int n;
  DcFrustum f[kDcMaxSources];
};

// ---- host: the geometry -------------------------------------------------------------------------------------------
// R, t: Eigen::Affine3d of m2s (tf2::transformToEigen).  depth_camera_observation_buffer.cpp:148-174.
inline void frustum_build(DcFrustum& F, double fov_w, double fov_v, double min_d, double max_d, const double R[9], const double t[3]) {
  // findFrustumVertex (depth_camera_observation.cpp:114-127): double products rounded into pcl::PointXYZ floats
  const double tw = std::tan(fov_w / 2.0), tv = std::tan(fov_v / 2.0);
  const double dist[2] = {min_d, max_d};
  float v[8][3];
  for (int far = 0; far < 2; ++far) {
    const double d = dist[far];
    const float px = (float)d, pw = (float)(d * tw), nw = (float)(-d * tw), pv = (float)(d * tv), nv = (float)(-d * tv);
    const float q[4][3] = {{px, pw, pv}, {px, nw, pv}, {px, pw, nv}, {px, nw, nv}};
    for (int k = 0; k < 4; ++k)
      for (int a = 0; a < 3; ++a) v[4 * far + k][a] = q[k][a];
  }
  // pcl::transformPointCloud(frustum_, frustum_, Affine3d) (:166-167): double multiply-add, float result
  for (int k = 0; k < 8; ++k)
    for (int a = 0; a < 3; ++a)
      F.vtx[k][a] = (float)(R[3 * a + 0] * v[k][0] + R[3 * a + 1] * v[k][1] + R[3 * a + 2] * v[k][2] + t[a]);
  // findFrustumNormal (:130-200): getVec (second minus first) and getCrossProduct in float, the y term times -1.0 in double
  enum { TLN, TRN, BLN, BRN, TLF, TRF, BLF, BRF };
  auto normal = [&](int a0, int a1, int b0, int b1, float out[3]) {
    float u[3], w[3];
    for (int a = 0; a < 3; ++a) {
      u[a] = F.vtx[a1][a] - F.vtx[a0][a];
      w[a] = F.vtx[b1][a] - F.vtx[b0][a];
    }
    out[0] = u[1] * w[2] - u[2] * w[1];
    out[1] = (float)((u[0] * w[2] - u[2] * w[0]) * -1.0);
    out[2] = u[0] * w[1] - u[1] * w[0];
  };
  normal(TLN, TRN, TRN, BRN, F.nrm[0]);   // pn
  normal(TRN, TRF, TRF, BRF, F.nrm[1]);   // pr
  normal(BRN, BRF, BRF, BLF, F.nrm[2]);   // pb
  normal(BLN, BLF, BLF, TLF, F.nrm[3]);   // pl
  normal(BRF, TRF, TRF, TLF, F.nrm[4]);   // pf
  normal(TLF, TRF, TRF, TRN, F.nrm[5]);   // pt
  // findFrustumPlane / getPlaneN (:99-112, :202-239), all float
  auto plane = [&](int i1, int i2, int i3, float out[4]) {
    const float* p1 = F.vtx[i1];
    const float* p2 = F.vtx[i2];
    const float* p3 = F.vtx[i3];
    const float a1 = p2[0] - p1[0], b1 = p2[1] - p1[1], c1 = p2[2] - p1[2];
    const float a2 = p3[0] - p1[0], b2 = p3[1] - p1[1], c2 = p3[2] - p1[2];
    out[0] = b1 * c2 - b2 * c1;
    out[1] = a2 * c1 - a1 * c2;
    out[2] = a1 * b2 - b1 * a2;
    out[3] = (-out[0] * p1[0] - out[1] * p1[1] - out[2] * p1[2]);
  };
  plane(TLN, TLF, BLN, F.pl[0]);
  plane(BLN, BRN, BLF, F.pl[1]);
  plane(TRN, BRN, BRF, F.pl[2]);
  plane(TLN, TRN, TLF, F.pl[3]);
  plane(TLN, BLN, BRN, F.pl[4]);
  plane(TLF, TRF, BRF, F.pl[5]);
  for (int a = 0; a < 3; ++a) F.origin[a] = t[a];   // :148-150
  F.max_d = max_d;
}

// ---- device: the point tests --------------------------------------------------------------------------------------
// The loop body of isinFrustumsObservations / the second half of isInsideFRUSTUMwoAttach: BRNear_ = vtx[3] for the
// first three normals, TLFar_ = vtx[4] for the others.
__device__ __forceinline__ bool dc_in_frustum(const DcFrustum& F, float x, float y, float z) {
  for (int i = 0; i < 6; ++i) {
    const float* c = F.vtx[i < 3 ? 3 : 4];
    const float vx = x - c[0], vy = y - c[1], vz = z - c[2];
    const double test = vx * F.nrm[i][0] + vy * F.nrm[i][1] + vz * F.nrm[i][2];
    if (test < 0) return false;
  }
  return true;
}
__device__ __forceinline__ bool dc_in_frustums(const DcFrustums& S, float x, float y, float z) {
  for (int s = 0; s < S.n; ++s)
    if (dc_in_frustum(S.f[s], x, y, z)) return true;
  return false;
}
// `dis <= dis2rej && hypot(...) < max_detect_distance_ + 0.5` for one plane (frustum_utils.cpp:134-142, :170-177)
__device__ __forceinline__ bool dc_plane_attaches(const DcFrustum& F, int i, float x, float y, float z) {
  const float a = F.pl[i][0], b = F.pl[i][1], c = F.pl[i][2], d = F.pl[i][3];
  float dis = fabsf(a * x + b * y + c * z + d);
  dis = dis / sqrtf(a * a + b * b + c * c);
  const float dis2rej = 0.12;
  return dis <= dis2rej && hypot(x - F.origin[0], y - F.origin[1]) < F.max_d + 0.5;
}
__device__ __forceinline__ bool dc_inside_wo_attach(const DcFrustum& F, float x, float y, float z) {
  for (int i = 0; i < 6; ++i)
    if (dc_plane_attaches(F, i, x, y, z)) return false;
  return dc_in_frustum(F, x, y, z);
}
// isAttachFRUSTUMs: decided by the FIRST plane of the first camera that attaches -- true unless another camera holds
// the point inside and unattached; later planes and cameras are not asked.
__device__ __forceinline__ bool dc_attach(const DcFrustums& S, float x, float y, float z) {
  for (int s = 0; s < S.n; ++s)
    for (int i = 0; i < 6; ++i)
      if (dc_plane_attaches(S.f[s], i, x, y, z)) {
        for (int t = 0; t < S.n; ++t) {
          if (t == s) continue;
          if (dc_inside_wo_attach(S.f[t], x, y, z)) return false;
        }
        return true;
      }
  return false;
}

// One point per lane; out: bit 0 = isinFrustumsObservations, bit 1 = isAttachFRUSTUMs.  xyz and out are host-mapped.
__global__ __launch_bounds__(256) void k_dc_frustum_test(DcFrustums S, const float* __restrict__ xyz, uint32_t n,
                                                         uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  out[i] = (uint8_t)((dc_in_frustums(S, x, y, z) ? 1 : 0) | (dc_attach(S, x, y, z) ? 2 : 0));
}

// ---- device: the observation grid ---------------------------------------------------------------------------------
// floats as unsigned ints of the same order, for atomicMin / atomicMax
__device__ __forceinline__ uint32_t dc_ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dc_unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// bounds: [0..2] min x y z, [3..5] max x y z (ordered encoding; k_dc_shape leaves them at 0xFFFFFFFF / 0)
__global__ __launch_bounds__(256) void k_dc_bounds(const float4* __restrict__ pts, uint32_t n, uint32_t* __restrict__ bounds) {
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = pts[i];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
    const uint32_t e[3] = {dc_ordered(p.x), dc_ordered(p.y), dc_ordered(p.z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], e[a]);
      hi[a] = max(hi[a], e[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min(lo[a]);
    hi[a] = wave_max(hi[a]);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&bounds[a], lo[a]);
      atomicMax(&bounds[3 + a], hi[a]);
    }
  }
}

// One lane: the grid's geometry from the box (point_grid_plan.hip.h's grid_shape, on the device), into the header the
// other kernels read.  The header's cell_start / sorted pointers were set once by the host.
__global__ void k_dc_shape(uint32_t* __restrict__ bounds, PointGrid* __restrict__ hdr, uint32_t n, uint32_t cap_cells) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    const bool any = bounds[a] <= bounds[3 + a];
    lo[a] = any ? dc_unordered(bounds[a]) : 0.f;
    hi[a] = any ? dc_unordered(bounds[3 + a]) : 0.f;
    bounds[a] = 0xFFFFFFFFu;          // the next build starts from an empty box
    bounds[3 + a] = 0u;
  }
  float cell = kDcCell;
  int nx, ny, nz;
  for (int it = 0;; ++it) {
    const float ex = fminf((hi[0] - lo[0]) / cell, 1.0e6f), ey = fminf((hi[1] - lo[1]) / cell, 1.0e6f),
                ez = fminf((hi[2] - lo[2]) / cell, 1.0e6f);
    nx = max(1, (int)ceilf(ex) + 1);
    ny = max(1, (int)ceilf(ey) + 1);
    nz = max(1, (int)ceilf(ez) + 1);
    if ((unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz <= cap_cells) break;
    if (it >= 200) { nx = ny = nz = 1; break; }     // cannot happen for a finite box (1.3^200); one cell is still exact
    cell *= 1.3f;
  }
  hdr->ox = lo[0];
  hdr->oy = lo[1];
  hdr->oz = lo[2];
  hdr->inv_xy = 1.0f / cell;
  hdr->inv_z = 1.0f / cell;
  hdr->nx = nx;
  hdr->ny = ny;
  hdr->nz = nz;
  hdr->n = n;
}

__global__ __launch_bounds__(256) void k_dc_count(const PointGrid* __restrict__ hdr, const float4* __restrict__ pts,
                                                  uint32_t* __restrict__ counts, uint2* __restrict__ slot) {
  const PointGrid g = *hdr;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.n) return;
  const float4 p = pts[i];
  const uint32_t c = (uint32_t)((grid_cz(g, p.z) * g.ny + grid_cy(g, p.y)) * g.nx + grid_cx(g, p.x));
  slot[i] = make_uint2(c, atomicAdd(&counts[c], 1u));
}
__global__ __launch_bounds__(256) void k_dc_scatter(const PointGrid* __restrict__ hdr, const float4* __restrict__ pts,
                                                    const uint2* __restrict__ slot) {
  const PointGrid g = *hdr;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.n) return;
  const float4 p = pts[i];
  const uint2 s = slot[i];
  g.sorted[g.cell_start[s.x] + s.y] = make_float4(p.x, p.y, p.z, __int_as_float((int)i));
}

// ---- device: the verdicts -----------------------------------------------------------------------------------------
struct DcVerdictParams {
  double res, hres;          // resolution_, height_resolution_
  uint32_t m;                // markings
  uint32_t observation_clear;   // the observation has <= 5 points (depth_camera_layer.cpp:258-264): no search is made
};

// selfClear's decision tree for one marking by one wave (:324-422), shared by k_dc_verdicts (markings shipped by the host)
// and k_dl_verdicts (markings in the device store, depth_layer.hip.h).  vx / vy / vz: the marking's voxel key; n_pts and
// point(j) -> float3: its stored cluster pc_.  Every argument but `lane` is wave-uniform, and so is the result:
// .x = verdict (bit 0 kept, bits 1-2 branch: 1 outside the frustums, 2 attached, 3 inside; kDcEmptyCluster),
// .y = engagement count where the branch computes one.
template <class P>
__device__ __forceinline__ uint2 dc_marking_verdict(double res, double hres, bool clear, const DcFrustums& S,
                                                    const PointGrid* __restrict__ hdr, int vx, int vy, int vz, uint32_t n_pts,
                                                    int lane, P&& point) {
  // pt.x = (*it_x).first * resolution_ (:325-327): int times double, rounded to the float of pcl::PointXYZI
  const float px = (float)(vx * res);
  const float py = (float)(vy * res);
  const float pz = (float)(vz * hres);
  uint32_t verdict = 0, engaged = 0;
  if (!dc_in_frustums(S, px, py, pz)) {
    // :333-351 (taken when the voxel is in NO frustum, whatever the comment above it says)
    bool near = false;
    if (!clear) {
      const PointGrid g = *hdr;
      near = grid_radius_count(g, px, py, pz, 0.05f + kDcPad, static_cast<float>(0.05 * 0.05), 1) > 0;
    }
    verdict = (1u << 1) | (near ? 1u : 0u);
  } else {
    // :357-421: the attached and the unattached branch run the same engagement test
    const uint32_t branch = dc_attach(S, px, py, pz) ? 2u : 3u;
    verdict = branch << 1;
    if (!clear) {
      if (n_pts == 0) {
        verdict |= kDcEmptyCluster;
      } else {
        const PointGrid g = *hdr;
        const float r2 = static_cast<float>(0.01 * 0.01);
        for (uint32_t j0 = 0; j0 < n_pts; j0 += 64) {          // wave-uniform bounds
          const uint32_t j = j0 + (uint32_t)lane;
          bool hit = false;
          if (j < n_pts) {
            const float3 q = point(j);
            hit = grid_radius_count(g, q.x, q.y, q.z, 0.01f + kDcPad, r2, 1) > 0;
          }
          engaged += (uint32_t)__popcll(__ballot(hit));
        }
        // 1.0 * engage_count / pc_->points.size() > 0.1 (:374, :406)
        if (1.0 * (double)engaged / (double)n_pts > 0.1) verdict |= 1u;
      }
    }
  }
  return make_uint2(verdict, engaged);
}

// One wave per marking.  voxel / offsets / cluster are host-mapped (each is read once), out is host-mapped:
// out[i] = dc_marking_verdict's result.
__global__ __launch_bounds__(256) void k_dc_verdicts(DcVerdictParams k, DcFrustums S, const PointGrid* __restrict__ hdr,
                                                     const int32_t* __restrict__ voxel, const uint32_t* __restrict__ offsets,
                                                     const float* __restrict__ cluster, uint2* __restrict__ out) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= k.m) return;                                  // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint32_t b = offsets[i], e = offsets[i + 1];
  const uint2 v = dc_marking_verdict(k.res, k.hres, k.observation_clear != 0, S, hdr, voxel[3 * (size_t)i + 0],
                                     voxel[3 * (size_t)i + 1], voxel[3 * (size_t)i + 2], e - b, lane, [&](uint32_t j) {
                                       const size_t r = 3 * ((size_t)b + j);
                                       return make_float3(cluster[r + 0], cluster[r + 1], cluster[r + 2]);
                                     });
  if (lane == 0) out[i] = v;
}

// ---- host: scratch ------------------------------------------------------------------------------------------------
struct DepthClear {
  PointGrid* hdr = nullptr;          // device
  uint32_t* bounds = nullptr;        // device, 6 words
  float4* pts = nullptr;             // the depth sources' observations behind one another
  uint2* slot = nullptr;
  uint32_t* cell_start = nullptr;
  float4* sorted = nullptr;
  char* temp = nullptr;              // rocPRIM storage of the scan
  size_t temp_bytes = 0;
  uint32_t n_obs = 0;
  uint64_t built_epoch = 0;
  bool built = false;
  // pinned + mapped staging, grown on demand
  void* in_host = nullptr;
  void* in_dev = nullptr;
  size_t in_cap = 0;
  void* out_host = nullptr;
  void* out_dev = nullptr;
  size_t out_cap = 0;
  uint32_t launches_last = 0;        // kernels, memsets and copies the last verdict call enqueued
  Owned mem;
};

inline void dc_free(DepthClear& d) { d = DepthClear(); }

// temp_bytes: what rocPRIM's exclusive scan over kDcCapCells + 1 cells asks for (the caller's query: it needs the device)
inline int dc_alloc(DepthClear& d, size_t max_points, size_t temp_bytes) {
  const size_t np = std::max<size_t>(max_points, 1);
  DevAllocs& dev = d.mem.dev;
  d.temp_bytes = temp_bytes;
  if (dev_alloc(dev, &d.hdr, 1) != hipSuccess || dev_alloc(dev, &d.bounds, 6) != hipSuccess || dev_alloc(dev, &d.pts, np) != hipSuccess ||
      dev_alloc(dev, &d.slot, np) != hipSuccess || dev_alloc(dev, &d.cell_start, (size_t)kDcCapCells + 1) != hipSuccess ||
      dev_alloc(dev, &d.sorted, np) != hipSuccess || dev_alloc(dev, &d.temp, std::max<size_t>(temp_bytes, 16)) != hipSuccess)
    return -1;
  PointGrid g;
  g.cell_start = d.cell_start;
  g.sorted = d.sorted;
  const uint32_t b0[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
  if (hipMemcpy(d.hdr, &g, sizeof(g), hipMemcpyHostToDevice) != hipSuccess) return -1;
  if (hipMemcpy(d.bounds, b0, sizeof(b0), hipMemcpyHostToDevice) != hipSuccess) return -1;
  return 0;
}

// count -> exclusive scan -> scatter of d.pts[0 .. n) on `stream`; returns the operations enqueued, < 0 on error
inline int dc_build_grid(DepthClear& d, uint32_t n, hipStream_t stream) {
  d.n_obs = n;
  const unsigned blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_dc_bounds, dim3(std::min(blocks, 1024u)), dim3(256), 0, stream, d.pts, n, d.bounds);
  hipLaunchKernelGGL(k_dc_shape, dim3(1), dim3(64), 0, stream, d.bounds, d.hdr, n, kDcCapCells);
  if (hipMemsetAsync(d.cell_start, 0, ((size_t)kDcCapCells + 1) * sizeof(uint32_t), stream) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_dc_count, dim3(blocks), dim3(256), 0, stream, d.hdr, d.pts, d.cell_start, d.slot);
  size_t need = d.temp_bytes;
  if (rocprim::exclusive_scan(d.temp, need, d.cell_start, d.cell_start, 0u, (size_t)kDcCapCells + 1, rocprim::plus<uint32_t>(),
                              stream) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(k_dc_scatter, dim3(blocks), dim3(256), 0, stream, d.hdr, d.pts, d.slot);
  if (hipGetLastError() != hipSuccess) return -1;
  return 6;
}

}  // namespace dddmr
