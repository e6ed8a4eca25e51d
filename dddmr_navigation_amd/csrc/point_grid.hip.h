// point_grid.hip.h -- the uniform grid every spatial query of the library goes through: cell-sorted copies of a point
// set that answer the reference's kd-tree radius searches exactly (FLANN's float L2_Simple distance, strict <).  Here:
// the grid and its device walks, its storage and its builder.  The host arithmetic around it (a grid's shape, staging a
// caller's cloud, the box limits) is point_grid_plan.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>             // (rocPRIM's texture_cache_iterator.hpp calls memset without it)
#include <rocprim/rocprim.hpp>

#include "dev_memory.hip.h"    // DevAllocs, dev_alloc
#include "exact_float.hip.h"

#pragma clang fp contract(off)

namespace dddmr {

struct PointGrid {            // uniform grid over a point set; cell = (cz * ny + cy) * nx + cx
  float ox = 0, oy = 0, oz = 0;
  float inv_xy = 1, inv_z = 1;
  int nx = 1, ny = 1, nz = 1;
  uint32_t n = 0;
  uint32_t* cell_start = nullptr;   // [nx * ny * nz + 1]
  float4* sorted = nullptr;         // x y z, w = original index (bits)
};

__device__ __forceinline__ int grid_cx(const PointGrid& g, float x) { return min(max((int)floorf((x - g.ox) * g.inv_xy), 0), g.nx - 1); }
__device__ __forceinline__ int grid_cy(const PointGrid& g, float y) { return min(max((int)floorf((y - g.oy) * g.inv_xy), 0), g.ny - 1); }
__device__ __forceinline__ int grid_cz(const PointGrid& g, float z) { return min(max((int)floorf((z - g.oz) * g.inv_z), 0), g.nz - 1); }
// Cell of q + d (a search ball's edge), the origin subtracted FIRST: q - origin is a small number carried exactly or to
// ~1e-6 m, whereas q + d rounds to the float grid of q -- 0.24 mm at 4 km, more than the 0.1 mm by which the callers
// widen their balls, so that a neighbour could fall into a cell outside the range (found with the scene shifted by
// kilometres: tests/test_marking_gpu.py::test_marking_far_from_the_map_origin).
__device__ __forceinline__ int grid_cx(const PointGrid& g, float q, float d) { return min(max((int)floorf(((q - g.ox) + d) * g.inv_xy), 0), g.nx - 1); }
__device__ __forceinline__ int grid_cy(const PointGrid& g, float q, float d) { return min(max((int)floorf(((q - g.oy) + d) * g.inv_xy), 0), g.ny - 1); }
__device__ __forceinline__ int grid_cz(const PointGrid& g, float q, float d) { return min(max((int)floorf(((q - g.oz) + d) * g.inv_z), 0), g.nz - 1); }

__global__ __launch_bounds__(256) void k_grid_count(PointGrid g, const float4* __restrict__ pts, uint32_t* __restrict__ counts,
                                                    uint2* __restrict__ slot) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.n) return;
  const float4 p = pts[i];
  const uint32_t c = (uint32_t)((grid_cz(g, p.z) * g.ny + grid_cy(g, p.y)) * g.nx + grid_cx(g, p.x));
  slot[i] = make_uint2(c, atomicAdd(&counts[c], 1u));
}
__global__ __launch_bounds__(256) void k_grid_scatter(PointGrid g, const float4* __restrict__ pts, const uint2* __restrict__ slot) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.n) return;
  const float4 p = pts[i];
  const uint2 s = slot[i];
  g.sorted[g.cell_start[s.x] + s.y] = make_float4(p.x, p.y, p.z, __int_as_float((int)i));
}

// All points of the cells the ball's bounding box touches (the caller applies FLANN's float distance test).
template <class F>
__device__ __forceinline__ void grid_for_each(const PointGrid& g, float qx, float qy, float qz, float r, F&& f) {
  const int x0 = grid_cx(g, qx, -r), x1 = grid_cx(g, qx, r);
  const int y0 = grid_cy(g, qy, -r), y1 = grid_cy(g, qy, r);
  const int z0 = grid_cz(g, qz, -r), z1 = grid_cz(g, qz, r);
  const int nys = y1 - y0 + 1, nrows = nys * (z1 - z0 + 1);
  if (nrows <= 4 && nys <= 2) {
    // The usual case (a ball no wider than a cell: at most 2 x 2 rows of cells): the bounds of all rows and the first point
    // of each are loaded together, then walked in the same order -- two dependent round trips per query instead of two
    // per row (the ray tests and the "still observed" test are chains of these).
    uint32_t b[4], e[4];
    float4 first[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int q = min(rr, nrows - 1);
      const int cz = z0 + (nys == 2 ? (q >> 1) : q), cy = y0 + (nys == 2 ? (q & 1) : 0);
      const int row = (cz * g.ny + cy) * g.nx;
      b[rr] = g.cell_start[row + x0];
      e[rr] = g.cell_start[row + x1 + 1];
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      if (rr >= nrows) e[rr] = b[rr];
      first[rr] = b[rr] < e[rr] ? g.sorted[b[rr]] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      if (b[rr] < e[rr]) {
        if (f(first[rr])) return;
        for (uint32_t k = b[rr] + 1u; k < e[rr]; ++k)
          if (f(g.sorted[k])) return;
      }
    }
    return;
  }
  for (int cz = z0; cz <= z1; ++cz)
    for (int cy = y0; cy <= y1; ++cy) {
      const uint32_t b = g.cell_start[(cz * g.ny + cy) * g.nx + x0], e = g.cell_start[(cz * g.ny + cy) * g.nx + x1 + 1];
      for (uint32_t k = b; k < e; ++k)
        if (f(g.sorted[k])) return;
    }
}
// The same walk with the 64 lanes of a wave striding each row's run (one query per wave).
template <class F>
__device__ __forceinline__ void grid_for_each_wave(const PointGrid& g, float qx, float qy, float qz, float r, int lane, F&& f) {
  const int x0 = grid_cx(g, qx, -r), x1 = grid_cx(g, qx, r);
  const int y0 = grid_cy(g, qy, -r), y1 = grid_cy(g, qy, r);
  const int z0 = grid_cz(g, qz, -r), z1 = grid_cz(g, qz, r);
  for (int cz = z0; cz <= z1; ++cz)
    for (int cy = y0; cy <= y1; ++cy) {
      const uint32_t b = g.cell_start[(cz * g.ny + cy) * g.nx + x0], e = g.cell_start[(cz * g.ny + cy) * g.nx + x1 + 1];
      for (uint32_t k = b + (uint32_t)lane; k < e; k += 64) f(g.sorted[k]);
    }
}
// pcl::KdTreeFLANN::radiusSearch count with the squared radius already cast to float
__device__ __forceinline__ int grid_radius_count(const PointGrid& g, float qx, float qy, float qz, float r, float r2, int stop_at) {
  int cnt = 0;
  grid_for_each(g, qx, qy, qz, r, [&](const float4 p) {
    if (l2_simple(p.x, p.y, p.z, qx, qy, qz) < r2) ++cnt;
    return cnt >= stop_at;
  });
  return cnt;
}

// The smallest FLANN distance among the points of the cells the ball's box (half width r_box) touches, +inf without one.
// Whoever is nearer than the ball's radius is among them, so a caller that only asks "below the radius?" has the exact
// nearest neighbour of radiusSearch(q, r, ids, d2, 1).  (The particle filter once kept 3e38 for "none": its one test,
// d2 < r2_match, cannot tell that from +inf, and no real d2 reaches it -- cloud_coords_ok bounds a map's coordinates to 1e6 m.)
__device__ __forceinline__ float grid_nearest(const PointGrid& g, float qx, float qy, float qz, float r_box) {
  float best = __int_as_float(0x7F800000);
  grid_for_each(g, qx, qy, qz, r_box, [&](const float4 p) {
    best = fminf(best, l2_simple(p.x, p.y, p.z, qx, qy, qz));
    return false;
  });
  return best;
}
// The same search keeping who it was: radiusSearch keeps d2 < r2, strictly; among equals the smaller original index.
constexpr uint32_t kGridNone = 0xFFFFFFFFu;
struct GridHit { uint32_t id; float d2; };   // kGridNone and r2: no point inside the radius
__device__ __forceinline__ GridHit grid_nearest_id(const PointGrid& g, float qx, float qy, float qz, float r_box, float r2) {
  GridHit best{kGridNone, r2};
  grid_for_each(g, qx, qy, qz, r_box, [&](const float4 c) {
    const float d2 = l2_simple(c.x, c.y, c.z, qx, qy, qz);
    const uint32_t id = (uint32_t)__float_as_int(c.w);
    if (d2 < r2 && (d2 < best.d2 || (d2 == best.d2 && id < best.id))) { best.d2 = d2; best.id = id; }
    return false;
  });
  return best;
}

// ---- storage and builder (host) ---------------------------------------------------------------------------------------
struct GridBuf {              // a PointGrid with its storage
  PointGrid g;
  uint32_t cap_cells = 0, cap_points = 0;
  uint32_t max_row = 0;       // static grids: points of the fullest (y, z) row of cells
};

inline int grid_alloc(DevAllocs& mem, GridBuf& b, uint32_t cap_cells, uint32_t cap_points) {
  b.cap_cells = cap_cells;
  b.cap_points = cap_points;
  return dev_alloc(mem, &b.g.cell_start, (size_t)cap_cells + 1) == hipSuccess &&
                 dev_alloc(mem, &b.g.sorted, std::max<uint32_t>(cap_points, 1)) == hipSuccess
             ? 0
             : -1;
}

// The builder reports a failed HIP call through the context (HIPCHK and fail() of rollout_engine.hip, which declares
// both ahead of its headers): a program without a context has the grid and its storage, and no builder.
#ifdef HIPCHK
// count -> exclusive scan (rocPRIM storage `temp`) -> scatter on `stream`; `counts` doubles as cell_start
inline int grid_build(dddmr_rollout_ctx* ctx, void* temp, size_t temp_bytes, GridBuf& b, const float4* pts, uint32_t n, uint2* slot,
                      hipStream_t stream) {
  PointGrid& g = b.g;
  g.n = n;
  const size_t cells = (size_t)g.nx * g.ny * g.nz;
  HIPCHK(ctx, hipMemsetAsync(g.cell_start, 0, (cells + 1) * sizeof(uint32_t), stream));
  if (n == 0) return DDDMR_OK;
  hipLaunchKernelGGL(k_grid_count, dim3((n + 255) / 256), dim3(256), 0, stream, g, pts, g.cell_start, slot);
  HIPCHK(ctx, rocprim::exclusive_scan(temp, temp_bytes, g.cell_start, g.cell_start, 0u, cells + 1, rocprim::plus<uint32_t>(), stream));
  hipLaunchKernelGGL(k_grid_scatter, dim3((n + 255) / 256), dim3(256), 0, stream, g, pts, slot);
  return DDDMR_OK;
}
#endif

}  // namespace dddmr
