// point_grid_plan.hip.h -- the host arithmetic around a PointGrid (point_grid.hip.h): the grid's shape over a box, the
// cell functions on the host, staging a caller's strided cloud as float4 records with their box or as packed xyz, and the limits a cloud
// has to keep for the search pads to hold.  Host code only -- no HIP runtime call, no context -- so that
// tests/cpp/point_grid_plan_test.cpp runs it on a machine without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "point_grid.hip.h"

namespace dddmr {

// Grid geometry over [lo, hi] with the wanted cell sizes, coarsened until it fits `cap_cells`.
inline void grid_shape(PointGrid& g, const float lo[3], const float hi[3], float cell_xy, float cell_z, uint32_t cap_cells) {
  for (;;) {
    g.nx = std::max(1, (int)std::ceil((hi[0] - lo[0]) / cell_xy) + 1);
    g.ny = std::max(1, (int)std::ceil((hi[1] - lo[1]) / cell_xy) + 1);
    g.nz = std::max(1, (int)std::ceil((hi[2] - lo[2]) / cell_z) + 1);
    if ((uint64_t)g.nx * g.ny * g.nz <= cap_cells) break;
    cell_xy *= 1.3f;
    cell_z *= 1.3f;
  }
  g.ox = lo[0]; g.oy = lo[1]; g.oz = lo[2];
  g.inv_xy = 1.0f / cell_xy;
  g.inv_z = 1.0f / cell_z;
}

// grid_cx / grid_cy / grid_cz of point_grid.hip.h on the host (same float operations)
inline int host_cx(const PointGrid& g, float x) { return std::min(std::max((int)std::floor((x - g.ox) * g.inv_xy), 0), g.nx - 1); }
inline int host_cy(const PointGrid& g, float y) { return std::min(std::max((int)std::floor((y - g.oy) * g.inv_xy), 0), g.ny - 1); }
inline int host_cz(const PointGrid& g, float z) { return std::min(std::max((int)std::floor((z - g.oz) * g.inv_z), 0), g.nz - 1); }

// a caller's cloud argument: n records of at least x y z, float-aligned
inline bool cloud_arg_ok(const float* xyz, size_t n, size_t stride_bytes) {
  return !n || (xyz && stride_bytes >= 12 && stride_bytes % 4 == 0);
}

// n records (stride_bytes apart, x y z first) into out[0 .. n) as float4 with w = 0, each through transform(v) (v: the
// three coordinates, changed in place), and the box of what was written (zeros without a point).  False when a coordinate
// was not finite, before or after the transform; `out` and the box are then of no use (a caller that refuses reads neither).
template <class Transform = void (*)(float*)>
inline bool stage_cloud(const float* xyz, size_t n, size_t stride_bytes, float4* out, float lo[3], float hi[3], Transform transform = [](float*) {}) {
  const size_t sf = stride_bytes / sizeof(float);
  bool finite = true;
  for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0.f;
  for (size_t i = 0; i < n; ++i) {
    const float* p = xyz + i * sf;
    float v[3] = {p[0], p[1], p[2]};
    finite = finite && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
    transform(v);
    for (int a = 0; a < 3; ++a) {
      finite = finite && std::isfinite(v[a]);
      lo[a] = i ? std::min(lo[a], v[a]) : v[a];
      hi[a] = i ? std::max(hi[a], v[a]) : v[a];
    }
    out[i] = make_float4(v[0], v[1], v[2], 0.f);
  }
  return finite;
}

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

// A staged cloud that owns its records (one zero element without a point).  It refuses nothing: whoever has to looks at
// `finite` (the normals of mcl_set_map and the marking layers' static clouds go through as they are).
struct HostCloud {
  std::vector<float4> pts;
  float lo[3], hi[3];
  bool finite;
  HostCloud(const float* xyz, size_t n, size_t stride_bytes) : pts(std::max<size_t>(n, 1), make_float4(0.f, 0.f, 0.f, 0.f)) {
    finite = stage_cloud(xyz, n, stride_bytes, pts.data(), lo, hi);
  }
};

// The limits the search pads rest on (kMclPad's argument, mcl_measure.hip.h): finite coordinates within 1e6 m, and a box no
// wider than kCloudMaxExtent on any axis.
constexpr float kCloudMaxExtent = 4096.0f;
inline bool cloud_box_ok(const float lo[3], const float hi[3]) {
  for (int a = 0; a < 3; ++a)
    if (!(std::fabs(lo[a]) <= 1e6f) || !(std::fabs(hi[a]) <= 1e6f) || !(hi[a] - lo[a] <= kCloudMaxExtent)) return false;
  return true;
}
// The widest static cloud whose search boxes a pad of 1e-4 m covers (the marking and depth layers': kDcPad and the
// marking layer's `pad`).  A neighbour with d2 < r2 can land in a cell outside the walked range only when
// p - q > r_box - ulp / 2, the ulp being that of extent + r_box: the three roundings of (q - origin) + r_box and of
// p - origin can add up to 1.5 ulp, and the float grid both sides land on takes a whole ulp of it back.  A pad of at least
// half that ulp is therefore safe: 1e-4 m while extent + r_box stays below 2048 m (ulp 1.22e-4), and the widest box
// half width of those layers (the inflation radius) has 48 m of room under this limit.  Past 2048 m it is not:
// origin -1986.9237060546875, q = 61.126224517822266, p = 61.07622528076172 on the ground grid (0.5 m cells, r = 0.05)
// have d2 < r2 with p in cell 4095 and the box starting at cell 4096 (tests/test_point_grid_cpu.py keeps the triple and
// the search that found it; none was found below the limit).
constexpr float kSmallPadMaxExtent = 2000.0f;
inline bool small_pad_extent_ok(const float lo[3], const float hi[3]) {
  for (int a = 0; a < 3; ++a)
    if (hi[a] - lo[a] > kSmallPadMaxExtent) return false;      // (a NaN passes: these layers take a cloud as it is)
  return true;
}
// every coordinate within the limits: the box is the cloud's only once nothing in it is NaN (std::min and max pass one by)
inline bool cloud_coords_ok(const HostCloud& h) { return h.finite && cloud_box_ok(h.lo, h.hi); }

}  // namespace dddmr
