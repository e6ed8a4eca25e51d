// mcl_submap_plan.hip.h -- the parts of SubMaps (dddmr_mcl_3dl/src/sub_maps.cpp) that are host arithmetic alone: the
// transform of a keyframe's points (readPoseGraph, :126-156) and the keyframe radius search of warmUpThread (:225-235).
// No HIP call and no HIP type, so that tests/cpp/submap_plan_test.cpp builds it with a plain host compiler;
// mcl_submap.hip.h calls the same functions from dddmr_rollout_submap_add_keyframe and _submap_select.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace dddmr {

// pcl::transformPointCloud(cloud, cloud, Affine3d) for one coordinate: the double expression, rounded to float once.
// T is 3 x 4 row-major; `row` 0 .. 2.  (The translation unit switches floating-point contraction off.)
inline float submap_transform_row(const double* T, int row, float x, float y, float z) {
  const double* t = T + 4 * row;
  return (float)(t[0] * x + t[1] * y + t[2] * z + t[3]);
}

// kdtree_poses_.radiusSearch(pose, sub_map_search_radius, ...): position and keyframe positions as floats, FLANN's
// L2_Simple in float (x, y, z order), kept where d2 <= float(radius * radius).  Ids ascending (this library's order;
// the reference's unsorted result has the tree's traversal order).  kf_pos: [n][3].  ids_out may be null (count only);
// returns the count, which may exceed `capacity` (nothing is written beyond it).
inline size_t submap_select(const float* kf_pos, size_t n, const double position[3], double radius, int32_t* ids_out, size_t capacity) {
  const float px = (float)position[0], py = (float)position[1], pz = (float)position[2];
  const float r2 = (float)(radius * radius);
  size_t cnt = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* k = kf_pos + 3 * i;
    float d2 = 0.0f;
    const float dx = k[0] - px, dy = k[1] - py, dz = k[2] - pz;
    d2 += dx * dx;
    d2 += dy * dy;
    d2 += dz * dz;
    if (d2 <= r2) {
      if (ids_out && cnt < capacity) ids_out[cnt] = (int32_t)i;
      ++cnt;
    }
  }
  return cnt;
}

}  // namespace dddmr
