// static_layer_plan.hip.h -- the parts of the static layer's regeneration (dddmr_perception_3d/plugins/static_layer.cpp
// :233-285, :287-420) that are host arithmetic alone: the radii of the adaptive connection search, the cell sizes of the
// three grids and the edge-capacity decision.  No HIP call and no HIP type, so that tests/cpp/static_layer_plan_test.cpp
// builds it with a plain host compiler; static_layer.hip.h calls the same functions.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace dddmr {

// The adaptive search (:244-260, :299-315): `float search_r = 0.5; int search_cnt = 1;` and radiusSearch(node,
// search_r + 0.2 * search_cnt) until the count reaches adaptive_connection_number or hard_interrupt_cnt (100) runs out:
// search_cnt 1 .. 101.
constexpr int kSlAdaptiveSteps = 101;
constexpr uint32_t kSlMaxAdaptiveNumber = 32;
constexpr double sl_adaptive_radius(int k) { return (double)0.5f + 0.2 * (double)k; }   // (constexpr: the kernels call it too)
// radiusSearch(p, r) keeps d2 < float(double(r) * double(r)) (FLANN's float distance against PCL's cast radius)
inline float sl_radius2(double r) { return (float)(r * r); }

// By how much the search boxes are widened: kMclPad's argument (mcl_measure.hip.h).  The distance test decides; the pad
// only has to cover the rounding of (q - origin) + r against (p - origin), three float operations of half an ulp each on
// numbers no larger than the cloud's extent plus the radius.  The extent is at most 4096 m (the build refuses more) and
// the radii at most kSlMaxRadius, so the numbers stay below 8192 m, where an ulp is 4.9e-4 m: 1.5 of them are under the pad.
constexpr float kSlPad = 1e-3f;
constexpr double kSlMaxRadius = 1000.0;

// Cell sizes.  Ground: the connection ball is about four cells wide (the adaptive search starts at r_1 = 0.7 m and most
// nodes stop there).  Map: the nearest-obstacle ball (inscribed_radius) and the overhang box (1 m x 1 m x 0.9 m) are two
// to three cells wide.  Zones: the inflation ball is about three cells wide.  grid_shape coarsens a cell that would
// need more cells than the grid owns.
inline float sl_clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline float sl_ground_cell(bool adaptive, double radius_of_ground_connection) {
  const float r = adaptive ? (float)sl_adaptive_radius(1) : (float)radius_of_ground_connection;
  return sl_clampf(0.5f * (r + kSlPad), 0.05f, 64.0f);
}
inline float sl_map_cell(double inscribed_radius) { return sl_clampf((float)inscribed_radius, 0.25f, 4.0f); }
inline float sl_zone_cell(double inflation_distance) { return sl_clampf((float)inflation_distance, 0.25f, 4.0f); }

// The decision between the degree pass and the fill pass: the graph is written only when every edge fits.
inline bool sl_edges_fit(uint64_t n_edges, uint32_t max_edges) { return n_edges <= (uint64_t)max_edges; }

}  // namespace dddmr
