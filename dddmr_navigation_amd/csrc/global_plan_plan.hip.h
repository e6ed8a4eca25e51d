// global_plan_plan.hip.h -- the arithmetic of the pre-graph global planner (dddmr_global_planner/src/a_star_on_pre_graph.cpp,
// A_Star_on_PreGraph::getPath :191-289 and getThetaFromParent2Expanding :133-157) that is a pure function of its
// arguments: the frontier's key, the edge filter, the turning angle and the cost of one successor.  No HIP call and no HIP
// type, so that tests/cpp/global_plan_plan_test.cpp builds it with a plain host compiler; global_plan.hip.h calls the same
// functions from its kernel.  DESIGN.md 4d-4 restates every expression with its line.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define DDDMR_GP_HD __host__ __device__ inline
#else
#define DDDMR_GP_HD inline
#endif

namespace dddmr {

// dddmr_global_plan_result.status
constexpr uint32_t kGpFound = 0, kGpNoPath = 1, kGpBudget = 2, kGpOpenFull = 3;
constexpr uint32_t kGpNone = 0xFFFFFFFFu;      // "no node" of nearest, "no entry" of the frontier

// The frontier is a std::set<std::pair<float, unsigned>> (a_star_on_pre_graph.h: f_p_): its order is (f, index).  The key
// orders the same way as an unsigned 64-bit number for every f that is not NaN, negative ones and -0 < +0 excepted
// (-0.0f == 0.0f in the pair's compare; a cost here is a sum of non-negative terms, and +0 is the only zero it can be):
// the float's bits with the sign bit flipped for f >= 0 and all bits flipped for f < 0, then the index.
DDDMR_GP_HD uint32_t gp_float_bits(float f) {
  union { float f; uint32_t u; } v;
  v.f = f;
  return v.u;
}
DDDMR_GP_HD float gp_bits_float(uint32_t u) {
  union { float f; uint32_t u; } v;
  v.u = u;
  return v.f;
}
DDDMR_GP_HD uint32_t gp_order_bits(float f) {
  const uint32_t u = gp_float_bits(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DDDMR_GP_HD uint64_t gp_key(float f, uint32_t index) { return ((uint64_t)gp_order_bits(f) << 32) | (uint64_t)index; }
DDDMR_GP_HD uint32_t gp_key_index(uint64_t key) { return (uint32_t)key; }
DDDMR_GP_HD float gp_key_f(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return gp_bits_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// :203, :248  sqrt(pcl::geometry::squaredDistance(a, b)), the float overload
DDDMR_GP_HD float gp_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// :222, :229  an edge longer than the expanding radius (float against double) or onto a node nearer to an obstacle than the
// inscribed radius is not a successor
DDDMR_GP_HD bool gp_edge_skipped(float weight, double expanding_radius, double dgraph_value, double inscribed_radius) {
  return (double)weight > expanding_radius || dgraph_value < inscribed_radius;
}

// :240
DDDMR_GP_HD double gp_factor(double rate, double dgraph_value, double inscribed_radius) { return exp(-1.0 * rate * (dgraph_value - inscribed_radius)); }

// :133-157 up to the acos: the float cosine, clamped (:143-144).  NaN where a vector is zero; the rules below zero that.
DDDMR_GP_HD float gp_cos_theta(float vx1, float vy1, float vx2, float vy2) {
  float c = (vx1 * vx2 + vy1 * vy2) / (sqrtf(vx1 * vx1 + vy1 * vy1) * sqrtf(vx2 * vx2 + vy2 * vy2));
  if (fabsf(c) > 1.f) c = 1.0f;
  return c;
}
// :145-156 behind the acos.  acos_double: acos of the float cosine computed in double; the reference calls the float
// overload, whose correctly rounded value this rounds to.
DDDMR_GP_HD double gp_theta_rules(float vx1, float vy1, float vx2, float vy2, double acos_double) {
  double theta = (double)(float)acos_double;
  if (vx1 == 0.f && vy1 == 0.f) theta = 0;
  else if (vx2 == 0.f && vy2 == 0.f) theta = 0;
  else if ((double)fabsf(fabsf(vx1) - fabsf(vx2)) <= 0.0001) theta = 0;
  if (fabs(theta) <= 0.345) theta = 0.0;     // cap (NaN passes through, as in the reference)
  return theta;
}
// parent -> current -> expanding, x and y only
DDDMR_GP_HD double gp_theta(float px, float py, float cx, float cy, float ex, float ey) {
  const float vx1 = cx - px, vy1 = cy - py, vx2 = ex - cx, vy2 = ey - cy;
  return gp_theta_rules(vx1, vy1, vx2, vy2, acos((double)gp_cos_theta(vx1, vy1, vx2, vy2)));
}

// :245-246  float new_g = current.g + weight + factor * 1.0 + theta * turning_weight + intensity[current]: the first sum
// in float, the others in double, left to right
DDDMR_GP_HD float gp_new_g(float g, float weight, double factor, double theta, double turning_weight, float intensity) {
  const float gw = g + weight;
  return (float)((((double)gw + factor * 1.0) + theta * turning_weight) + (double)intensity);
}

// What a row's lane decides for its successor once the record of the node is read: 0 nothing, 1 the record is written,
// 2 the record is written and an entry (f, index) is filed.  An opened node is updated only by a smaller g (:258); the
// entry of an update whose f equals the node's current f is the pair the set already holds, so it is not filed again.
DDDMR_GP_HD int gp_file(bool closed, bool opened, float stored_g, float stored_f, float new_g, float new_f) {
  if (closed) return 0;
  if (!opened) return 2;
  if (!(stored_g > new_g)) return 0;
  return gp_float_bits(stored_f) == gp_float_bits(new_f) ? 1 : 2;
}

}  // namespace dddmr
