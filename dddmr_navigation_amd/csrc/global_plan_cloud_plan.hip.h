// global_plan_cloud_plan.hip.h -- the arithmetic of the global planner's default A* (dddmr_global_planner/src/a_star_on_pc.cpp,
// A_Star_on_Graph::getPath :200-329 and isLineOfSightClear :168-198) that is a pure function of its arguments and that
// global_plan_plan.hip.h does not have already: the squared radius of the kd-tree wrapper, the line of sight's sample
// sequence, the cost of one successor and the rule by which the 8-nearest search accepts a shell.  No HIP call and no HIP
// type, so that tests/cpp/global_plan_cloud_plan_test.cpp builds it with a plain host compiler; global_plan_cloud.hip.h
// calls the same functions from its kernel.  DESIGN.md 4d-5 restates every expression with its line.
#pragma once
#include "global_plan_plan.hip.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace dddmr {

constexpr uint32_t kGpRowFull = 4;                 // dddmr_global_plan_result.status, beside global_plan_plan.hip.h's four
constexpr uint32_t kGpCloudMaxSuccessors = 1024;   // DDDMR_GLOBAL_PLAN_CLOUD_MAX_SUCCESSORS
constexpr uint32_t kGpLosMaxSamples = 4096;        // DDDMR_GLOBAL_PLAN_LOS_MAX_SAMPLES
constexpr uint32_t kGpCloudKnn = 8;                // :243-244  fewer than 8 in the radius: the 8 nearest instead

// nanoflann_pcl.hpp:189-213  radiusSearch(point, float radius, ...): the double argument becomes a float at the call and
// is squared in float (:202); RadiusResultSet::addPoint keeps dist < radius, strictly.  Not sl_radius2, which squares in
// double.
DDDMR_GP_HD float gp_cloud_radius2(double radius) {
  const float r = (float)radius;
  return r * r;
}

// :257, :273  current_expanding_g = sqrt(d2) in float; the line of sight is tested when it is >= 2 * inscribed_radius,
// a float against a double
DDDMR_GP_HD bool gp_cloud_los_needed(float d2, double inscribed_radius) { return (double)sqrtf(d2) >= 2.0 * inscribed_radius; }

// :171-180  distance = sqrt(dX*dX + dY*dY + dZ*dZ) in float, divided by inscribed_radius in double and stored as a float;
// dt = 1 / distance in float
DDDMR_GP_HD float gp_cloud_los_dt(float dX, float dY, float dZ, double inscribed_radius) {
  float distance = sqrtf((dX * dX + dY * dY) + dZ * dZ);
  distance = (float)((double)distance / inscribed_radius);
  return 1.0f / distance;
}
// :181  for (float t = 0; t <= 1.0 + dt; t += dt): the end test in double, t accumulated in float
DDDMR_GP_HD bool gp_cloud_los_goes_on(float t, float dt) { return (double)t <= 1.0 + (double)dt; }
// :182-184  r = t, 1 from t >= 1.0 on
DDDMR_GP_HD float gp_cloud_los_r(float t) { return t >= 1.0f ? 1.0f : t; }
// the t of sample k: k additions of dt to 0, in float (not k * dt)
DDDMR_GP_HD float gp_cloud_los_t(float dt, uint32_t k) {
  float t = 0.f;
  for (uint32_t i = 0; i < k; ++i) t += dt;
  return t;
}
// How many samples the loop of :181 visits, kGpLosMaxSamples + 1 where it would visit more than kGpLosMaxSamples (the
// reference's own loop stops advancing near 2^24 samples, and never ends for dt == 0 or a dt that is not a number).
DDDMR_GP_HD uint32_t gp_cloud_los_samples(float dt) {
  uint32_t n = 0;
  for (float t = 0.f; gp_cloud_los_goes_on(t, dt); t += dt) {
    if (++n > kGpLosMaxSamples) break;
  }
  return n;
}
// :187-189  one coordinate of a sample, in float: two roundings
DDDMR_GP_HD float gp_cloud_los_coord(float cur, float d, float r) {
  const float m = d * r;
  return cur + m;
}

// :288  float new_g = current.g + current_expanding_g + factor * 1.0 + node_weight + theta * turning_weight_ + avg_intensity:
// the first sum in float, the others in double, left to right, the result a float
DDDMR_GP_HD float gp_cloud_new_g(float g, float edge, double factor, float node_weight, double theta, double turning_weight, float avg_intensity) {
  const float ge = g + edge;
  return (float)(((((double)ge + factor * 1.0) + (double)node_weight) + theta * turning_weight) + (double)avg_intensity);
}

// :248-252  the float sum over the list in list order, divided by the list's size (a size_t, converted to float)
DDDMR_GP_HD float gp_cloud_avg_intensity(float sum, uint32_t n) { return sum / (float)n; }

// The 8-nearest search walks the cells of a box of half width h around the node.  A point the walk does not see is
// farther than h less the rounding of the cell functions ((q - origin) + h against p - origin: below 1e-3 m for the
// clouds a build accepts, kSlPad's argument) on one axis at least, so its float distance squared is above
// (h - 1e-3)^2 (1 - 3 * 2^-23).  The shell is accepted once 8 points lie at d2 <= gp_cloud_shell_d2(h), a bound that
// stays below that with room to spare; the 8 smallest (d2, id) of the walk are then the 8 smallest of the cloud, equal
// distances included.  0 for a box too small to promise anything.
DDDMR_GP_HD float gp_cloud_shell_d2(float h) {
  const float hm = h * 0.999f - 2e-3f;
  return hm > 0.f ? hm * hm : 0.f;
}
DDDMR_GP_HD bool gp_cloud_shell_accepts(uint32_t n_inside, bool box_covers_the_grid) { return box_covers_the_grid || n_inside >= kGpCloudKnn; }

}  // namespace dddmr
