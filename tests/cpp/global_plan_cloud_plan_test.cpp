// Checks csrc/global_plan_cloud_plan.hip.h (the kd-tree wrapper's squared radius, the line of sight's sample sequence, the
// cost of a successor and the shell rule of the 8-nearest search) from a plain host build against values worked out by
// hand (a_star_on_pc.cpp:168-198, :288; nanoflann_pcl.hpp:189-213).  Prints "global plan cloud arithmetic OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "global_plan_cloud_plan.hip.h"

using namespace dddmr;

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("line %d: %s\n", __LINE__, #c);                     \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// the r of every sample of an edge along x of length dx
static std::vector<float> march(float dx, double inscribed, float* dt_out) {
  const float dt = gp_cloud_los_dt(dx, 0.f, 0.f, inscribed);
  *dt_out = dt;
  std::vector<float> r;
  const uint32_t n = gp_cloud_los_samples(dt);
  for (uint32_t k = 0; k < n && k < 64; ++k) r.push_back(gp_cloud_los_r(gp_cloud_los_t(dt, k)));
  CHECK(n > kGpLosMaxSamples || r.size() == n || n > 64);
  return r;
}

int main() {
  static_assert(kGpRowFull == 4 && kGpCloudMaxSuccessors == 1024 && kGpLosMaxSamples == 4096 && kGpCloudKnn == 8, "the header's constants");
  // the radius: to float first, squared in float.  0.3 -> 0x3e99999a, squared 0.09 -> 0x3db851ec; 0.5 * 0.5 is exact
  CHECK(bits(gp_cloud_radius2(0.5)) == bits(0.25f));
  CHECK(bits(gp_cloud_radius2(2.0 * 0.15)) == 0x3db851ecu);
  CHECK(bits(gp_cloud_radius2(1e-30)) == bits((float)1e-30 * (float)1e-30));   // (underflows to 0 in float, not in double)

  // an edge of exactly 2 * inscribed_radius is marched (>=), the float below is not
  CHECK(gp_cloud_los_needed(0.0625f, 0.125));
  CHECK(!gp_cloud_los_needed(std::nextafterf(0.0625f, 0.f), 0.125));
  CHECK(gp_cloud_los_needed(std::nextafterf(0.0625f, 1.f), 0.125));
  CHECK(!gp_cloud_los_needed(0.f, 0.125));                                      // the node itself
  // (double)sqrtf(0.09f) = 0.300000011920929 >= 2 * 0.15 = 0.3 in double: marched
  CHECK(gp_cloud_los_needed(0.09f, 0.15));

  float dt = 0.f;
  // 0.25 m at 0.125: distance 2, dt 0.5; t = 0, 0.5, 1.0, 1.5 <= 1.5: r = 1 is visited twice; t = 2.0 ends it
  std::vector<float> r = march(0.25f, 0.125, &dt);
  CHECK(bits(dt) == bits(0.5f));
  CHECK(r.size() == 4 && r[0] == 0.f && r[1] == 0.5f && r[2] == 1.f && r[3] == 1.f);
  // 0.9 m at 0.15: dt = 1/6 = 0x3e2aaaab; six additions give exactly 1.0, the seventh 1.1666666 <= 1 + dt: r = 1 twice, 8 samples
  r = march(0.9f, 0.15, &dt);
  CHECK(bits(dt) == 0x3e2aaaabu);
  CHECK(r.size() == 8 && bits(r[5]) == 0x3f555556u && r[6] == 1.f && r[7] == 1.f);
  CHECK(bits(gp_cloud_los_t(dt, 7)) == 0x3f955555u);
  // 0.45 m at 0.15: dt = 1/3 = 0x3eaaaaab; t = 0, 1/3, 2/3, 1.0, then 1.3333334 in float, above 1 + dt in double: r = 1 once, 4 samples
  r = march(0.45f, 0.15, &dt);
  CHECK(bits(dt) == 0x3eaaaaabu);
  CHECK(r.size() == 4 && bits(r[2]) == 0x3f2aaaabu && r[3] == 1.f);
  CHECK(!gp_cloud_los_goes_on(gp_cloud_los_t(dt, 4), dt));
  // 2.5 m at 0.15: distance 16.666666, dt 0.060000002 = 0x3d75c290; t passes 1.0 between sample 16 (0.96000004) and sample 17
  // (1.02, r = 1), and 1.08 is beyond 1 + dt: 18 samples
  r = march(2.5f, 0.15, &dt);
  CHECK(bits(dt) == 0x3d75c290u);
  CHECK(gp_cloud_los_samples(dt) == 18);
  CHECK(r.size() == 18 && bits(r[16]) == 0x3f75c290u && r[17] == 1.f);
  CHECK(bits(gp_cloud_los_t(dt, 17)) == 0x3f828f5cu);                           // (accumulated, not 17 * dt)
  // the cap: 700 m at 0.15 would take 4667 samples
  CHECK(gp_cloud_los_samples(gp_cloud_los_dt(700.f, 0.f, 0.f, 0.15)) == kGpLosMaxSamples + 1);
  CHECK(gp_cloud_los_samples(gp_cloud_los_dt(600.f, 0.f, 0.f, 0.15)) <= kGpLosMaxSamples);
  CHECK(gp_cloud_los_samples(0.f) == kGpLosMaxSamples + 1);                     // dt 0: the reference's loop does not end
  CHECK(gp_cloud_los_samples(INFINITY) == kGpLosMaxSamples + 1);                // distance 0: t stays at +inf <= +inf
  // a sample's coordinate: the product rounded, then the sum rounded (no fused multiply-add)
  {
    const float cur = 1.0f, d = 0.1f, rr = 0.3f;
    const float prod = d * rr;
    CHECK(bits(gp_cloud_los_coord(cur, d, rr)) == bits(cur + prod));
    CHECK(gp_cloud_los_coord(4000.25f, 0.25f, 1.0f) == 4000.5f);
  }

  // new_g: (g + edge) in float, then double sums left to right.  1.5 + 0.25 = 1.75; + 0.5 + 0.125 + 0.75 * 0.1 + 0.0625 = 2.5125
  CHECK(bits(gp_cloud_new_g(1.5f, 0.25f, 0.5, 0.125f, 0.75, 0.1, 0.0625f)) == bits(2.5125f));
  // the float sum comes first: 16777216 + 1 is 16777216 in float, and the double terms cannot bring the 1 back
  CHECK(gp_cloud_new_g(16777216.f, 1.f, 0.0, 0.f, 0.0, 0.0, 0.f) == 16777216.f);
  CHECK(gp_cloud_new_g(0.f, 0.f, 1.0, 0.f, 0.0, 0.0, 0.f) == 1.f);
  CHECK(gp_cloud_avg_intensity(0.75f, 3) == 0.25f);
  CHECK(bits(gp_cloud_avg_intensity(1.0f, 3)) == 0x3eaaaaabu);

  // the shell rule: 8 points inside the ball the box is sure to contain, or a box that is the whole grid
  CHECK(!gp_cloud_shell_accepts(7, false) && gp_cloud_shell_accepts(8, false) && gp_cloud_shell_accepts(0, true));
  for (float h = 0.5f; h < 8192.f; h *= 2.f) {
    const float d2 = gp_cloud_shell_d2(h);
    CHECK(d2 > 0.f && std::sqrt((double)d2) < (double)h - 2e-3 && std::sqrt((double)d2) > 0.99 * (double)h - 3e-3);
  }
  CHECK(gp_cloud_shell_d2(1e-3f) == 0.f);

  if (failures) return 1;
  std::printf("global plan cloud arithmetic OK\n");
  return 0;
}
