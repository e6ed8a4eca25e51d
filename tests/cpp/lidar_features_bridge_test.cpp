// sweepFeatures() of perception_bridge.h WITHOUT ROS or a GPU: instantiated with a stand-in cloud type against a fake
// C-ABI that records the calls.  Checked: the two-call protocol (size first with null outputs, then the points with no
// index output), source and `which` passed through, points and rings, an empty list (one call), a list that grew between
// the two calls, the library's codes handed back with the output left alone, and a null context.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct Cloud { std::vector<PointXYZI> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int rc = DDDMR_OK, calls = 0, source = -1, which = -1, grow = 0, index_asked = 0;
  std::vector<float> list[3];                                             // what the "device" holds: x y z ring
} F;
extern "C" {
int dddmr_rollout_get_lidar_sweep_features(dddmr_rollout_ctx*, int32_t source, int which, float* out, uint32_t* seg_index, size_t capacity,
                                           size_t* n_points) {
  ++F.calls; F.source = source; F.which = which;
  if (seg_index) ++F.index_asked;
  if (F.rc != DDDMR_OK) return F.rc;
  if (which < 0 || which > 2) return DDDMR_ERR_BAD_ARG;
  std::vector<float>& l = F.list[which];
  if (out && F.grow) { l.resize(l.size() + 4 * (size_t)F.grow, 1.f); F.grow = 0; }      // another sweep came in
  *n_points = l.size() / 4;
  if (!out) return DDDMR_OK;
  if (capacity < *n_points) return DDDMR_ERR_CAPACITY;
  std::memcpy(out, l.data(), l.size() * sizeof(float));
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  Cloud out;
  out.points.resize(3);
  assert(sweepFeatures(&ctx, 1, 2, out) == DDDMR_OK && out.points.empty() && F.calls == 1 && F.source == 1 && F.which == 2);   // empty: one call
  F.list[1] = {1.f, 2.f, 3.f, 0.f, 4.f, 5.f, 6.f, 0.f, 7.f, 8.f, 9.f, 15.f};
  F.list[2] = {-1.f, -2.f, -3.f, 4.f};
  assert(sweepFeatures(&ctx, 3, 1, out) == DDDMR_OK && out.points.size() == 3 && F.calls == 3 && F.source == 3 && F.which == 1);
  assert(out.points[1].x == 4.f && out.points[1].y == 5.f && out.points[1].z == 6.f && out.points[1].intensity == 0.f);
  assert(out.points[2].intensity == 15.f);
  assert(sweepFeatures(&ctx, 3, 2, out) == DDDMR_OK && out.points.size() == 1 && out.points[0].z == -3.f && out.points[0].intensity == 4.f);
  assert(sweepFeatures(&ctx, 3, 0, out) == DDDMR_OK && out.points.empty());
  assert(F.index_asked == 0);
  // the list grew between the two calls: the library's code comes back, the output is what it was
  assert(sweepFeatures(&ctx, 3, 1, out) == DDDMR_OK && out.points.size() == 3);
  F.grow = 2;
  assert(sweepFeatures(&ctx, 3, 1, out) == DDDMR_ERR_CAPACITY && out.points.size() == 3);
  assert(sweepFeatures(&ctx, 3, 7, out) == DDDMR_ERR_BAD_ARG && out.points.size() == 3);
  for (int code : {DDDMR_ERR_STATE, DDDMR_ERR_HIP}) {                     // features off / not a sweep source; a device error
    F.rc = code;
    assert(sweepFeatures(&ctx, 2, 1, out) == code && out.points.size() == 3);
  }
  F.rc = DDDMR_OK;
  const int calls = F.calls;
  assert(sweepFeatures(static_cast<dddmr_rollout_ctx*>(nullptr), 1, 1, out) == DDDMR_ERR_BAD_ARG && F.calls == calls);
  std::printf("lidar features bridge OK\n");
  return 0;
}
