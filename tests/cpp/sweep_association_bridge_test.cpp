// sweepAssociation() of perception_bridge.h WITHOUT ROS or a GPU: instantiated with stand-in cloud and message types
// against a fake C-ABI that records the calls.  Checked: the two-call protocol per cloud (size first with null outputs,
// then the points with no index output), source, `which` and `frame` passed through, the four clouds, the outliers and
// the three orientation fields, empty clouds (one call each), the library's codes handed back with EVERY output left
// alone whichever call fails, and a null context.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct Cloud { std::vector<PointXYZI> points; };
struct CloudInfo { float start_orientation = -1.f, end_orientation = -1.f, orientation_diff = -1.f; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int calls = 0, fail_at = -1, fail_code = DDDMR_OK, source = -1, frame = -1, index_asked = 0, grow = 0;
  float orient[3] = {0.25f, 6.5f, 6.25f};
  std::vector<float> cloud[5];                                          // sharp, less sharp, flat, less flat, outliers: x y z i
  std::vector<int> which_seen;
  int answer(std::vector<float>& l, float* out, size_t capacity, size_t* n) {
    if (out && grow) { l.resize(l.size() + 4 * (size_t)grow, 1.f); grow = 0; }
    *n = l.size() / 4;
    if (!out) return DDDMR_OK;
    if (capacity < *n) return DDDMR_ERR_CAPACITY;
    std::memcpy(out, l.data(), l.size() * sizeof(float));
    return DDDMR_OK;
  }
  bool failing() { return calls++ == fail_at; }
} F;
extern "C" {
int dddmr_rollout_get_lidar_sweep_orientation(dddmr_rollout_ctx*, int32_t source, float out[3], int32_t* half_index) {
  if (F.failing()) return F.fail_code;
  F.source = source;
  assert(out && !half_index);
  std::memcpy(out, F.orient, sizeof(F.orient));
  return DDDMR_OK; }
int dddmr_rollout_get_lidar_sweep_association(dddmr_rollout_ctx*, int32_t source, int which, int frame, float* out, uint32_t* seg_index,
                                              size_t capacity, size_t* n) {
  if (F.failing()) return F.fail_code;
  assert(source == F.source);
  F.frame = frame;
  F.which_seen.push_back(which);
  if (seg_index) ++F.index_asked;
  if (which < 0 || which > 3 || frame < 0 || frame > 1) return DDDMR_ERR_BAD_ARG;
  return F.answer(F.cloud[which], out, capacity, n); }
int dddmr_rollout_get_lidar_sweep_outliers(dddmr_rollout_ctx*, int32_t source, float* out, size_t capacity, size_t* n) {
  if (F.failing()) return F.fail_code;
  assert(source == F.source);
  return F.answer(F.cloud[4], out, capacity, n); }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  Cloud c[5];
  CloudInfo info;
  auto call = [&](int source, int frame) { return sweepAssociation(&ctx, source, frame, c[0], c[1], c[2], c[3], info, c[4]); };
  for (Cloud& x : c) x.points.resize(2);
  // everything empty: the orientation and one call per cloud
  assert(call(2, 0) == DDDMR_OK && F.calls == 6 && F.source == 2 && F.frame == 0);
  for (Cloud& x : c) assert(x.points.empty());
  assert(info.start_orientation == 0.25f && info.end_orientation == 6.5f && info.orientation_diff == 6.25f);
  assert((F.which_seen == std::vector<int>{0, 1, 2, 3}));
  F.cloud[0] = {1.f, 2.f, 3.f, 0.5f};
  F.cloud[1] = {1.f, 2.f, 3.f, 0.5f, 4.f, 5.f, 6.f, 1.25f};
  F.cloud[3] = {7.f, 8.f, 9.f, 15.0625f, -1.f, -2.f, -3.f, 2.f, 0.f, 0.f, 0.f, 3.f};
  F.cloud[4] = {9.f, 9.f, 9.f, 12.004f};
  F.calls = 0;
  F.which_seen.clear();
  F.orient[0] = -2.f;
  assert(call(3, 1) == DDDMR_OK && F.calls == 1 + 2 + 2 + 1 + 2 + 2 && F.source == 3 && F.frame == 1 && F.index_asked == 0);
  assert((F.which_seen == std::vector<int>{0, 0, 1, 1, 2, 3, 3}));
  assert(c[0].points.size() == 1 && c[1].points.size() == 2 && c[2].points.empty() && c[3].points.size() == 3 && c[4].points.size() == 1);
  assert(c[1].points[1].x == 4.f && c[1].points[1].y == 5.f && c[1].points[1].z == 6.f && c[1].points[1].intensity == 1.25f);
  assert(c[3].points[0].intensity == 15.0625f && c[3].points[1].z == -3.f && c[4].points[0].intensity == 12.004f);
  assert(info.start_orientation == -2.f);
  // whichever call fails, its code comes back and every output is what it was
  F.orient[0] = 1.f;
  F.cloud[0].clear();
  for (int at = 0; at < 9; ++at) {
    for (int code : {DDDMR_ERR_STATE, DDDMR_ERR_HIP}) {
      F.calls = 0; F.fail_at = at; F.fail_code = code;
      assert(call(3, 1) == code);
      assert(c[0].points.size() == 1 && c[1].points.size() == 2 && c[3].points.size() == 3 && c[4].points.size() == 1);
      assert(info.start_orientation == -2.f);
    }
  }
  F.fail_at = -1;
  // a cloud that grew between the two calls, and a bad frame
  F.calls = 0; F.grow = 2;
  assert(call(3, 1) == DDDMR_ERR_CAPACITY && c[1].points.size() == 2 && info.start_orientation == -2.f);
  assert(call(3, 2) == DDDMR_ERR_BAD_ARG && c[3].points.size() == 3);
  assert(call(3, 1) == DDDMR_OK && c[0].points.empty() && info.start_orientation == 1.f && c[1].points.size() == 4);
  const int calls = F.calls;
  assert(sweepAssociation(static_cast<dddmr_rollout_ctx*>(nullptr), 1, 0, c[0], c[1], c[2], c[3], info, c[4]) == DDDMR_ERR_BAD_ARG && F.calls == calls);
  std::printf("sweep association bridge OK\n");
  return 0;
}
