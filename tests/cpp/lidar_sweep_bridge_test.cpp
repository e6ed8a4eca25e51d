// feedSweep() and sweepCloud() of perception_bridge.h WITHOUT ROS or a GPU: instantiated with stand-in cloud and
// transform types against a fake C-ABI that records the calls.  Checked: the first point's address and the record
// size passed through, both transforms in x y z qx qy qz qw order, source id, window and height, the three counts
// handed back, a successful feed noted for the planner and a failing one reported, not swallowed and not noted, an
// empty sweep and a null context; sweepCloud's two-call protocol, its points and labels, and a sweep that grew
// between the two calls.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct V3 { double x = 0, y = 0, z = 0; };
struct Q4 { double x = 0, y = 0, z = 0, w = 1; };
struct TransformStamped { struct { V3 translation; Q4 rotation; } transform; };
struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct Cloud { std::vector<PointXYZI> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int rc = DDDMR_OK, calls = 0, source = -1, get_calls = 0, grow = 0;
  size_t n = 0, stride = 0;
  const float* xyz = nullptr;
  double b2s[7], g2b[7], window = 0, height = 0;
  std::vector<float> cloud;                                               // what the "device" holds: x y z label
} F;
extern "C" {
int dddmr_rollout_set_lidar_sweep(dddmr_rollout_ctx*, int32_t source, const float* xyz, size_t n_points, size_t stride_bytes,
                                  const double b2s[7], const double g2b[7], double window, double height, uint32_t* n_seg,
                                  uint32_t* n_src, uint32_t* n_all) {
  ++F.calls; F.source = source; F.xyz = xyz; F.n = n_points; F.stride = stride_bytes; F.window = window; F.height = height;
  std::memcpy(F.b2s, b2s, sizeof(F.b2s)); std::memcpy(F.g2b, g2b, sizeof(F.g2b));
  if (F.rc != DDDMR_OK) return F.rc;
  if (n_seg) *n_seg = 7;
  if (n_src) *n_src = 5;
  if (n_all) *n_all = 19;
  return DDDMR_OK; }
int dddmr_rollout_get_lidar_sweep_cloud(dddmr_rollout_ctx*, int32_t source, float* out, size_t capacity, size_t* n_points) {
  ++F.get_calls; F.source = source;
  if (F.rc != DDDMR_OK) return F.rc;
  if (out && F.grow) { F.cloud.resize(F.cloud.size() + 4 * (size_t)F.grow, 1.f); F.grow = 0; }   // another sweep came in
  *n_points = F.cloud.size() / 4;
  if (!out) return DDDMR_OK;
  if (capacity < *n_points) return DDDMR_ERR_CAPACITY;
  std::memcpy(out, F.cloud.data(), F.cloud.size() * sizeof(float));
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  TransformStamped b2s, g2b;
  b2s.transform.translation.x = 0.25; b2s.transform.translation.z = 0.5; b2s.transform.rotation.z = 0.6; b2s.transform.rotation.w = 0.8;
  g2b.transform.translation.x = 2.0; g2b.transform.translation.y = -1.0; g2b.transform.rotation.z = -0.6; g2b.transform.rotation.w = 0.8;
  Cloud sweep;
  sweep.points.resize(100);
  (void)SharedContext::consumeDeviceFeed();
  uint32_t n_seg = 0, n_src = 0, n_all = 0;
  assert(feedSweep(&ctx, 1, sweep, b2s, g2b, 8.0, 1.8, &n_seg, &n_src, &n_all) == DDDMR_OK);
  assert(F.calls == 1 && F.source == 1 && F.n == 100 && F.stride == sizeof(PointXYZI) && F.window == 8.0 && F.height == 1.8);
  assert(F.xyz == &sweep.points[0].x);
  const double want_b2s[7] = {0.25, 0, 0.5, 0, 0, 0.6, 0.8}, want_g2b[7] = {2.0, -1.0, 0, 0, 0, -0.6, 0.8};
  assert(std::memcmp(F.b2s, want_b2s, sizeof(want_b2s)) == 0 && std::memcmp(F.g2b, want_g2b, sizeof(want_g2b)) == 0);
  assert(n_seg == 7 && n_src == 5 && n_all == 19);
  assert(SharedContext::consumeDeviceFeed());            // the planner must not upload a CPU aggregate over it
  // the counts are optional; an empty sweep passes no pointer
  Cloud none;
  assert(feedSweep(&ctx, 0, none, b2s, g2b, 8.0, 1.8) == DDDMR_OK && F.calls == 2 && F.source == 0 && F.n == 0 && F.xyz == nullptr);
  assert(SharedContext::consumeDeviceFeed());
  // a refused sweep is reported with the library's code, is no device feed, and leaves the outputs alone
  for (int code : {DDDMR_ERR_CAPACITY, DDDMR_ERR_BAD_ARG, DDDMR_ERR_HIP}) {
    F.rc = code;
    n_seg = 99;
    assert(feedSweep(&ctx, 1, sweep, b2s, g2b, 8.0, 1.8, &n_seg) == code && n_seg == 99);
    assert(!SharedContext::consumeDeviceFeed());
  }
  assert(F.calls == 5);
  F.rc = DDDMR_OK;
  assert(feedSweep(static_cast<dddmr_rollout_ctx*>(nullptr), 1, sweep, b2s, g2b, 8.0, 1.8) == DDDMR_ERR_BAD_ARG && F.calls == 5);

  // sweepCloud: size first, then the points; labels go to intensity
  Cloud out;
  out.points.resize(3);
  assert(sweepCloud(&ctx, 1, out) == DDDMR_OK && out.points.empty() && F.get_calls == 1);   // nothing yet: one call
  F.cloud = {1.f, 2.f, 3.f, 1.f, 4.f, 5.f, 6.f, 1.f, 7.f, 8.f, 9.f, 2.f};
  assert(sweepCloud(&ctx, 1, out) == DDDMR_OK && out.points.size() == 3 && F.get_calls == 3);
  assert(out.points[1].x == 4.f && out.points[1].y == 5.f && out.points[1].z == 6.f && out.points[1].intensity == 1.f);
  assert(out.points[2].intensity == 2.f);
  // the source's cloud grew between the two calls: the library's code comes back, the output is what it was
  F.grow = 2;
  assert(sweepCloud(&ctx, 1, out) == DDDMR_ERR_CAPACITY && out.points.size() == 3);
  F.rc = DDDMR_ERR_STATE;
  assert(sweepCloud(&ctx, 2, out) == DDDMR_ERR_STATE && out.points.size() == 3);
  assert(sweepCloud(static_cast<dddmr_rollout_ctx*>(nullptr), 1, out) == DDDMR_ERR_BAD_ARG);
  std::printf("lidar sweep bridge OK\n");
  return 0;
}
