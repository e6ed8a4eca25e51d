// feedDepthFrame() of perception_bridge.h WITHOUT ROS, PCL or a GPU: instantiated with stand-in message / cloud types
// against a fake C-ABI that records the call.  Checked: the record stride and count of a pcl::PointXYZ cloud, both
// transforms in x y z qx qy qz qw order, source id and stamp passed through, the three counts handed back, a
// successful feed noted for the planner (and only a successful one), an empty frame and a null context.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct V3 { double x = 0, y = 0, z = 0; };
struct Q4 { double x = 0, y = 0, z = 0, w = 1; };
struct TransformStamped { struct { V3 translation; Q4 rotation; } transform; };
struct alignas(16) PointXYZ { float x = 0, y = 0, z = 0, pad = 1; };
template <class P> struct Cloud { typedef P PointType; std::vector<P> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int rc = DDDMR_OK, calls = 0, source = -1;
  size_t n = 0, stride = 0;
  const float* xyz = nullptr;
  double b2s[7], g2b[7];
  int64_t stamp = 0;
} F;
extern "C" {
int dddmr_rollout_set_depth_frame(dddmr_rollout_ctx*, int32_t source, const float* xyz, size_t n, size_t stride, const double b2s[7],
                                  const double g2b[7], int64_t stamp_ns, uint32_t* n_frame, uint32_t* n_src, uint32_t* n_all) {
  ++F.calls; F.source = source; F.xyz = xyz; F.n = n; F.stride = stride; F.stamp = stamp_ns;
  std::memcpy(F.b2s, b2s, sizeof(F.b2s)); std::memcpy(F.g2b, g2b, sizeof(F.g2b));
  if (F.rc != DDDMR_OK) return F.rc;
  if (n_frame) *n_frame = 11;
  if (n_src) *n_src = 23;
  if (n_all) *n_all = 47;
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  TransformStamped b2s, g2b;
  b2s.transform.translation.x = 0.25; b2s.transform.translation.z = 0.5; b2s.transform.rotation.y = 0.1; b2s.transform.rotation.w = 0.9;
  g2b.transform.translation.x = 2.0; g2b.transform.translation.y = -1.0; g2b.transform.rotation.z = 0.6; g2b.transform.rotation.w = 0.8;
  Cloud<PointXYZ> frame;
  frame.points.resize(160 * 120);
  (void)SharedContext::consumeDeviceFeed();
  uint32_t n_frame = 0, n_src = 0, n_all = 0;
  const int64_t stamp = 1700000000123456789ll;
  assert(feedDepthFrame(&ctx, 2, frame, b2s, g2b, stamp, &n_frame, &n_src, &n_all) == DDDMR_OK);
  assert(F.calls == 1 && F.source == 2 && F.n == 160u * 120u && F.stride == 16 && F.xyz == &frame.points[0].x && F.stamp == stamp);
  const double want_b2s[7] = {0.25, 0, 0.5, 0, 0.1, 0, 0.9}, want_g2b[7] = {2.0, -1.0, 0, 0, 0, 0.6, 0.8};
  assert(std::memcmp(F.b2s, want_b2s, sizeof(want_b2s)) == 0 && std::memcmp(F.g2b, want_g2b, sizeof(want_g2b)) == 0);
  assert(n_frame == 11 && n_src == 23 && n_all == 47);
  assert(SharedContext::consumeDeviceFeed());            // the planner must not upload a CPU aggregate over it
  // the counts are optional
  assert(feedDepthFrame(&ctx, 1, frame, b2s, g2b, stamp + 1) == DDDMR_OK && F.calls == 2 && F.source == 1 && F.stamp == stamp + 1);
  assert(SharedContext::consumeDeviceFeed());
  // a refused frame is reported and is no device feed
  F.rc = DDDMR_ERR_CAPACITY;
  n_frame = 99;
  assert(feedDepthFrame(&ctx, 2, frame, b2s, g2b, stamp, &n_frame) == DDDMR_ERR_CAPACITY && F.calls == 3 && n_frame == 99);
  assert(!SharedContext::consumeDeviceFeed());
  F.rc = DDDMR_OK;
  // an empty frame (every pixel without a return is still a record; a driver may also send none at all)
  Cloud<PointXYZ> none;
  assert(feedDepthFrame(&ctx, 2, none, b2s, g2b, stamp) == DDDMR_OK && F.calls == 4 && F.n == 0 && F.xyz == nullptr);
  // no context: nothing is called
  assert(feedDepthFrame(static_cast<dddmr_rollout_ctx*>(nullptr), 2, frame, b2s, g2b, stamp) == DDDMR_ERR_BAD_ARG && F.calls == 4);
  std::printf("depth bridge OK\n");
  return 0;
}
