// feedDepthImage() of perception_bridge.h WITHOUT ROS or a GPU: instantiated with a stand-in transform type against a
// fake C-ABI that records the call.  Checked: the image pointer and the message's step passed through as the row stride,
// both transforms in x y z qx qy qz qw order, source id and stamp, the four counts handed back, a successful feed noted
// for the planner and a failing one reported, not swallowed and not noted (the caller falls back to its CPU path), a
// null image / context.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct V3 { double x = 0, y = 0, z = 0; };
struct Q4 { double x = 0, y = 0, z = 0, w = 1; };
struct TransformStamped { struct { V3 translation; Q4 rotation; } transform; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int rc = DDDMR_OK, calls = 0, source = -1;
  size_t stride = 0;
  const uint16_t* img = nullptr;
  double b2o[7], g2b[7];
  int64_t stamp = 0;
} F;
extern "C" {
int dddmr_rollout_set_depth_image(dddmr_rollout_ctx*, int32_t source, const uint16_t* depth_mm, size_t row_stride_bytes,
                                  const double b2o[7], const double g2b[7], int64_t stamp_ns, uint32_t* n_cam, uint32_t* n_frame,
                                  uint32_t* n_src, uint32_t* n_all) {
  ++F.calls; F.source = source; F.img = depth_mm; F.stride = row_stride_bytes; F.stamp = stamp_ns;
  std::memcpy(F.b2o, b2o, sizeof(F.b2o)); std::memcpy(F.g2b, g2b, sizeof(F.g2b));
  if (F.rc != DDDMR_OK) return F.rc;
  if (n_cam) *n_cam = 5;
  if (n_frame) *n_frame = 11;
  if (n_src) *n_src = 23;
  if (n_all) *n_all = 47;
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  TransformStamped b2o, g2b;
  b2o.transform.translation.x = 0.25; b2o.transform.translation.z = 0.5;
  b2o.transform.rotation.x = -0.5; b2o.transform.rotation.y = 0.5; b2o.transform.rotation.z = -0.5; b2o.transform.rotation.w = 0.5;
  g2b.transform.translation.x = 2.0; g2b.transform.translation.y = -1.0; g2b.transform.rotation.z = 0.6; g2b.transform.rotation.w = 0.8;
  const uint32_t width = 160, height = 120, step = 2 * 160 + 64;          // a padded sensor_msgs::msg::Image
  std::vector<uint8_t> data((size_t)step * height, 0);
  (void)SharedContext::consumeDeviceFeed();
  uint32_t n_cam = 0, n_frame = 0, n_src = 0, n_all = 0;
  const int64_t stamp = 1700000000123456789ll;
  assert(feedDepthImage(&ctx, 2, data.data(), width, height, step, b2o, g2b, stamp, &n_cam, &n_frame, &n_src, &n_all) == DDDMR_OK);
  assert(F.calls == 1 && F.source == 2 && F.stride == step && F.stamp == stamp);
  assert(reinterpret_cast<const uint8_t*>(F.img) == data.data());
  const double want_b2o[7] = {0.25, 0, 0.5, -0.5, 0.5, -0.5, 0.5}, want_g2b[7] = {2.0, -1.0, 0, 0, 0, 0.6, 0.8};
  assert(std::memcmp(F.b2o, want_b2o, sizeof(want_b2o)) == 0 && std::memcmp(F.g2b, want_g2b, sizeof(want_g2b)) == 0);
  assert(n_cam == 5 && n_frame == 11 && n_src == 23 && n_all == 47);
  assert(SharedContext::consumeDeviceFeed());            // the planner must not upload a CPU aggregate over it
  // the counts are optional
  assert(feedDepthImage(&ctx, 1, data.data(), width, height, step, b2o, g2b, stamp + 1) == DDDMR_OK && F.calls == 2 && F.source == 1);
  assert(SharedContext::consumeDeviceFeed());
  // a refused image is reported with the library's code, is no device feed, and leaves the outputs alone
  for (int code : {DDDMR_ERR_CAPACITY, DDDMR_ERR_BAD_ARG, DDDMR_ERR_HIP}) {
    F.rc = code;
    n_frame = 99;
    assert(feedDepthImage(&ctx, 2, data.data(), width, height, step, b2o, g2b, stamp, nullptr, &n_frame) == code && n_frame == 99);
    assert(!SharedContext::consumeDeviceFeed());
  }
  assert(F.calls == 5);
  F.rc = DDDMR_OK;
  // no image, no context: nothing is called
  assert(feedDepthImage(&ctx, 2, static_cast<const uint8_t*>(nullptr), width, height, step, b2o, g2b, stamp) == DDDMR_ERR_BAD_ARG);
  assert(feedDepthImage(static_cast<dddmr_rollout_ctx*>(nullptr), 2, data.data(), width, height, step, b2o, g2b, stamp) == DDDMR_ERR_BAD_ARG);
  assert(F.calls == 5 && !SharedContext::consumeDeviceFeed());
  std::printf("depth image bridge OK\n");
  return 0;
}
