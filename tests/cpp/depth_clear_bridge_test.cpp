// feedDepthFrustum() and depthClearVerdicts() of perception_bridge.h WITHOUT ROS, PCL or a GPU: instantiated with
// stand-in transform / cloud types against a fake C-ABI that records the calls.  Checked: m2s in x y z qx qy qz qw order,
// the camera parameters in the config's fields, no device feed noted; the markings flattened into voxel keys, offsets
// and packed cluster points in order, verdicts split into kept / branch, engagement counts handed back, a refusal
// reported with the library's code and the outputs left alone, a null cluster / context.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct V3 { double x = 0, y = 0, z = 0; };
struct Q4 { double x = 0, y = 0, z = 0, w = 1; };
struct TransformStamped { struct { V3 translation; Q4 rotation; } transform; };
struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };       // 32 bytes, as PCL's
struct Cloud { std::vector<PointXYZI> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int rc = DDDMR_OK, frustum_calls = 0, verdict_calls = 0, source = -1;
  dddmr_depth_frustum_config cfg{};
  double m2s[7];
  double res = 0, hres = 0;
  std::vector<int32_t> voxel;
  std::vector<uint32_t> offsets;
  std::vector<float> xyz;
} F;
extern "C" {
int dddmr_rollout_set_depth_frustum(dddmr_rollout_ctx*, int32_t source, const dddmr_depth_frustum_config* cfg, const double m2s[7]) {
  ++F.frustum_calls; F.source = source; F.cfg = *cfg;
  std::memcpy(F.m2s, m2s, sizeof(F.m2s));
  return F.rc; }
int dddmr_rollout_depth_clear_verdicts(dddmr_rollout_ctx*, double res, double hres, const int32_t* voxel, const uint32_t* offsets,
                                       const float* xyz, size_t m, uint8_t* verdict, uint32_t* engaged) {
  ++F.verdict_calls; F.res = res; F.hres = hres;
  F.voxel.assign(voxel, voxel + 3 * m);
  F.offsets.assign(offsets, offsets + m + 1);
  F.xyz.assign(xyz, xyz + 3 * (size_t)offsets[m]);
  if (F.rc != DDDMR_OK) return F.rc;
  const uint8_t v[3] = {(1 << 1) | 1, (2 << 1) | 0, (3 << 1) | 1};
  for (size_t i = 0; i < m; ++i) { verdict[i] = v[i % 3]; if (engaged) engaged[i] = (uint32_t)(10 * i); }
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  TransformStamped m2s;
  m2s.transform.translation.x = 2.0; m2s.transform.translation.y = -1.0; m2s.transform.translation.z = 0.35;
  m2s.transform.rotation.z = 0.6; m2s.transform.rotation.w = 0.8;
  (void)SharedContext::consumeDeviceFeed();
  assert(feedDepthFrustum(&ctx, 1, 1.5184, 1.0123, 0.3, 5.0, m2s) == DDDMR_OK);
  assert(F.frustum_calls == 1 && F.source == 1);
  assert(F.cfg.FOV_W == 1.5184 && F.cfg.FOV_V == 1.0123 && F.cfg.obstacle_min_range == 0.3 && F.cfg.obstacle_max_range == 5.0);
  const double want[7] = {2.0, -1.0, 0.35, 0, 0, 0.6, 0.8};
  assert(std::memcmp(F.m2s, want, sizeof(want)) == 0);
  assert(!SharedContext::consumeDeviceFeed());           // a frustum is no observation
  F.rc = DDDMR_ERR_STATE;
  assert(feedDepthFrustum(&ctx, 0, 1.5, 1.0, 0.3, 5.0, m2s) == DDDMR_ERR_STATE && F.frustum_calls == 2);
  F.rc = DDDMR_OK;
  assert(feedDepthFrustum(static_cast<dddmr_rollout_ctx*>(nullptr), 0, 1.5, 1.0, 0.3, 5.0, m2s) == DDDMR_ERR_BAD_ARG && F.frustum_calls == 2);

  Cloud a, b, c;
  for (int i = 0; i < 2; ++i) a.points.push_back(PointXYZI{1.0f + i, 2.0f, 3.0f, 0, 0, {0, 0, 0}});
  for (int i = 0; i < 3; ++i) c.points.push_back(PointXYZI{-1.0f, -2.0f - i, 0.5f, 0, 0, {0, 0, 0}});
  std::vector<DepthMarkingRef<Cloud>> markings = {{10, -20, 3, &a}, {11, -21, 4, &b}, {12, -22, 5, &c}};
  std::vector<uint8_t> kept, branch;
  std::vector<uint32_t> engaged;
  assert(depthClearVerdicts(&ctx, 0.05, 0.1, markings, kept, &branch, &engaged) == DDDMR_OK);
  assert(F.verdict_calls == 1 && F.res == 0.05 && F.hres == 0.1);
  assert((F.voxel == std::vector<int32_t>{10, -20, 3, 11, -21, 4, 12, -22, 5}));
  assert((F.offsets == std::vector<uint32_t>{0, 2, 2, 5}));
  assert((F.xyz == std::vector<float>{1, 2, 3, 2, 2, 3, -1, -2, 0.5f, -1, -3, 0.5f, -1, -4, 0.5f}));
  assert((kept == std::vector<uint8_t>{1, 0, 1}) && (branch == std::vector<uint8_t>{1, 2, 3}));
  assert((engaged == std::vector<uint32_t>{0, 10, 20}));
  // the optional outputs may be left out
  std::vector<uint8_t> kept2;
  assert(depthClearVerdicts(&ctx, 0.05, 0.1, markings, kept2) == DDDMR_OK && kept2 == kept);
  // a refusal is reported and writes nothing
  F.rc = DDDMR_ERR_STATE;
  std::vector<uint8_t> kept3 = {7};
  assert(depthClearVerdicts(&ctx, 0.05, 0.1, markings, kept3) == DDDMR_ERR_STATE && kept3 == std::vector<uint8_t>{7});
  F.rc = DDDMR_OK;
  const int calls = F.verdict_calls;
  markings[1].pc = nullptr;                              // the reference skips such entries before it gets here
  assert(depthClearVerdicts(&ctx, 0.05, 0.1, markings, kept3) == DDDMR_ERR_BAD_ARG && F.verdict_calls == calls);
  assert(depthClearVerdicts(static_cast<dddmr_rollout_ctx*>(nullptr), 0.05, 0.1, markings, kept3) == DDDMR_ERR_BAD_ARG);
  std::printf("depth clear bridge OK\n");
  return 0;
}
