// DepthLayerBridge of perception_bridge.h WITHOUT ROS, PCL or a GPU: instantiated with stand-in transform / cloud types
// against a fake C-ABI that records the calls.  Checked: ready() only after a create that returned DDDMR_OK; the clouds'
// pointers / strides and the pose handed on; the host copies of the dGraph and the lethal flags after a pass; the lethal
// and marking clouds; create, update, a getter or reset failing -> the code reaches the caller and ready() is false, so the
// caller falls back to its CPU pass and a further clearThenMark does not reach the library.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct V3 { double x = 0, y = 0, z = 0; };
struct Q4 { double x = 0, y = 0, z = 0, w = 1; };
struct TransformStamped { struct { V3 translation; Q4 rotation; } transform; };
struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };       // 32 bytes, as PCL's
struct PointXYZ { float x, y, z, pad; };
struct Cloud { typedef PointXYZI PointType; std::vector<PointXYZI> points; void push_back(const PointXYZI& p) { points.push_back(p); } };
struct GroundCloud { std::vector<PointXYZ> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int rc_create = DDDMR_OK, rc_update = DDDMR_OK, rc_reset = DDDMR_OK, rc_dgraph = DDDMR_OK, rc_lethal = DDDMR_OK;
  int creates = 0, updates = 0, resets = 0;
  dddmr_depth_layer_config cfg{};
  size_t n_ground = 0, ground_stride = 0, n_map = 0, map_stride = 0;
  const float* ground = nullptr;
  const float* map = nullptr;
  double g2b[7];
} F;
extern "C" {
int dddmr_rollout_depth_layer_create(dddmr_rollout_ctx*, const dddmr_depth_layer_config* cfg, const float* g, size_t ng, size_t gs,
                                     const float* m, size_t nm, size_t ms) {
  ++F.creates; F.cfg = *cfg; F.ground = g; F.n_ground = ng; F.ground_stride = gs; F.map = m; F.n_map = nm; F.map_stride = ms;
  return F.rc_create; }
int dddmr_rollout_depth_layer_update(dddmr_rollout_ctx*, const double g2b[7], dddmr_depth_layer_stats* st) {
  ++F.updates;
  assert(st);
  std::memcpy(F.g2b, g2b, sizeof(F.g2b));
  std::memset(st, 0, sizeof(*st));
  st->n_accepted = 3; st->host_waits = 1;
  return F.rc_update; }
int dddmr_rollout_depth_layer_reset(dddmr_rollout_ctx*) { ++F.resets; return F.rc_reset; }
int dddmr_rollout_depth_layer_get_dgraph(dddmr_rollout_ctx*, double* out, size_t cap) {
  if (F.rc_dgraph != DDDMR_OK) return F.rc_dgraph;
  assert(cap == F.n_ground + 1);
  for (size_t i = 0; i < cap; ++i) out[i] = 0.25 * (double)i;
  return DDDMR_OK; }
int dddmr_rollout_depth_layer_get_lethal(dddmr_rollout_ctx*, uint8_t* out, size_t cap) {
  if (F.rc_lethal != DDDMR_OK) return F.rc_lethal;
  assert(cap == F.n_ground + 1);
  for (size_t i = 0; i < cap; ++i) out[i] = (i % 3 == 1) ? 1 : 0;
  return DDDMR_OK; }
int dddmr_rollout_depth_layer_get_voxels(dddmr_rollout_ctx*, int32_t*, size_t, size_t* n) { *n = 2; return DDDMR_OK; }
int dddmr_rollout_depth_layer_get_clusters(dddmr_rollout_ctx*, int32_t* vox, uint32_t* off, float* xyz, size_t cap_m, size_t cap_p,
                                           size_t* m, size_t* p) {
  *m = 2; *p = 3;
  if (!vox) { assert(!off && !xyz && cap_m == 0 && cap_p == 0); return DDDMR_OK; }
  assert(cap_m == 2 && cap_p == 3);
  const float q[9] = {10, 11, 12, 20, 21, 22, 30, 31, 32};
  const int32_t v[6] = {1, 2, 3, 4, 5, 6};
  std::memcpy(xyz, q, sizeof(q)); std::memcpy(vox, v, sizeof(v));
  off[0] = 0; off[1] = 2; off[2] = 3;
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

static dddmr_depth_layer_config config() {
  dddmr_depth_layer_config c;
  std::memset(&c, 0, sizeof(c));
  c.xy_resolution = 0.05; c.height_resolution = 0.1; c.max_obstacle_distance = 77.0; c.max_markings = 8;
  return c;
}

int main() {
  dddmr_rollout_ctx ctx{0};
  GroundCloud ground; ground.points.resize(7);
  for (size_t i = 0; i < 7; ++i) ground.points[i] = PointXYZ{(float)i, (float)(2 * i), 0.5f, 0.f};
  Cloud map;
  TransformStamped g2b;
  g2b.transform.translation.x = 1.5; g2b.transform.translation.z = -2.0; g2b.transform.rotation.z = 0.6; g2b.transform.rotation.w = 0.8;

  {  // before create, and a null context
    DepthLayerBridge b;
    assert(!b.ready() && b.clearThenMark(g2b) == DDDMR_ERR_STATE && b.reset() == DDDMR_ERR_STATE && F.updates == 0 && F.resets == 0);
    assert(b.create(nullptr, config(), ground, 7, map) == DDDMR_ERR_BAD_ARG && !b.ready() && F.creates == 0);
  }
  {  // create fails: the code reaches the caller, the bridge is not ready and does not reach the library again
    DepthLayerBridge b;
    F.rc_create = DDDMR_ERR_CAPACITY;
    assert(b.create(&ctx, config(), ground, 7, map) == DDDMR_ERR_CAPACITY && !b.ready() && F.creates == 1);
    assert(b.clearThenMark(g2b) == DDDMR_ERR_STATE && F.updates == 0);
    Cloud none;
    assert(b.markingPointCloud(none) == DDDMR_ERR_STATE && none.points.empty());
    F.rc_create = DDDMR_OK;
  }
  DepthLayerBridge b;
  assert(b.create(&ctx, config(), ground, 7, map) == DDDMR_OK && b.ready());
  assert(F.n_ground == 7 && F.ground_stride == 16 && F.ground == &ground.points[0].x && F.n_map == 0 && F.map == nullptr);
  assert(F.cfg.height_resolution == 0.1 && F.cfg.max_markings == 8);
  assert(b.dGraphValue(3) == 77.0 && b.dGraphValue(7) == 77.0 && b.dGraphValue(8) == 9999.0);
  dddmr_depth_layer_stats st;
  assert(b.clearThenMark(g2b, &st) == DDDMR_OK && b.ready() && F.updates == 1 && st.n_accepted == 3);
  assert(F.g2b[0] == 1.5 && F.g2b[2] == -2.0 && F.g2b[5] == 0.6 && F.g2b[6] == 0.8);
  assert(b.dGraphValue(4) == 1.0 && b.dGraphValue(0) == 0.0);
  Cloud lethal;
  b.lethalPointCloud(ground, lethal);
  assert(lethal.points.size() == 2 && lethal.points[0].x == 1.f && lethal.points[1].x == 4.f && lethal.points[1].y == 8.f);   // nodes 1 and 4 (7 is past the ground)
  Cloud marks;
  assert(b.markingPointCloud(marks) == DDDMR_OK && marks.points.size() == 3 && marks.points[2].z == 32.f);
  assert(b.reset() == DDDMR_OK && b.ready() && F.resets == 1 && b.dGraphValue(4) == 77.0);
  assert(b.clearThenMark(g2b) == DDDMR_OK && F.updates == 2);           // (stats may be left out)

  // update fails: visible to the caller, not ready, no further call reaches the library until a create succeeds
  F.rc_update = DDDMR_ERR_CAPACITY;
  assert(b.clearThenMark(g2b) == DDDMR_ERR_CAPACITY && !b.ready() && F.updates == 3);
  F.rc_update = DDDMR_OK;
  assert(b.clearThenMark(g2b) == DDDMR_ERR_STATE && F.updates == 3 && b.reset() == DDDMR_ERR_STATE && F.resets == 1);
  assert(b.create(&ctx, config(), ground, 7, map) == DDDMR_OK && b.ready());
  // a getter failing after a good update is a failed pass too
  F.rc_lethal = DDDMR_ERR_HIP;
  assert(b.clearThenMark(g2b) == DDDMR_ERR_HIP && !b.ready());
  F.rc_lethal = DDDMR_OK;
  assert(b.create(&ctx, config(), ground, 7, map) == DDDMR_OK && b.ready());
  F.rc_reset = DDDMR_ERR_HIP;
  assert(b.reset() == DDDMR_ERR_HIP && !b.ready());
  std::printf("depth layer bridge OK\n");
  return 0;
}
