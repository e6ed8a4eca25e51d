// depthMarkCreate() and depthMarkClusters() of perception_bridge.h WITHOUT ROS, PCL or a GPU: instantiated with stand-in
// transform / cloud types against a fake C-ABI that records the calls.  Checked: the config's fields and the clouds'
// pointers / strides, the count-only call before the sized one, the clusters unpacked in order with their points, the
// coefficients, a refusal reported with the library's code and no cluster handed out, a null context.
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
struct Cloud { std::vector<PointXYZI> points; };
struct GroundCloud { std::vector<PointXYZ> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int rc_create = DDDMR_OK, rc_count = DDDMR_OK, rc_fill = DDDMR_OK, creates = 0, counts = 0, fills = 0;
  dddmr_depth_mark_config cfg{};
  size_t n_ground = 0, ground_stride = 0, n_map = 0, map_stride = 0;
  const float* ground = nullptr;
  const float* map = nullptr;
  double g2b[7];
} F;
extern "C" {
int dddmr_rollout_depth_mark_create(dddmr_rollout_ctx*, const dddmr_depth_mark_config* cfg, const float* g, size_t ng, size_t gs,
                                    const float* m, size_t nm, size_t ms) {
  ++F.creates; F.cfg = *cfg; F.ground = g; F.n_ground = ng; F.ground_stride = gs; F.map = m; F.n_map = nm; F.map_stride = ms;
  return F.rc_create; }
int dddmr_rollout_depth_mark_clusters(dddmr_rollout_ctx*, const double g2b[7], size_t cap_c, size_t cap_p, float* cen, int32_t* vox,
                                      uint32_t* size, uint32_t* off, float* xyz, float plane[4], dddmr_depth_mark_stats* st) {
  std::memcpy(F.g2b, g2b, sizeof(F.g2b));
  std::memset(st, 0, sizeof(*st));
  st->n_accepted = 2; st->n_points = 3; st->n_clusters = 5;
  if (!cen) { ++F.counts; assert(!vox && !size && !off && !xyz && !plane && cap_c == 0 && cap_p == 0); return F.rc_count; }
  ++F.fills;
  if (F.rc_fill != DDDMR_OK) return F.rc_fill;
  assert(cap_c == 2 && cap_p == 3);
  const float c[6] = {1, 2, 3, 4, 5, 6}, p[9] = {10, 11, 12, 20, 21, 22, 30, 31, 32}, pl[4] = {0, 0, 1, -0.5f};
  const int32_t v[6] = {20, 40, 60, 80, 100, 120};
  std::memcpy(cen, c, sizeof(c)); std::memcpy(xyz, p, sizeof(p)); std::memcpy(plane, pl, sizeof(pl)); std::memcpy(vox, v, sizeof(v));
  size[0] = 9; size[1] = 4; off[0] = 0; off[1] = 2; off[2] = 3;
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  GroundCloud ground; ground.points.resize(7);
  Cloud map;
  assert(depthMarkCreate(&ctx, ground, map, 0.05, 0.1, 0.1, 1, 0.2, 1u << 16) == DDDMR_OK);
  assert(F.creates == 1 && F.n_ground == 7 && F.ground_stride == 16 && F.ground == &ground.points[0].x && F.n_map == 0 && F.map == nullptr);
  assert(F.cfg.xy_resolution == 0.05 && F.cfg.height_resolution == 0.1 && F.cfg.euclidean_cluster_extraction_tolerance == 0.1 &&
         F.cfg.euclidean_cluster_extraction_min_cluster_size == 1 && F.cfg.segmentation_ignore_ratio == 0.2 &&
         F.cfg.max_observation_points == (1u << 16) && F.cfg.reserved == 0 && F.cfg.reserved2 == 0);
  map.points.resize(3);
  F.rc_create = DDDMR_ERR_STATE;
  assert(depthMarkCreate(&ctx, ground, map, 0.05, 0.1, 0.1, 1, 0.2, 1u << 16) == DDDMR_ERR_STATE);
  assert(F.n_map == 3 && F.map_stride == 32);
  assert(depthMarkCreate(static_cast<dddmr_rollout_ctx*>(nullptr), ground, map, 0.05, 0.1, 0.1, 1, 0.2, 16) == DDDMR_ERR_BAD_ARG);

  TransformStamped g2b;
  g2b.transform.translation.x = 2.0; g2b.transform.translation.z = 0.1; g2b.transform.rotation.z = 0.6; g2b.transform.rotation.w = 0.8;
  DepthMarkClusters<Cloud> out;
  (void)SharedContext::consumeDeviceFeed();
  assert(depthMarkClusters(&ctx, g2b, out) == DDDMR_OK);
  assert(F.counts == 1 && F.fills == 1 && !SharedContext::consumeDeviceFeed());
  const double want[7] = {2.0, 0, 0.1, 0, 0, 0.6, 0.8};
  assert(std::memcmp(F.g2b, want, sizeof(want)) == 0);
  assert(out.clusters.size() == 2 && out.stats.n_clusters == 5);
  assert(out.clusters[0].cx == 1 && out.clusters[0].cz == 3 && out.clusters[1].cy == 5 && out.clusters[0].size == 9 && out.clusters[1].size == 4);
  assert(out.clusters[0].voxel[2] == 60 && out.clusters[1].voxel[0] == 80);
  assert(out.clusters[0].cloud.points.size() == 2 && out.clusters[1].cloud.points.size() == 1);
  assert(out.clusters[0].cloud.points[1].y == 21 && out.clusters[1].cloud.points[0].z == 32);
  assert(out.coefficients[2] == 1 && out.coefficients[3] == -0.5f);
  // refusals: the library's code, no cluster
  F.rc_count = DDDMR_ERR_STATE;
  assert(depthMarkClusters(&ctx, g2b, out) == DDDMR_ERR_STATE && out.clusters.empty() && F.fills == 1);
  F.rc_count = DDDMR_OK; F.rc_fill = DDDMR_ERR_CAPACITY;
  assert(depthMarkClusters(&ctx, g2b, out) == DDDMR_ERR_CAPACITY && out.clusters.empty() && F.fills == 2);
  assert(depthMarkClusters(static_cast<dddmr_rollout_ctx*>(nullptr), g2b, out) == DDDMR_ERR_BAD_ARG);
  std::printf("depth mark bridge OK\n");
  return 0;
}
