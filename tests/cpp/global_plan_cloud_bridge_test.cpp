// GlobalPlanBridge's entries for the default A* (global_plan_bridge.h: planOnCloud, setLethalCloud, setGraphNodeWeights)
// WITHOUT ROS, PCL or a GPU: stand-in cloud types against a fake C-ABI that records the calls.  Checked: nothing is sent
// before a create; setLethalCloud hands the records over where they are, with PCL's stride, and clears with an empty
// cloud; planOnCloud asks nearest for both ends in one call, plans only when both have a node, passes the result through
// and cuts the path out of the buffer by offset and length.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/global_plan_bridge.h"

struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct PointXYZ { float x, y, z, pad; };                               // 16 bytes
template <class P> struct Cloud { std::vector<P> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int creates = 0, nearests = 0, plans = 0, lethals = 0, weights = 0;
  int plan_rc = DDDMR_OK;
  const float* lethal_xyz = nullptr;
  size_t lethal_n = 99, lethal_stride = 0, n_weights = 99, path_capacity = 0;
  std::vector<float> nearest_xyz;
  uint32_t ends[2] = {5, 9};
  uint32_t start = 0, goal = 0;
  std::vector<uint32_t> path{5, 6, 7, 9};
  uint32_t status = DDDMR_GLOBAL_PLAN_FOUND, offset = 0;
} F;
extern "C" {
int dddmr_rollout_global_plan_create(dddmr_rollout_ctx*, const dddmr_global_plan_config*) { ++F.creates; return DDDMR_OK; }
int dddmr_rollout_global_plan_nearest(dddmr_rollout_ctx*, const float* xyz, size_t n, uint32_t* ids) {
  ++F.nearests;
  F.nearest_xyz.assign(xyz, xyz + 3 * n);
  for (size_t i = 0; i < n; ++i) ids[i] = F.ends[i];
  return DDDMR_OK; }
int dddmr_rollout_global_plan_set_graph_node_weights(dddmr_rollout_ctx*, const float*, size_t n) { ++F.weights; F.n_weights = n; return DDDMR_OK; }
int dddmr_rollout_global_plan_set_lethal_points(dddmr_rollout_ctx*, const float* xyz, size_t n, size_t stride) {
  ++F.lethals; F.lethal_xyz = xyz; F.lethal_n = n; F.lethal_stride = stride;
  return DDDMR_OK; }
int dddmr_rollout_global_plan_plan_on_cloud(dddmr_rollout_ctx*, const uint32_t* start, const uint32_t* goal, size_t nq, uint32_t* path_out, size_t cap,
                                            dddmr_global_plan_cloud_result* res) {
  ++F.plans;
  assert(nq == 1);
  F.start = start[0]; F.goal = goal[0]; F.path_capacity = cap;
  std::memset(res, 0, sizeof(*res));
  res->plan.status = F.status;
  res->n_los_tested = 31; res->n_los_blocked = 4; res->max_successors = 13;
  if (F.status == DDDMR_GLOBAL_PLAN_FOUND) {
    assert(cap >= F.offset + F.path.size());
    std::memcpy(path_out + F.offset, F.path.data(), F.path.size() * 4);
    res->plan.path_offset = F.offset;
    res->plan.path_len = (uint32_t)F.path.size();
  }
  return F.plan_rc; }
}

int main() {
  using dddmr_rollout_adapter::GlobalPlanBridge;
  static_assert(sizeof(dddmr_global_plan_cloud_result) == 56, "the size the library and the ctypes mirror pin");
  dddmr_rollout_ctx ctx{0};
  GlobalPlanBridge b;
  std::vector<uint32_t> ids{1, 2};
  Cloud<PointXYZI> lethal;
  lethal.points.resize(3);
  lethal.points[1].x = 2.5f;
  const PointXYZ s{0.5f, 1.5f, 0.25f, 0.f}, g{3.f, 4.f, 0.f, 0.f};
  // nothing before a create
  assert(b.planOnCloud(s, g, ids) == DDDMR_ERR_STATE && ids.empty());
  assert(b.setLethalCloud(lethal) == DDDMR_ERR_STATE && b.setGraphNodeWeights(std::vector<float>{1.f}) == DDDMR_ERR_STATE);
  assert(F.creates + F.nearests + F.plans + F.lethals + F.weights == 0);
  dddmr_global_plan_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.max_queries = 1; cfg.max_open_entries = 1000; cfg.max_expansions = 100; cfg.inscribed_radius = 0.15;
  assert(b.create(&ctx, cfg, 64) == DDDMR_OK);

  // the lethal cloud: the records where they are, PCL's stride; an empty cloud clears
  assert(b.setLethalCloud(lethal) == DDDMR_OK && F.lethals == 1 && F.lethal_n == 3 && F.lethal_stride == 32 && F.lethal_xyz == &lethal.points[0].x);
  assert(F.lethal_xyz[8] == 2.5f);                                              // (the second record, 32 bytes on)
  Cloud<PointXYZ> none;
  assert(b.setLethalCloud(none) == DDDMR_OK && F.lethals == 2 && F.lethal_n == 0 && F.lethal_xyz == nullptr);
  assert(b.setGraphNodeWeights(std::vector<float>{0.1f, 0.2f, 0.3f}) == DDDMR_OK && F.n_weights == 3);
  assert(b.setGraphNodeWeights(std::vector<float>()) == DDDMR_OK && F.n_weights == 0 && F.weights == 2);

  // a plan: one nearest call for both ends, the result passed through, the path cut out by offset and length
  dddmr_global_plan_cloud_result res;
  uint32_t sid = 0, gid = 0;
  F.offset = 3;
  assert(b.planOnCloud(s, g, ids, &res, &sid, &gid) == DDDMR_OK);
  assert(F.nearests == 1 && F.plans == 1 && F.nearest_xyz.size() == 6 && F.nearest_xyz[1] == 1.5f && F.nearest_xyz[3] == 3.f);
  assert(sid == 5 && gid == 9 && F.start == 5 && F.goal == 9 && F.path_capacity == 64);
  assert((ids == std::vector<uint32_t>{5, 6, 7, 9}) && res.plan.status == DDDMR_GLOBAL_PLAN_FOUND && res.n_los_tested == 31 && res.max_successors == 13);
  // an end without a ground node: no plan call, an empty path, DDDMR_OK ("Goal is not found.")
  F.ends[1] = UINT32_MAX;
  assert(b.planOnCloud(s, g, ids, &res, &sid, &gid) == DDDMR_OK && ids.empty() && F.plans == 1 && gid == UINT32_MAX);
  assert(res.plan.status == DDDMR_GLOBAL_PLAN_NO_PATH);
  F.ends[1] = 9;
  // no path, and a refused call: the status and the error come through, the path stays empty
  F.status = DDDMR_GLOBAL_PLAN_NO_PATH;
  assert(b.planOnCloud(s, g, ids, &res) == DDDMR_OK && ids.empty() && res.plan.status == DDDMR_GLOBAL_PLAN_NO_PATH && F.plans == 2);
  F.status = DDDMR_GLOBAL_PLAN_ROW_FULL;
  F.plan_rc = DDDMR_ERR_CAPACITY;
  assert(b.planOnCloud(s, g, ids, &res) == DDDMR_ERR_CAPACITY && ids.empty() && res.plan.status == DDDMR_GLOBAL_PLAN_ROW_FULL);
  // without a result pointer
  F.status = DDDMR_GLOBAL_PLAN_FOUND; F.plan_rc = DDDMR_OK; F.offset = 0;
  assert(b.planOnCloud(s, g, ids) == DDDMR_OK && ids.size() == 4);
  std::printf("global plan cloud bridge OK\n");
  return 0;
}
