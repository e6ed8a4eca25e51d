// GlobalPlanBridge (global_plan_bridge.h) WITHOUT ROS, PCL, tf2 or a GPU: stand-in cloud types against a fake C-ABI that
// records the calls.  Checked: nothing is sent before a create; makePlanIds asks nearest for both ends in one call, plans
// only when both have a node, and cuts the path out of the buffer by offset and length; dwaGoalPivot makes one probe call
// for the poses behind `from` and walks the reference's loop on a scripted answer (a blocked goal and a goal without
// ground each push the look-ahead by a metre; the path's end and the 100 m limit end the loop); pathPoses against
// hand-computed rows: a level segment, a climbing one, the interpolation's spacing and a one-node path.
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/global_plan_bridge.h"

struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct Cloud { std::vector<PointXYZI> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int create_rc = DDDMR_OK, plan_rc = DDDMR_OK;
  int creates = 0, weights = 0, nearests = 0, probes = 0, plans = 0;
  dddmr_global_plan_config cfg;
  std::vector<float> nearest_xyz, probe_xyz;
  uint32_t ends[2] = {5, 9};
  uint32_t start = 0, goal = 0;
  size_t n_weights = 0, path_capacity = 0;
  std::vector<uint32_t> near;
  std::vector<uint8_t> blocked;
  std::vector<uint32_t> path{5, 6, 7, 9};
  uint32_t status = DDDMR_GLOBAL_PLAN_FOUND;
} F;
extern "C" {
int dddmr_rollout_global_plan_create(dddmr_rollout_ctx*, const dddmr_global_plan_config* cfg) { ++F.creates; F.cfg = *cfg; return F.create_rc; }
int dddmr_rollout_global_plan_set_node_weights(dddmr_rollout_ctx*, const float*, size_t n) { ++F.weights; F.n_weights = n; return DDDMR_OK; }
int dddmr_rollout_global_plan_nearest(dddmr_rollout_ctx*, const float* xyz, size_t n, uint32_t* ids) {
  ++F.nearests;
  F.nearest_xyz.assign(xyz, xyz + 3 * n);
  for (size_t i = 0; i < n; ++i) ids[i] = F.ends[i];
  return DDDMR_OK; }
int dddmr_rollout_global_plan_probe(dddmr_rollout_ctx*, const float* xyz, size_t n, uint32_t* near, uint8_t* blocked) {
  ++F.probes;
  F.probe_xyz.assign(xyz, xyz + 3 * n);
  assert(F.near.size() >= n);
  for (size_t i = 0; i < n; ++i) { near[i] = F.near[i]; blocked[i] = F.blocked[i]; }
  return DDDMR_OK; }
int dddmr_rollout_global_plan_plan(dddmr_rollout_ctx*, const uint32_t* start, const uint32_t* goal, size_t nq, uint32_t* path_out, size_t cap,
                                   dddmr_global_plan_result* res) {
  ++F.plans;
  assert(nq == 1);
  F.start = start[0]; F.goal = goal[0]; F.path_capacity = cap;
  std::memset(res, 0, sizeof(*res));
  res->status = F.status;
  if (F.status == DDDMR_GLOBAL_PLAN_FOUND) {
    assert(cap >= F.path.size());
    std::memcpy(path_out, F.path.data(), F.path.size() * 4);
    res->path_len = (uint32_t)F.path.size();
  }
  return F.plan_rc; }
}

static bool close_to(double a, double b) { return std::fabs(a - b) <= 1e-12; }

int main() {
  using dddmr_rollout_adapter::GlobalPlanBridge;
  dddmr_rollout_ctx ctx{0};
  GlobalPlanBridge b;
  std::vector<uint32_t> ids;
  size_t pivot = 99;
  // nothing before a create
  assert(b.makePlanIds({{0, 0, 0}}, {{1, 1, 0}}, ids) == DDDMR_ERR_STATE && b.setNodeWeights({1.f}) == DDDMR_ERR_STATE);
  assert(b.dwaGoalPivot({{{0, 0, 0}}}, 0, 2.0, &pivot) == DDDMR_ERR_STATE);
  assert(F.creates + F.nearests + F.probes + F.plans + F.weights == 0);
  dddmr_global_plan_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.turning_weight = 0.1; cfg.max_queries = 1; cfg.max_open_entries = 1000; cfg.max_expansions = 100;
  F.create_rc = DDDMR_ERR_STATE;
  assert(b.create(&ctx, cfg, 64) == DDDMR_ERR_STATE && !b.created());
  F.create_rc = DDDMR_OK;
  assert(b.create(&ctx, cfg, 64) == DDDMR_OK && b.created() && F.cfg.turning_weight == 0.1);
  assert(b.setNodeWeights({0.1f, 0.2f}) == DDDMR_OK && F.n_weights == 2);

  // makePlanIds: one nearest call with both ends, one plan
  dddmr_global_plan_result res;
  uint32_t s = 0, g = 0;
  assert(b.makePlanIds({{1.f, 2.f, 3.f}}, {{4.f, 5.f, 6.f}}, ids, &res, &s, &g) == DDDMR_OK);
  assert(F.nearests == 1 && F.plans == 1 && F.nearest_xyz == (std::vector<float>{1, 2, 3, 4, 5, 6}));
  assert(F.start == 5 && F.goal == 9 && s == 5 && g == 9 && F.path_capacity == 64 && ids == F.path && res.status == DDDMR_GLOBAL_PLAN_FOUND);
  // an end without a ground node: no plan call, an empty path
  F.ends[1] = UINT32_MAX;
  assert(b.makePlanIds({{1.f, 2.f, 3.f}}, {{4.f, 5.f, 6.f}}, ids, &res, &s, &g) == DDDMR_OK && ids.empty() && F.plans == 1 && g == UINT32_MAX);
  F.ends[1] = 9;
  F.status = DDDMR_GLOBAL_PLAN_NO_PATH;
  assert(b.makePlanIds({{1.f, 2.f, 3.f}}, {{4.f, 5.f, 6.f}}, ids, &res) == DDDMR_OK && ids.empty() && F.plans == 2 && res.status == DDDMR_GLOBAL_PLAN_NO_PATH);
  F.status = DDDMR_GLOBAL_PLAN_OPEN_FULL; F.plan_rc = DDDMR_ERR_CAPACITY;
  assert(b.makePlanIds({{1.f, 2.f, 3.f}}, {{4.f, 5.f, 6.f}}, ids, &res) == DDDMR_ERR_CAPACITY && ids.empty() && res.status == DDDMR_GLOBAL_PLAN_OPEN_FULL);

  // dwaGoalPivot: a straight path, a pose every 0.5 m, 21 poses; from = 2; look ahead 2 m
  std::vector<GlobalPlanBridge::Point> path;
  for (int i = 0; i < 21; ++i) path.push_back({{0.5f * i, 1.f, 0.f}});
  F.near.assign(19, 3);
  F.blocked.assign(19, 0);
  // the inner loop adds the distance to the previous pose before it steps: from pose 2 it stops at pivot 2 + 5 = 7
  assert(b.dwaGoalPivot(path, 2, 2.0, &pivot) == DDDMR_OK && pivot == 7 && F.probes == 1);
  assert(F.probe_xyz.size() == 3 * 19 && F.probe_xyz[0] == 1.0f && F.probe_xyz[3 * 18] == 10.0f);
  // pose 7 blocked, pose 9 without ground, pose 11 clear: one metre further each time
  F.blocked[7 - 2] = 1;
  F.near[9 - 2] = 0;
  assert(b.dwaGoalPivot(path, 2, 2.0, &pivot) == DDDMR_OK && pivot == 11 && F.probes == 2);
  // everything behind blocked: the path's end
  F.blocked.assign(19, 1);
  assert(b.dwaGoalPivot(path, 2, 2.0, &pivot) == DDDMR_OK && pivot == 20);
  // a look-ahead beyond the path's end: its end, whatever the probe says; from at the last pose
  F.blocked.assign(19, 0);
  assert(b.dwaGoalPivot(path, 2, 50.0, &pivot) == DDDMR_OK && pivot == 20);
  assert(b.dwaGoalPivot(path, 20, 2.0, &pivot) == DDDMR_OK && pivot == 20);
  assert(b.dwaGoalPivot(path, 21, 2.0, &pivot) == DDDMR_ERR_BAD_ARG);
  // the 100 m limit on a long blocked path
  std::vector<GlobalPlanBridge::Point> far;
  for (int i = 0; i < 300; ++i) far.push_back({{1.f * i, 0.f, 0.f}});
  assert(GlobalPlanBridge::pivotFromProbe(far, 0, 2.0, std::vector<uint32_t>(300, 1), std::vector<uint8_t>(300, 1)) == 299);

  // pathPoses
  Cloud ground;
  auto pt = [](float x, float y, float z) { PointXYZI p; std::memset(&p, 0, sizeof(p)); p.x = x; p.y = y; p.z = z; return p; };
  ground.points = {pt(1.f, 1.f, 0.f), pt(1.f, 2.f, 0.f), pt(2.f, 2.f, 1.f), pt(-3.f, 0.f, 0.f), pt(0.f, 4.f, 0.f)};
  // level, along +y: yaw = pi / 2 -> (0, 0, sin(pi/4), cos(pi/4)); the node, then 0.15, 0.30, ... 0.90 along the edge
  auto rows = GlobalPlanBridge::pathPoses(std::vector<uint32_t>{0, 1, 2}, ground);
  const double h = std::sqrt(0.5);
  assert(close_to(rows[0][0], 1) && close_to(rows[0][1], 1) && close_to(rows[0][2], 0));
  assert(close_to(rows[0][3], 0) && close_to(rows[0][4], 0) && close_to(rows[0][5], h) && close_to(rows[0][6], h));
  size_t second = 0;
  for (size_t i = 1; i < rows.size(); ++i) if (close_to(rows[i][0], 1) && close_to(rows[i][1], 2) && close_to(rows[i][2], 0)) second = i;
  assert(second >= 6 && second <= 9);                                        // 0.05 steps kept when more than 0.1 m apart: every third, or second
  for (size_t i = 1; i < second; ++i) {
    const double d = rows[i][1] - rows[i - 1][1];
    assert(d > 0.1 && d < 0.2 + 1e-9 && close_to(rows[i][0], 1) && close_to(rows[i][5], h));
  }
  assert(rows[second - 1][1] < 2.0 - 0.01);                                  // step < 0.99: the next node itself comes from its own turn
  // climbing along (1, 0, 1): axis = (h, 0, h), right = axis x (1, 0, 0) = (0, h, 0), angle = -acos(h) = -pi / 4
  // -> q = (0, sin(-pi / 8), 0, cos(pi / 8))
  const double pi = std::acos(-1.0);
  assert(close_to(rows[second][3], 0) && close_to(rows[second][4], std::sin(-pi / 8)) && close_to(rows[second][5], 0) && close_to(rows[second][6], std::cos(pi / 8)));
  // the last node: next_pst is the origin, v = -(2, 2, 1), vz != 0: axis = -(2, 2, 1) / 3, right = (0, az, -ay) = (0, -1/3, 2/3)
  const auto& last = rows.back();
  assert(close_to(last[0], 2) && close_to(last[1], 2) && close_to(last[2], 1));
  {
    const double angle = -std::acos(-2.0 / 3.0), d = std::sqrt(5.0) / 3.0, sn = std::sin(angle / 2) / d;
    assert(close_to(last[3], 0) && close_to(last[4], -1.0 / 3.0 * sn) && close_to(last[5], 2.0 / 3.0 * sn) && close_to(last[6], std::cos(angle / 2)));
  }
  // one node on z = 0: v = -(−3, 0, 0) = (3, 0, 0), yaw 0; one pose
  rows = GlobalPlanBridge::pathPoses(std::vector<uint32_t>{3}, ground);
  assert(rows.size() == 1 && close_to(rows[0][0], -3) && close_to(rows[0][5], 0) && close_to(rows[0][6], 1));
  rows = GlobalPlanBridge::pathPoses(std::vector<uint32_t>{4}, ground);      // v = (0, -4, 0): yaw = -pi / 2
  assert(rows.size() == 1 && close_to(rows[0][5], -h) && close_to(rows[0][6], h));
  assert(GlobalPlanBridge::pathPoses(std::vector<uint32_t>{}, ground).empty());
  std::printf("global plan bridge OK\n");
  return 0;
}
