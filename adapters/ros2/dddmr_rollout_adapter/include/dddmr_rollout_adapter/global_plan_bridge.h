// global_plan_bridge.h -- the global planner's side of the A* on the device graph: what a patched GlobalPlanner /
// DWA_GlobalPlanner calls instead of walking sGraph and asking get_min_dGraphValue node by node.
//
//   GlobalPlanner::getStartGoalID + A_Star_on_PreGraph::getPath   (global_planner.cpp:393-470, a_star_on_pre_graph.cpp:191-289)
//                                                                   -> makePlanIds(start_xyz, goal_xyz)
//   DWA_GlobalPlanner::determineDWAPlan's look-ahead loop          (dynamic_window_aware_global_planner.cpp:209-273)
//                                                                   -> dwaGoalPivot(path, from, look_ahead), one probe call
//   GlobalPlanner::getStartGoalID + A_Star_on_Graph::getPath      (a_star_on_pc.cpp:200-329, use_pre_graph: false, the default)
//                                                                   -> planOnCloud(start, goal), setLethalCloud(host layers' lethal cloud)
//   GlobalPlanner::getROSPath                                      (global_planner.cpp:313-391)
//                                                                   -> pathPoses(ids, ground): rows x y z qx qy qz qw
//
// This header includes neither PCL, ROS nor tf2, so it is compiled and run in a plain C++ toolchain
// (tests/cpp/global_plan_bridge_test.cpp).  The rows of pathPoses are what dddmr_rollout_set_prune_plan's caller prunes.
#ifndef DDDMR_ROLLOUT_ADAPTER_GLOBAL_PLAN_BRIDGE_H_
#define DDDMR_ROLLOUT_ADAPTER_GLOBAL_PLAN_BRIDGE_H_

#include <array>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "dddmr_rollout.h"

namespace dddmr_rollout_adapter
{

class GlobalPlanBridge
{
public:
  typedef std::array<double, 7> Pose;                    // x y z qx qy qz qw
  typedef std::array<float, 3> Point;

  // max_nodes: the static layer's max_ground_points (the longest path there can be)
  int create(dddmr_rollout_ctx * ctx, const dddmr_global_plan_config & cfg, size_t max_nodes)
  {
    ctx_ = nullptr;
    if (!ctx) {return DDDMR_ERR_BAD_ARG;}
    const int rc = dddmr_rollout_global_plan_create(ctx, &cfg);
    if (rc != DDDMR_OK) {return rc;}
    ctx_ = ctx;                      // only after a successful create
    max_nodes_ = max_nodes;
    return DDDMR_OK;
  }
  bool created() const {return ctx_ != nullptr;}

  // pc_original_z_up_'s intensity (a_star_on_pre_graph.cpp:246), after every regeneration of the static layer
  int setNodeWeights(const std::vector<float> & w)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    return dddmr_rollout_global_plan_set_node_weights(ctx_, w.empty() ? nullptr : w.data(), w.size());
  }

  // getStartGoalID, then getPath: ids from start to goal; empty with DDDMR_OK where the reference's path stays empty (no
  // ground node within 0.5 m of an end, or no path).  result, when given, says which (status; UINT32_MAX ids in path_offset
  // are not used: start_id / goal_id tell a missing end).
  int makePlanIds(const Point & start_xyz, const Point & goal_xyz, std::vector<uint32_t> & ids, dddmr_global_plan_result * result = nullptr,
                  uint32_t * start_id = nullptr, uint32_t * goal_id = nullptr)
  {
    ids.clear();
    if (!ctx_) {return DDDMR_ERR_STATE;}
    const float xyz[6] = {start_xyz[0], start_xyz[1], start_xyz[2], goal_xyz[0], goal_xyz[1], goal_xyz[2]};
    uint32_t ends[2] = {UINT32_MAX, UINT32_MAX};
    int rc = dddmr_rollout_global_plan_nearest(ctx_, xyz, 2, ends);
    if (start_id) {*start_id = ends[0];}
    if (goal_id) {*goal_id = ends[1];}
    dddmr_global_plan_result r = dddmr_global_plan_result();
    r.status = DDDMR_GLOBAL_PLAN_NO_PATH;
    if (result) {*result = r;}
    if (rc != DDDMR_OK) {return rc;}
    if (ends[0] == UINT32_MAX || ends[1] == UINT32_MAX) {return DDDMR_OK;}       // :408, :452  "Goal / Start is not found."
    std::vector<uint32_t> path(max_nodes_ ? max_nodes_ : 1);
    rc = dddmr_rollout_global_plan_plan(ctx_, &ends[0], &ends[1], 1, path.data(), path.size(), &r);
    if (result) {*result = r;}
    if (rc != DDDMR_OK) {return rc;}
    ids.assign(path.begin() + r.path_offset, path.begin() + r.path_offset + r.path_len);
    return DDDMR_OK;
  }

  // ---- use_pre_graph: false (global_planner.cpp:100, the default): A_Star_on_Graph::getPath, a_star_on_pc.cpp:200-329 ----
  // sGraph_ptr_->getNodeWeight of every ground node (a_star_on_pc.cpp:287), after every regeneration of the static layer
  template<class Weights>
  int setGraphNodeWeights(const Weights & w)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    return dddmr_rollout_global_plan_set_graph_node_weights(ctx_, w.empty() ? nullptr : w.data(), w.size());
  }

  // The lethal clouds of the plugins that stay on the host (the no-entry layer, a host-side plugin), appended as
  // aggregateLethal appends them (stacked_perception.cpp:142-155); the device layers' lethal nodes are read where they are.
  // lethal: anything with .points of records that begin with float x, y, z (a pcl::PointCloud); an empty one clears.
  template<class Cloud>
  int setLethalCloud(const Cloud & lethal)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    if (lethal.points.empty()) {return dddmr_rollout_global_plan_set_lethal_points(ctx_, nullptr, 0, 12);}
    typedef typename std::remove_reference<decltype(lethal.points[0])>::type PointT;
    static_assert(sizeof(PointT) >= 12 && sizeof(PointT) % 4 == 0, "records of floats, x y z first");
    return dddmr_rollout_global_plan_set_lethal_points(ctx_, &lethal.points[0].x, lethal.points.size(), sizeof(PointT));
  }

  // getStartGoalID, then A_Star_on_Graph::getPath: makePlanIds with the default search.  PointT: anything with .x .y .z.
  template<class PointT>
  int planOnCloud(const PointT & start, const PointT & goal, std::vector<uint32_t> & ids, dddmr_global_plan_cloud_result * result = nullptr,
                  uint32_t * start_id = nullptr, uint32_t * goal_id = nullptr)
  {
    ids.clear();
    if (!ctx_) {return DDDMR_ERR_STATE;}
    const float xyz[6] = {(float)start.x, (float)start.y, (float)start.z, (float)goal.x, (float)goal.y, (float)goal.z};
    uint32_t ends[2] = {UINT32_MAX, UINT32_MAX};
    int rc = dddmr_rollout_global_plan_nearest(ctx_, xyz, 2, ends);
    if (start_id) {*start_id = ends[0];}
    if (goal_id) {*goal_id = ends[1];}
    dddmr_global_plan_cloud_result r = dddmr_global_plan_cloud_result();
    r.plan.status = DDDMR_GLOBAL_PLAN_NO_PATH;
    if (result) {*result = r;}
    if (rc != DDDMR_OK) {return rc;}
    if (ends[0] == UINT32_MAX || ends[1] == UINT32_MAX) {return DDDMR_OK;}       // global_planner.cpp:408, :452
    std::vector<uint32_t> path(max_nodes_ ? max_nodes_ : 1);
    rc = dddmr_rollout_global_plan_plan_on_cloud(ctx_, &ends[0], &ends[1], 1, path.data(), path.size(), &r);
    if (result) {*result = r;}
    if (rc != DDDMR_OK) {return rc;}
    ids.assign(path.begin() + r.plan.path_offset, path.begin() + r.plan.path_offset + r.plan.path_len);
    return DDDMR_OK;
  }

  // determineDWAPlan's loop (:209-273) over pcl_global_path_ from the pose nearest to the robot (`from`): the index of the
  // DWA goal.  The goal test of every pose behind `from` is asked in one probe call; the loop then runs on its answers.
  int dwaGoalPivot(const std::vector<Point> & path, size_t from, double look_ahead_distance, size_t * dwa_pivot)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    if (!dwa_pivot || path.empty() || from >= path.size()) {return DDDMR_ERR_BAD_ARG;}
    const size_t n = path.size() - from;
    std::vector<float> xyz(3 * n);
    for (size_t i = 0; i < n; ++i) {
      for (int a = 0; a < 3; ++a) {xyz[3 * i + a] = path[from + i][a];}
    }
    std::vector<uint32_t> near(n);
    std::vector<uint8_t> blocked(n);
    const int rc = dddmr_rollout_global_plan_probe(ctx_, xyz.data(), n, near.data(), blocked.data());
    if (rc != DDDMR_OK) {return rc;}
    *dwa_pivot = pivotFromProbe(path, from, look_ahead_distance, near, blocked);
    return DDDMR_OK;
  }

  // the loop itself, on probe answers for path[from ..] (near[i], blocked[i] belong to path[from + i])
  static size_t pivotFromProbe(const std::vector<Point> & path, size_t from, double look_ahead_distance, const std::vector<uint32_t> & near,
                               const std::vector<uint8_t> & blocked)
  {
    bool dwa_goal_clear = false;
    double look_ahead_step = 0.0;
    size_t dwa_pivot = 0;
    while (!dwa_goal_clear) {
      double accumulative_distance = 0.0;
      size_t pivot = from;
      Point last_point = path[pivot];
      while (accumulative_distance < look_ahead_distance + look_ahead_step && pivot < path.size() - 1) {       // :217
        const Point current_point = path[pivot];
        const double dx = current_point[0] - last_point[0], dy = current_point[1] - last_point[1], dz = current_point[2] - last_point[2];
        accumulative_distance += std::sqrt(dx * dx + dy * dy + dz * dz);
        last_point = current_point;
        pivot++;
      }
      if (pivot >= path.size() - 1) {return path.size() - 1;}                                                  // :227
      if (look_ahead_distance + look_ahead_step > 100.0) {return path.size() - 1;}                              // :236
      if (near[pivot - from] == 0 || blocked[pivot - from]) {                                                  // :251, :261
        look_ahead_step += 1.0;
        dwa_goal_clear = false;
      } else {
        dwa_goal_clear = true;
      }
      dwa_pivot = pivot;
    }
    return dwa_pivot;
  }

  // getROSPath (:313-391) in plain doubles.  ground: anything with .points[i].x / .y / .z (pcl_ground_).
  template<class Cloud>
  static std::vector<Pose> pathPoses(const std::vector<uint32_t> & ids, const Cloud & ground)
  {
    std::vector<Pose> out;
    for (size_t it = 0; it < ids.size(); ++it) {
      const double px = ground.points[ids[it]].x, py = ground.points[ids[it]].y, pz = ground.points[ids[it]].z;
      double nx = 0.0, ny = 0.0, nz = 0.0;                                     // :326  a default-constructed next_pst behind the last node
      if (it + 1 < ids.size()) {
        nx = ground.points[ids[it + 1]].x; ny = ground.points[ids[it + 1]].y; nz = ground.points[ids[it + 1]].z;
      }
      const double vx = nx - px, vy = ny - py, vz = nz - pz;
      Pose pst = {{px, py, pz, 0.0, 0.0, 0.0, 1.0}};
      if (vz != 0) {
        // :340-348  tf2::Quaternion(axis x up, -acos(axis . up)) with up = (1, 0, 0); `right_vector.normalized()` discards its
        // result, and the constructor divides by the axis' length itself
        const double unit = std::sqrt(vx * vx + vy * vy + vz * vz);
        const double ax = vx / unit, ay = vy / unit, az = vz / unit;
        const double rx = ay * 0.0 - az * 0.0, ry = az * 1.0 - ax * 0.0, rz = ax * 0.0 - ay * 1.0;
        const double angle = -1.0 * std::acos(ax * 1.0 + ay * 0.0 + az * 0.0);
        const double d = std::sqrt(rx * rx + ry * ry + rz * rz);
        const double s = std::sin(angle * 0.5) / d;
        double q[4] = {rx * s, ry * s, rz * s, std::cos(angle * 0.5)};
        const double len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int a = 0; a < 4; ++a) {pst[3 + a] = q[a] / len;}
      } else {
        const double half = std::atan2(vy, vx) * 0.5;                          // :356-358  setRPY(0, 0, yaw)
        pst[5] = std::sin(half);
        pst[6] = std::cos(half);
      }
      out.push_back(pst);
      if (it + 1 < ids.size()) {                                                // :368-385
        Pose last_pst = pst, inter = pst;
        for (double step = 0.05; step < 0.99; step += 0.05) {
          inter[0] = pst[0] + vx * step; inter[1] = pst[1] + vy * step; inter[2] = pst[2] + vz * step;
          const double dx = inter[0] - last_pst[0], dy = inter[1] - last_pst[1], dz = inter[2] - last_pst[2];
          if (std::sqrt(dx * dx + dy * dy + dz * dz) > 0.1) {
            out.push_back(inter);
            last_pst = inter;
          }
        }
      }
    }
    return out;
  }

private:
  dddmr_rollout_ctx * ctx_ = nullptr;
  size_t max_nodes_ = 0;
};

}  // namespace dddmr_rollout_adapter
#endif
