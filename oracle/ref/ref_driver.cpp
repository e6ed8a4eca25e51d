/*
 * ref_driver.cpp -- drives the reference's own rollout units (compiled from the reference checkout by
 * `make -C oracle ref`, against the stand-ins in oracle/ref/shim/) through a C API that mirrors the oracle's
 * (oracle/oracle.h), so tests/test_reference_pin_cpu.py can hold the oracle against them bit for bit.
 *
 * TEST INFRASTRUCTURE ONLY.  Our code: it includes the reference's headers and calls its classes, and includes nothing
 * under oracle/ except the shared C structs of include/dddmr_rollout.h.
 *
 * What runs is reference code: the theories' onInitialize() (parameter defaults, cuboid parsing and order),
 * initialise() (dynamic window, speed zone, motor constraint, VelocityIterator) and nextTrajectory() /
 * generateTrajectory(); base_trajectory::Trajectory; the seven critics' onInitialize() / scoreTrajectory();
 * StackedScoringModel; ModelSharedData::updateData(); perception_3d::DynamicGraph.
 * What this file does in their place:
 *  - the parameter file: a dddmr_theory_config is written into the node's parameter map under the reference's
 *    parameter names (bench-mode extensions have no reference counterpart and are ignored);
 *  - mpc_critics_ros.cpp's loading loop (not compiled: it reads the plugin list from the node): critics are created
 *    through the pluginlib registry under their type names and handed to StackedScoringModel::addPluginByTraj in
 *    stack order;
 *  - the argmin of local_planner.cpp:447-463 (entangled with the node): RESTATED below, labelled as such.
 */
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <base_trajectory/trajectory.h>
#include <mpc_critics/stacked_scoring_model.h>
#include <perception_3d/dynamic_graph.h>
#include <trajectory_generators/trajectory_generator_theory.h>
#include <trajectory_generators/velocity_iterator.h>

#include "../../include/dddmr_rollout.h"

namespace {

using trajectory_generators::TrajectoryGeneratorTheory;

const char* theory_type(int kind) {
  switch (kind) {
    case DDDMR_THEORY_DD_SIMPLE: return "trajectory_generators::DDSimpleTrajectoryGeneratorTheory";
    case DDDMR_THEORY_OMNI_SIMPLE: return "trajectory_generators::OmniSimpleTrajectoryGeneratorTheory";
    case DDDMR_THEORY_DD_ROTATE_INPLACE: return "trajectory_generators::DDRotateInplaceTheory";
  }
  return "";
}
const char* critic_type(int kind) {
  switch (kind) {
    case DDDMR_CRITIC_COLLISION: return "mpc_critics::CollisionModel";
    case DDDMR_CRITIC_COLLISION_MIN_MAX: return "mpc_critics::CollisionMinMaxModel";
    case DDDMR_CRITIC_STICK_PATH: return "mpc_critics::StickPathModel";
    case DDDMR_CRITIC_PURE_PURSUIT: return "mpc_critics::PurePursuitModel";
    case DDDMR_CRITIC_TOWARD_GLOBAL_PLAN: return "mpc_critics::TowardGlobalPlanModel";
    case DDDMR_CRITIC_SHORTEST_ANGLE: return "mpc_critics::ShortestAngleModel";
    case DDDMR_CRITIC_TWIRLING: return "mpc_critics::TwirlingModel";
  }
  return "";
}

}  // namespace

// ref_peek.hpp / peek_*.cpp: the sample list and cursor of each theory (protected members; the theory headers have no
// include guards, so each theory's accessor lives in a translation unit of its own, as each theory does in the reference)
#include "ref_peek.hpp"

namespace {

std::vector<Eigen::Vector3f>& samples_of(int kind, TrajectoryGeneratorTheory& t) {
  switch (kind) {
    case DDDMR_THEORY_OMNI_SIMPLE: return ref_peek_samples_omni(t);
    case DDDMR_THEORY_DD_ROTATE_INPLACE: return ref_peek_samples_rotate(t);
    default: return ref_peek_samples_dd(t);
  }
}
unsigned int& cursor_of(int kind, TrajectoryGeneratorTheory& t) {
  switch (kind) {
    case DDDMR_THEORY_OMNI_SIMPLE: return ref_peek_cursor_omni(t);
    case DDDMR_THEORY_DD_ROTATE_INPLACE: return ref_peek_cursor_rotate(t);
    default: return ref_peek_cursor_dd(t);
  }
}

// The parameter file of one theory + its critic stack, under the reference's parameter names.
void write_params(rclcpp::Node& node, const dddmr_theory_config& c, const std::string& tn) {
  auto d = [&](const char* k, double v) { node.set_override(tn + "." + k, rclcpp::ParameterValue(v)); };
  d("min_vel_x", c.min_vel_x); d("max_vel_x", c.max_vel_x);
  d("min_vel_y", c.min_vel_y); d("max_vel_y", c.max_vel_y);
  d("min_vel_trans", c.min_vel_trans); d("max_vel_trans", c.max_vel_trans);
  d("min_vel_theta", c.min_vel_theta); d("max_vel_theta", c.max_vel_theta);
  d("acc_lim_x", c.acc_lim_x); d("acc_lim_y", c.acc_lim_y); d("acc_lim_theta", c.acc_lim_theta);
  d("deceleration_ratio", c.deceleration_ratio);
  node.set_override(tn + ".use_motor_constraint", rclcpp::ParameterValue(c.use_motor_constraint != 0));
  d("max_motor_shaft_rpm", c.max_motor_shaft_rpm); d("wheel_diameter", c.wheel_diameter);
  d("gear_ratio", c.gear_ratio); d("robot_radius", c.robot_radius);
  d("controller_frequency", c.controller_frequency); d("sim_time", c.sim_time);
  d("linear_x_sample", c.linear_x_sample); d("linear_y_sample", c.linear_y_sample);
  d("angular_z_sample", c.angular_z_sample);
  d("sim_granularity", c.sim_granularity); d("angular_sim_granularity", c.angular_sim_granularity);
  d("rotation_speed", c.rotation_speed);
  static const char* names[8] = {"blb", "brb", "blt", "flb", "brt", "frt", "flt", "frb"};  // dddmr_theory_config order
  for (int k = 0; k < 8; ++k)
    node.set_override(tn + ".cuboid." + names[k],
                      rclcpp::ParameterValue(std::vector<double>{c.cuboid[k][0], c.cuboid[k][1], c.cuboid[k][2]}));
}
std::string critic_name(int i) { return "critic_" + std::to_string(i); }
void write_critic_params(rclcpp::Node& node, const dddmr_critic_config& k, int i) {
  const std::string n = critic_name(i);
  node.set_override(n + ".weight", rclcpp::ParameterValue(k.weight));
  node.set_override(n + ".translation_weight", rclcpp::ParameterValue(k.translation_weight));
  node.set_override(n + ".orientation_weight", rclcpp::ParameterValue(k.orientation_weight));
}

struct Generator {
  std::shared_ptr<rclcpp::Node> node;
  std::shared_ptr<TrajectoryGeneratorTheory> theory;
  std::shared_ptr<trajectory_generators::TrajectoryGeneratorSharedData> sd;
  int kind;
  std::vector<Eigen::Vector3f> samples;

  Generator(const dddmr_theory_config& c, const dddmr_tick_input& in) : kind(c.kind) {
    const std::string tn = c.name;
    node = std::make_shared<rclcpp::Node>("local_planner");
    write_params(*node, c, tn);
    theory = pluginlib::ClassLoader<TrajectoryGeneratorTheory>("trajectory_generators",
                                                               "trajectory_generators::TrajectoryGeneratorTheory")
                 .createSharedInstance(theory_type(c.kind));
    theory->initialize(tn, node);
    sd = std::make_shared<trajectory_generators::TrajectoryGeneratorSharedData>(nullptr);
    auto& t = sd->robot_pose_.transform;
    t.translation.x = in.robot_pose[0]; t.translation.y = in.robot_pose[1]; t.translation.z = in.robot_pose[2];
    t.rotation.x = in.robot_pose[3]; t.rotation.y = in.robot_pose[4];
    t.rotation.z = in.robot_pose[5]; t.rotation.w = in.robot_pose[6];
    sd->robot_state_.twist.twist.linear.x = in.robot_twist[0];
    sd->robot_state_.twist.twist.linear.y = in.robot_twist[1];
    sd->robot_state_.twist.twist.angular.z = in.robot_twist[2];
    sd->current_allowed_max_linear_speed_ = in.allowed_max_linear_speed;
    theory->setSharedData(sd);
    theory->initialise();
    samples = samples_of(kind, *theory);
  }
  // nextTrajectory() on sample i (the cursor is set to i first): true iff generateTrajectory() was true
  bool generate(const Eigen::Vector3f& s, base_trajectory::Trajectory& traj) {
    auto& sp = samples_of(kind, *theory);
    sp.assign(1, s);
    cursor_of(kind, *theory) = 0;
    return theory->nextTrajectory(traj);
  }
};

struct Scorer {
  std::shared_ptr<rclcpp::Node> node = std::make_shared<rclcpp::Node>("local_planner");
  mpc_critics::StackedScoringModel stack{nullptr, nullptr};
  std::vector<std::shared_ptr<mpc_critics::ScoringModel>> critics;
  std::string tn;

  Scorer(const dddmr_theory_config& c, const float* cloud, size_t n_points, size_t stride_bytes, const double* plan,
         size_t n_plan, const dddmr_tick_input& in, const int32_t* order, int n_order)
      : tn(c.name) {
    for (int i = 0; i < c.n_critics; ++i) write_critic_params(*node, c.critics[i], i);
    pluginlib::ClassLoader<mpc_critics::ScoringModel> loader("mpc_critics", "mpc_critics::ScoringModel");
    for (int i = 0; i < c.n_critics; ++i) {
      auto m = loader.createSharedInstance(critic_type(c.critics[i].kind));
      m->initialize(critic_name(i), node);
      m->setSharedData(stack.getSharedDataPtr());  // what addPluginByTraj does; also for critics left out of `order`
      critics.push_back(m);
    }
    // mpc_critics_ros.cpp: addPluginByTraj in the stack's order (order == nullptr: the config's own order)
    for (int j = 0; j < (order ? n_order : c.n_critics); ++j) stack.addPluginByTraj(tn, critics[order ? order[j] : j]);
    auto sd = stack.getSharedDataPtr();
    sd->pcl_perception_ = std::make_shared<pcl::PointCloud<pcl::PointXYZI>>();
    const size_t st = stride_bytes / sizeof(float);
    for (size_t i = 0; i < n_points; ++i) {
      pcl::PointXYZI p;
      p.x = cloud[i * st + 0]; p.y = cloud[i * st + 1]; p.z = cloud[i * st + 2];
      sd->pcl_perception_->push_back(p);
    }
    for (size_t i = 0; i < n_plan; ++i) {
      geometry_msgs::msg::PoseStamped ps;
      const double* q = plan + 7 * i;
      ps.pose.position.x = q[0]; ps.pose.position.y = q[1]; ps.pose.position.z = q[2];
      ps.pose.orientation.x = q[3]; ps.pose.orientation.y = q[4]; ps.pose.orientation.z = q[5];
      ps.pose.orientation.w = q[6];
      sd->prune_plan_.poses.push_back(ps);
    }
    auto& t = sd->robot_pose_.transform;
    t.translation.x = in.robot_pose[0]; t.translation.y = in.robot_pose[1]; t.translation.z = in.robot_pose[2];
    t.rotation.x = in.robot_pose[3]; t.rotation.y = in.robot_pose[4];
    t.rotation.z = in.robot_pose[5]; t.rotation.w = in.robot_pose[6];
    sd->heading_deviation_ = in.heading_deviation;
    sd->updateData();
  }
};

}  // namespace

// Only the C API below is exported: the libraries are built with hidden visibility (oracle/Makefile), so that two
// builds loaded into one process (O0 and O2) never bind each other's C++ symbols.
#pragma GCC visibility push(default)
extern "C" {

typedef struct {
  int32_t planner_state;
  int32_t best_index;
  double best_cost;
  double vx, vy, wz;
  uint32_t n_samples;
  uint32_t n_generated;
} ref_result;

int ref_velocity_iterator(double mn, double mx, int num_samples, double* out, int capacity) {
  trajectory_generators::VelocityIterator it(mn, mx, num_samples);
  int n = 0;
  for (; !it.isFinished(); it++, ++n)
    if (n < capacity) out[n] = it.getVelocity();
  return n;
}

int ref_samples(const dddmr_theory_config* c, const dddmr_tick_input* in, float* out, int capacity) {
  Generator g(*c, *in);
  for (int i = 0; i < (int)g.samples.size() && i < capacity; ++i)
    for (int k = 0; k < 3; ++k) out[3 * i + k] = g.samples[i][k];
  return (int)g.samples.size();
}

// -> number of steps (0 if generateTrajectory() returned false); poses [S][7], cuboids [S][8][3], minmax [S][2][3]
int ref_generate(const dddmr_theory_config* c, const dddmr_tick_input* in, const float sample[3], double* poses,
                 float* cuboids, float* minmax, int capacity) {
  Generator g(*c, *in);
  Eigen::Vector3f s;
  s[0] = sample[0]; s[1] = sample[1]; s[2] = sample[2];
  base_trajectory::Trajectory traj;
  if (!g.generate(s, traj)) return 0;
  const int n = (int)traj.getPointsSize();
  for (int i = 0; i < n && i < capacity; ++i) {
    const auto p = traj.getPoint(i).pose;
    if (poses) {
      const double v[7] = {p.position.x, p.position.y, p.position.z, p.orientation.x, p.orientation.y,
                           p.orientation.z, p.orientation.w};
      std::memcpy(poses + 7 * i, v, sizeof(v));
    }
    if (cuboids) {
      const auto cub = traj.getCuboid(i);
      for (int k = 0; k < 8; ++k) {
        cuboids[24 * i + 3 * k + 0] = cub.points[k].x;
        cuboids[24 * i + 3 * k + 1] = cub.points[k].y;
        cuboids[24 * i + 3 * k + 2] = cub.points[k].z;
      }
    }
    if (minmax) {
      const auto mm = traj.getCuboidMinMax(i);
      const float v[6] = {mm.first.x, mm.first.y, mm.first.z, mm.second.x, mm.second.y, mm.second.z};
      std::memcpy(minmax + 6 * i, v, sizeof(v));
    }
  }
  return n;
}

// Samples [begin, end) of the tick are generated and scored (outputs indexed from begin).  per_critic [N][n_critics]: each critic of the config alone on
// the trajectory (in config order); stacked [N]: StackedScoringModel::scoreTrajectory with the critics in `order`
// (n_order entries, indices into the config's critics; nullptr = config order); steps [N]; generated [N].
// Not-generated samples get DDDMR_COST_NOT_GENERATED.  Returns N.
int ref_score(const dddmr_theory_config* c, const float* cloud, size_t n_points, size_t stride_bytes,
              const double* plan, size_t n_plan, const dddmr_tick_input* in, const int32_t* order, int n_order,
              uint32_t begin, uint32_t end, double* per_critic, double* stacked, int32_t* steps, uint8_t* generated,
              int capacity) {
  Generator g(*c, *in);
  Scorer sc(*c, cloud, n_points, stride_bytes, plan, n_plan, *in, order, n_order);
  const std::vector<Eigen::Vector3f> all = g.samples;
  const int b = (int)std::min<size_t>(begin, all.size()), e = (int)std::min<size_t>(end, all.size());
  for (int i = 0; i < e - b && i < capacity; ++i) {
    base_trajectory::Trajectory traj;
    const bool ok = g.generate(all[b + i], traj);
    if (generated) generated[i] = ok ? 1 : 0;
    if (steps) steps[i] = ok ? (int32_t)traj.getPointsSize() : 0;
    for (int k = 0; k < c->n_critics; ++k)
      if (per_critic) per_critic[(size_t)i * c->n_critics + k] = ok ? sc.critics[k]->scoreTrajectory(traj)
                                                                   : DDDMR_COST_NOT_GENERATED;
    if (ok) sc.stack.scoreTrajectory(sc.tn, traj);
    if (stacked) stacked[i] = ok ? traj.cost_ : DDDMR_COST_NOT_GENERATED;
  }
  return std::max(0, e - b);
}

// One control tick: generate every sample (local_planner.cpp:548-557 queues only generated trajectories), score them
// with the config's stack, and pick the winner.  costs / steps / samples_out [N].
int ref_tick(const dddmr_theory_config* c, const float* cloud, size_t n_points, size_t stride_bytes,
             const double* plan, size_t n_plan, const dddmr_tick_input* in, ref_result* out, double* costs,
             int32_t* steps, float* samples_out, int capacity) {
  Generator g(*c, *in);
  Scorer sc(*c, cloud, n_points, stride_bytes, plan, n_plan, *in, nullptr, 0);
  const std::vector<Eigen::Vector3f> all = g.samples;
  std::memset(out, 0, sizeof(*out));
  // RESTATED, not compiled: the argmin of Local_Planner::getBestTrajectory (local_planner.cpp:447-463):
  // best.cost_ = -1; minimum_cost = 9999999; scan in generation order, keep cost >= 0 && cost <= minimum_cost.
  double minimum_cost = 9999999;
  int best = -1;
  base_trajectory::Trajectory best_traj;
  for (int i = 0; i < (int)all.size(); ++i) {
    base_trajectory::Trajectory traj;
    const bool ok = g.generate(all[i], traj);
    if (ok) {
      sc.stack.scoreTrajectory(sc.tn, traj);
      ++out->n_generated;
      if (traj.cost_ >= 0 && traj.cost_ <= minimum_cost) {
        best = i;
        best_traj = traj;
        minimum_cost = traj.cost_;
      }
    }
    if (i < capacity) {
      if (costs) costs[i] = ok ? traj.cost_ : DDDMR_COST_NOT_GENERATED;
      if (steps) steps[i] = ok ? (int32_t)traj.getPointsSize() : 0;
      if (samples_out)
        for (int k = 0; k < 3; ++k) samples_out[3 * i + k] = all[i][k];
    }
  }
  out->n_samples = (uint32_t)all.size();
  out->best_index = best;
  if (best >= 0) {
    out->planner_state = DDDMR_TRAJECTORY_FOUND;
    out->best_cost = best_traj.cost_;
    out->vx = best_traj.xv_; out->vy = best_traj.yv_; out->wz = best_traj.thetav_;
  } else {
    out->planner_state = DDDMR_ALL_TRAJECTORIES_FAIL;
    out->best_cost = -1.0;
  }
  return (int)all.size();
}

// perception_3d::DynamicGraph
void* ref_dgraph_create() { return new perception_3d::DynamicGraph(); }
void ref_dgraph_destroy(void* g) { delete static_cast<perception_3d::DynamicGraph*>(g); }
void ref_dgraph_initial(void* g, size_t n, double max_obstacle_distance) {
  static_cast<perception_3d::DynamicGraph*>(g)->initial(n, max_obstacle_distance);
}
void ref_dgraph_set(void* g, unsigned int key, double d) { static_cast<perception_3d::DynamicGraph*>(g)->setValue(key, d); }
void ref_dgraph_clear_value(void* g, unsigned int key, double d) {
  static_cast<perception_3d::DynamicGraph*>(g)->clearValue(key, d);
}
void ref_dgraph_clear(void* g) { static_cast<perception_3d::DynamicGraph*>(g)->clear(); }
// -> graph size; keys / values sorted by key into the outputs (up to capacity)
size_t ref_dgraph_get(void* g, uint32_t* keys, double* values, size_t capacity) {
  auto& gr = static_cast<perception_3d::DynamicGraph*>(g)->graph_;
  std::vector<std::pair<unsigned int, double>> kv(gr.begin(), gr.end());
  std::sort(kv.begin(), kv.end());
  for (size_t i = 0; i < kv.size() && i < capacity; ++i) { keys[i] = kv[i].first; values[i] = kv[i].second; }
  return kv.size();
}

}  // extern "C"
#pragma GCC visibility pop
