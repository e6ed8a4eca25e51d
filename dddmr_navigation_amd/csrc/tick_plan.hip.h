// tick_plan.hip.h -- the host side of a tick that is arithmetic alone: the theory's initialise() (the dynamic-window
// sample axes of dd_simple_trajectory_generator_theory.cpp:236-295, omni_simple_...cpp:260-332,
// dd_rotate_inplace_theory.cpp:229-274), the local costmap tile's extent, and plan_tick(): every number the kernels of
// rollout_kernels.hip.h are launched with.  Host code only -- no HIP runtime call, no getenv, no context -- so that
// tests/cpp/tick_plan_test.cpp can replay recorded ticks through it on a machine without a GPU.
//
// Citations are relative to /root/reference/src/dddmr_local_planner/.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rollout_kernels.hip.h"

using namespace dddmr;

namespace {

constexpr uint32_t kCapCells = 1u << 20;
constexpr int kMaxAxis = 4096;
constexpr int kScoreLdsMax = 150 * 1024;   // dynamic LDS one k_score workgroup may use

struct Window {              // result of a theory's initialise()
  std::vector<float> ax, ay, ath;
  bool list_mode = false;
  std::vector<float4> list;  // explicit samples (rotate-in-place, motor-constraint filter)
  size_t count() const { return list_mode ? list.size() : ax.size() * ay.size() * ath.size(); }
};

// velocity_iterator.h:44-69 -- even samples in [lo,hi], max(2,n) of them, an
// extra 0.0 where the range straddles zero, last sample forced to hi.
void velocity_samples(double lo, double hi, int n, bool insert_zero, std::vector<float>& out) {
  out.clear();
  if (lo == hi) {
    out.push_back((float)lo);
    return;
  }
  n = std::max(2, n);
  const double step = (hi - lo) / double(std::max(1, n - 1));
  double next = lo;
  for (int j = 0; j < n - 1; ++j) {
    const double cur = next;
    next += step;
    out.push_back((float)cur);
    if (insert_zero && cur < 0 && next > 0) out.push_back(0.0f);
  }
  out.push_back((float)hi);
}

bool motor_rpm_ok(const dddmr_theory_config& c, float v, float w) {
  // dd_simple...cpp:297-312, dd_rotate_inplace_theory.cpp:276-286
  const double vr = v + c.robot_radius * w;
  const double vl = v - c.robot_radius * w;
  const double rpm_r = vr * c.gear_ratio * 60. / 3.1415926 / c.wheel_diameter;
  const double rpm_l = vl * c.gear_ratio * 60. / 3.1415926 / c.wheel_diameter;
  return !(std::fabs(rpm_r) >= c.max_motor_shaft_rpm || std::fabs(rpm_l) >= c.max_motor_shaft_rpm);
}

// The dynamic window is computed in float (Eigen::Vector3f max_vel/min_vel) from
// double limits, exactly like the theories' initialise().
void make_window(const dddmr_theory_config& c, const dddmr_tick_input& in, Window& w) {
  w = Window();
  if (!(c.linear_x_sample * c.angular_z_sample > 0)) {
    w.list_mode = true;  // no samples at all
    return;
  }
  const bool zero = c.bench_no_zero_insert == 0;
  const double period = 1.0 / c.controller_frequency;
  const double vx = in.robot_twist[0], vy = in.robot_twist[1], wz = in.robot_twist[2];
  const float accx = (float)c.acc_lim_x, accy = (float)c.acc_lim_y, acct = (float)c.acc_lim_theta;
  const double max_th = c.max_vel_theta, min_th = -1.0 * c.max_vel_theta;

  if (c.kind == DDDMR_THEORY_DD_ROTATE_INPLACE) {
    w.list_mode = true;
    const float sp = (float)c.rotation_speed, sn = (float)(-1.0 * c.rotation_speed);
    if (motor_rpm_ok(c, 0.f, sp)) w.list.push_back(make_float4(0.f, 0.f, sp, 0.f));
    if (motor_rpm_ok(c, 0.f, sn)) w.list.push_back(make_float4(0.f, 0.f, sn, 0.f));
    return;
  }

  float hi_x, lo_x, hi_t, lo_t;
  hi_t = (float)std::min(max_th, wz + acct * period);
  lo_t = (float)std::max(min_th, wz - acct * period);
  if (c.kind == DDDMR_THEORY_DD_SIMPLE) {
    double cap_x = c.max_vel_x;
    if (in.allowed_max_linear_speed > 0.0) cap_x = std::min(cap_x, in.allowed_max_linear_speed);
    hi_x = (float)std::min(cap_x, vx + accx * period);
    lo_x = (float)std::max(c.min_vel_x, vx / c.deceleration_ratio);
    if (hi_x < lo_x) {  // speed zone tighter than the robot can decelerate (:273-276)
      lo_x = (float)(vx / c.deceleration_ratio);
      hi_x = (float)(vx / c.deceleration_ratio);
    }
    velocity_samples(lo_x, hi_x, (int)c.linear_x_sample, zero, w.ax);
    velocity_samples(lo_t, hi_t, (int)c.angular_z_sample, zero, w.ath);
    w.ay.assign(1, 0.0f);
    if (c.use_motor_constraint) {  // filtered list keeps the x-major / theta-minor order
      w.list_mode = true;
      for (float x : w.ax)
        for (float t : w.ath)
          if (motor_rpm_ok(c, x, t)) w.list.push_back(make_float4(x, 0.f, t, 0.f));
    }
    return;
  }
  // omni (omni_simple...cpp:283-312)
  float hi_y, lo_y;
  hi_x = (float)std::min(c.max_vel_x, vx + accx * period);
  hi_y = (float)std::min(c.max_vel_y, vy + accy * period);
  lo_x = (float)std::max(c.min_vel_x, vx - accx * period);
  lo_y = (float)std::max(c.min_vel_y, vy - accy * period);
  if (vx >= c.max_vel_x / c.deceleration_ratio) lo_x = (float)std::max(c.min_vel_x, vx / c.deceleration_ratio);
  else if (vx <= c.min_vel_x / c.deceleration_ratio) hi_x = (float)std::min(c.max_vel_x, vx / c.deceleration_ratio);
  if (vy >= c.max_vel_y / c.deceleration_ratio) lo_y = (float)std::max(c.min_vel_y, vy / c.deceleration_ratio);
  else if (vy <= c.min_vel_y / c.deceleration_ratio) hi_y = (float)std::min(c.max_vel_y, vy / c.deceleration_ratio);
  velocity_samples(lo_x, hi_x, (int)c.linear_x_sample, zero, w.ax);
  velocity_samples(lo_y, hi_y, (int)c.linear_y_sample, zero, w.ay);
  velocity_samples(lo_t, hi_t, (int)c.angular_z_sample, zero, w.ath);
}

void quat_to_rot(const double p[7], double R[9]) {
  // Eigen::Quaterniond(w,x,y,z).toRotationMatrix(), as tf2::transformToEigen builds it
  const double x = p[3], y = p[4], z = p[5], w = p[6];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

float absmax(const std::vector<float>& v) {
  float m = 0.f;
  for (float x : v) m = std::max(m, std::fabs(x));
  return m;
}

// The points the collision critics look at around one pose, in the body frame: the 8 cuboid vertices (the min-max
// critic tests their bounding box) AND the 8 corners of the region CollisionModel tests, { d : |d . a_i| <= h_i } around
// the mean of the vertices with a_i, h_i from the edges e_i = v_i - v_0 (collision_model.cpp:85-115).  For a cuboid
// that is a body-frame box that region is the cuboid; for any other vertex list the three slabs meet in the DUAL
// parallelepiped, centre +- g_1 +- g_2 +- g_3, g_i = (e_j x e_k) |e_i|^2 / (2 det), which reaches beyond the vertices'
// hull -- a tile / candidate range sized by the vertices alone never looks at the points in between (found by a soak).
// A degenerate vertex list leaves the region unbounded: the corners then go to the 1 m search ball's box.
void collision_extent_points(const dddmr_theory_config& c, double out[16][3]) {
  double ctr[3] = {0, 0, 0}, e[3][3], g[3][3];
  for (int k = 0; k < 8; ++k)
    for (int a = 0; a < 3; ++a) { out[k][a] = c.cuboid[k][a]; ctr[a] += c.cuboid[k][a] / 8.0; }
  for (int i = 0; i < 3; ++i)
    for (int a = 0; a < 3; ++a) e[i][a] = (double)c.cuboid[i + 1][a] - (double)c.cuboid[0][a];
  auto cross = [](const double* u, const double* v, double* w) {
    w[0] = u[1] * v[2] - u[2] * v[1]; w[1] = u[2] * v[0] - u[0] * v[2]; w[2] = u[0] * v[1] - u[1] * v[0];
  };
  double cr[3][3];
  cross(e[1], e[2], cr[0]); cross(e[2], e[0], cr[1]); cross(e[0], e[1], cr[2]);
  const double det = e[0][0] * cr[0][0] + e[0][1] * cr[0][1] + e[0][2] * cr[0][2];
  const bool ok = std::fabs(det) > 1e-12;
  for (int i = 0; i < 3; ++i) {
    const double n2 = e[i][0] * e[i][0] + e[i][1] * e[i][1] + e[i][2] * e[i][2];
    for (int a = 0; a < 3; ++a) g[i][a] = ok ? cr[i][a] * n2 / (2.0 * det) : 0.0;
  }
  for (int corner = 0; corner < 8; ++corner)
    for (int a = 0; a < 3; ++a) {
      double v = ctr[a];
      for (int i = 0; i < 3; ++i) v += ((corner >> i) & 1) ? g[i][a] : -g[i][a];
      if (!ok) v = ((corner >> a) & 1) ? 1.0 : -1.0;
      out[8 + corner][a] = std::max(-3.0, std::min(3.0, v));
    }
}

// Extent of the local costmap tile: every cloud point that can be inside any
// cuboid of any trajectory of this tick.  A pose stays within rho =
// max speed * sim_time of base_link in the body xy-plane, a cuboid vertex
// within rv of its pose (any yaw), so the body-frame box
// [-(rho+rv), rho+rv]^2 x [vz_min, vz_max] bounds all vertices; points further
// than 1 m from every pose are ignored by the critic's radius search anyway
// (collision_model.cpp:122).
void tile_extent(const dddmr_theory_config& c, const Window& w, const double R[9], const double t[3],
                 double sim_time, float rmin[3], float rmax[3]) {
  double rho;
  if (c.kind == DDDMR_THEORY_DD_ROTATE_INPLACE) {
    rho = 0.0;
  } else if (w.list_mode) {
    double m = 0;
    for (const auto& s : w.list) m = std::max(m, std::hypot((double)s.x, (double)s.y));
    rho = m * sim_time;
  } else {
    rho = std::hypot((double)absmax(w.ax), (double)absmax(w.ay)) * sim_time;
  }
  rho = rho * 1.001 + 0.01;  // float state rounding
  double rv = 0, vz0 = 1e30, vz1 = -1e30;
  double ext[16][3];
  collision_extent_points(c, ext);
  for (int k = 0; k < 16; ++k) {
    rv = std::max(rv, std::hypot(ext[k][0], ext[k][1]));
    vz0 = std::min(vz0, ext[k][2]);
    vz1 = std::max(vz1, ext[k][2]);
  }
  const double e = rho + rv;
  const double margin = 0.02;
  for (int i = 0; i < 3; ++i) {
    double lo = 1e30, hi = -1e30;
    for (int corner = 0; corner < 8; ++corner) {
      const double bx = (corner & 1) ? e : -e, by = (corner & 2) ? e : -e, bz = (corner & 4) ? vz1 : vz0;
      const double v = R[3 * i + 0] * bx + R[3 * i + 1] * by + R[3 * i + 2] * bz + t[i];
      lo = std::min(lo, v);
      hi = std::max(hi, v);
    }
    // radius criterion: within 1 m of some pose, poses within rho of base_link
    lo = std::max(lo, t[i] - (rho + 1.0));
    hi = std::min(hi, t[i] + (rho + 1.0));
    rmin[i] = (float)(lo - margin);
    rmax[i] = (float)(hi + margin);
  }
}

// the command of global sample `idx` of the last collected tick (samples are a closed-form grid, or the
// tick's explicit list: every rank can recompute the winner's command from its index)
void sample_of(const Window& w, int idx, float* vx, float* vy, float* wz) {
  if (w.list_mode) {
    *vx = w.list[idx].x; *vy = w.list[idx].y; *wz = w.list[idx].z;
  } else {
    const int nth = (int)w.ath.size(), ny = (int)w.ay.size();
    *vx = w.ax[(idx / nth) / ny];
    *vy = w.ay[(idx / nth) % ny];
    *wz = w.ath[idx % nth];
  }
}

// What dddmr_rollout_create reads from the environment and the device, as far as planning a tick uses it.
struct TickKnobs {
  float cell_size = 0.25f;
  bool cell_forced = false;   // DDDMR_CELL given: no automatic growth on big shards
  bool gnz_one = false;       // DDDMR_GNZ_ONE: one cell column per (x, y)
  int tile_override = 0;      // DDDMR_TILE: trajectories per k_score workgroup
  int threads_override = 0;   // DDDMR_THREADS: force the 256- or 512-lane k_score
  int rt_override = 0;        // DDDMR_RT: trajectories per rollout workgroup
  bool tail_round = false;    // DDDMR_TAIL_ROUND=1: one last round of short k_score workgroups (measured: C3 +3 us, C4 -7 us; off)
  int final_mode = -1;        // DDDMR_FINAL: 1 always decode in k_finalize, 0 always in k_score's last workgroup, -1 by shard size
  int probe_mode = -1;        // DDDMR_PROBE: 1 / 0 force the walk's probe round on / off, -1 by collided_share
  bool no_assign = false;     // DDDMR_NO_ASSIGN: always deal the trajectories strided
  bool no_boxfast = false;    // DDDMR_NO_BOXFAST: always take the general vertex transform
  bool no_tab = false;        // DDDMR_NO_TAB: k_score reads the row-run index from L2 instead of staging it in LDS
  bool heading_rows = true;   // DDDMR_HEADING_ROWS=0: a heading chain per trajectory on every tick (rollout_kernels.hip.h)
  bool fuse_walk = true;      // DDDMR_FUSE_WALK=0: phase P always stays a phase of its own behind the collision walk
  bool skip_dead = true;      // DDDMR_SKIP_DEAD=0: a fused tick walks the plan and sums the distances of rejected trajectories too
  int deal_mode = -1;         // DDDMR_DEAL: -1 by shard size (TickPlan::deal), 0 always the snake, 1 / 2 sorted / light tail wherever there is an assignment
  int n_cu = 256;             // compute units of the device
};

// What the previous tick left for this one.  plan_tick only reads it; the caller files the new values.
struct TickFeedback {
  int load_theory = -1, load_nlocal = -1;   // what traj_load (device) describes
  float collided_share = 1.0f;              // share of the last tick's trajectories the collision critics rejected
};

enum SampleUpload {     // how the tick's samples reach the device
  kUploadNone = 0,      // nobody reads them (empty shard, no exchange)
  kUploadList,          // explicit list -> samples_dev
  kUploadAxesInline,    // axes inside DevTick::axes_inl: no copy
  kUploadAxesDev        // axes -> axes_dev
};

// Every number one tick's kernels are launched with.
struct TickPlan {
  DevTick k{};              // complete but for seq
  int s_tick = 0;           // horizon: steps of the tick's longest trajectory
  int rank = 0;             // cfg.rank, clamped to the world
  int thr = 512;            // k_score lanes
  size_t score_lds = 0;     // k_score dynamic LDS
  bool lean = false;        // k_score without pose records, min-max critic and general vertex transform
  int cnt_blocks = 0;       // binning workgroups of the k_bin_count launch
  int bin_blocks = 0;       // k_bin_scatter workgroups
  int roll_blocks = 0;      // rollout workgroups, riding along with k_bin_count
  size_t roll_lds = 0;      // the rollout's own dynamic LDS: its [rt][steps + 1] slots
  int heading_rows = 0;     // 1: the rollout shares heading rows per angular sample (heading_rows_shared())
  size_t roll_launch_lds = 0;   // dynamic LDS of the launch that rolls out: roll_lds, plus the rows when they are shared
  int fused_walk = 0;       // 1: k_score walks the prune plan as the tail of the collision walk, for every pair (fused_walk_share_max())
  int skip_dead = 0;        // 1: the fused walk and the StickPath sums leave out the trajectories the collision walk rejected (fused ticks only)
  int deal = 0;             // how the load-feedback assignment deals the trajectories to k_score's workgroups (deal_slot(): kDealSnake, kDealSorted, kDealLightTail)
  int deal_head = 0;        // kDealLightTail: workgroups per assignment group that belong to the launch's whole rounds of resident workgroups
  SampleUpload upload = kUploadNone;
  uint32_t n_samples = 0, local_begin = 0, n_local = 0;   // the result's head
};

// The fused walk (k_score, rollout_kernels.hip.h) spends phase P's arithmetic on every pair of a tile, colliding or not.
// The separate phase walks the plan with one lane per SURVIVING pair and halves its work (two lanes a pair) once a tile
// has at most 256 of them.  With `pairs` = tile x max_steps pairs a tile and a share c of the trajectories colliding, a
// typical tile keeps pairs x (1 - c): more than 256, i.e. nothing saved by waiting for the verdicts, while
// c <= 1 - 256 / pairs.  Derived, not tuned.  (C3: 6 x 80 pairs, bound 0.467; C2: 8 x 50, bound 0.36.)
inline float fused_walk_share_max(int pairs) { return 1.0f - 256.0f / (float)pairs; }

// dynamic LDS of a k_score workgroup of `tile` trajectories in the tick k describes
size_t plan_score_lds(const DevTick& k, int tile) {
  return score_lds_bytes(tile, k.max_steps, k.m, rec_words_of(k.rec_pose != 0, k.want_minmax != 0), k.tab_entries, k.rows_cap);
}

// The shard, the horizon, the local costmap grid, the k_score workgroup shape and the rollout tile of one tick, into
// *p (filled in place).  Returns DDDMR_OK or the tick's error code with its message in *err.
int plan_tick(const TickKnobs& kn, const TickFeedback& fb, const dddmr_rollout_config& cfg, const dddmr_theory_config& th,
              int theory_id, const dddmr_tick_input& in, const Window& w, uint32_t n_points, uint32_t plan_m,
              const double plan_last[7], bool exchange, TickPlan* p, std::string* err) {
  // ---- initialise(): velocity samples of this tick, and this rank's shard of them ----
  const size_t N = w.count();
  if (N > cfg.max_trajectories) {
    *err = std::to_string(N) + " samples > max_trajectories " + std::to_string(cfg.max_trajectories);
    return DDDMR_ERR_CAPACITY;
  }
  if (!w.list_mode && (w.ax.size() > (size_t)kMaxAxis || w.ay.size() > (size_t)kMaxAxis || w.ath.size() > (size_t)kMaxAxis)) {
    *err = "sample axis longer than " + std::to_string(kMaxAxis);
    return DDDMR_ERR_CAPACITY;
  }
  const int world = std::max(1, cfg.world_size);
  const int rank = std::min(std::max(0, cfg.rank), world - 1);
  const uint32_t begin = (uint32_t)((uint64_t)rank * N / world);
  const uint32_t end = (uint32_t)((uint64_t)(rank + 1) * N / world);
  p->rank = rank;
  p->n_samples = (uint32_t)N;
  p->local_begin = begin;
  p->n_local = end - begin;

  DevTick& k = p->k;
  k = DevTick{};
  k.kind = th.kind;
  k.fixed_steps = th.bench_fixed_steps > 0 ? th.bench_fixed_steps : 0;
  k.list_mode = w.list_mode ? 1 : 0;
  k.n_global = (int)N;
  k.begin = (int)begin;
  k.n_local = (int)(end - begin);
  k.nx = (int)std::max<size_t>(w.ax.size(), 1);
  k.ny = (int)std::max<size_t>(w.ay.size(), 1);
  k.nth = (int)std::max<size_t>(w.ath.size(), 1);
  k.ay_ofs = kMaxAxis;
  k.ath_ofs = 2 * kMaxAxis;
  k.sim_time = th.sim_time;
  k.sim_gran = th.sim_granularity;
  k.ang_gran = th.angular_sim_granularity;
  k.min_vel_x = th.min_vel_x;
  k.max_vel_x = th.max_vel_x;
  k.min_vel_theta = th.min_vel_theta;
  k.min_vel_trans = th.min_vel_trans;
  k.max_vel_trans = th.max_vel_trans;
  k.allowed_max = in.allowed_max_linear_speed;
  quat_to_rot(in.robot_pose, k.R);
  for (int i = 0; i < 3; ++i) k.t[i] = in.robot_pose[i];
  for (int v = 0; v < 8; ++v)
    for (int j = 0; j < 3; ++j) k.cub[3 * v + j] = th.cuboid[v][j];
  k.m = (int)plan_m;
  quat_to_rot(plan_last, k.planR);
  for (int i = 0; i < 3; ++i) k.planT[i] = plan_last[i];
  k.n_critics = th.n_critics;
  for (int m = 0; m < th.n_critics; ++m) {
    k.ckind[m] = th.critics[m].kind;
    k.cw[m] = th.critics[m].weight;
    k.ctw[m] = th.critics[m].translation_weight;
    k.cow[m] = th.critics[m].orientation_weight;
    if (k.ckind[m] == DDDMR_CRITIC_COLLISION) k.want_collision = 1;
    if (k.ckind[m] == DDDMR_CRITIC_COLLISION_MIN_MAX) k.want_minmax = 1;
  }
  k.heading_dev = in.heading_deviation;

  // ---- horizon of this tick (monotone in |v| and |w|, so the axis extremes bound it) ----
  double sim_time_eff = th.sim_time;
  int s_tick;
  {
    double vmax, wmax;
    if (w.list_mode) {
      vmax = 0; wmax = 0;
      for (const auto& s : w.list) {
        vmax = std::max(vmax, std::hypot((double)s.x, (double)s.y));
        wmax = std::max(wmax, std::fabs((double)s.z));
      }
    } else {
      vmax = std::hypot((double)absmax(w.ax), (double)absmax(w.ay));
      wmax = (double)absmax(w.ath);
    }
    if (th.bench_fixed_steps > 0) {
      s_tick = th.bench_fixed_steps;
    } else if (th.kind == DDDMR_THEORY_DD_ROTATE_INPLACE) {
      s_tick = (int)std::ceil(std::max(0.0, 6.28 / th.angular_sim_granularity)) + 1;
      sim_time_eff = 0.0;
    } else {
      s_tick = (int)std::ceil(std::max(vmax * th.sim_time / th.sim_granularity,
                                       wmax * th.sim_time / th.angular_sim_granularity)) + 1;
    }
    s_tick = std::max(s_tick, 1);
  }
  if ((uint32_t)s_tick > cfg.max_steps) {
    *err = "horizon of " + std::to_string(s_tick) + " steps > max_steps " + std::to_string(cfg.max_steps);
    return DDDMR_ERR_CAPACITY;
  }
  k.max_steps = s_tick;
  p->s_tick = s_tick;

  // ---- local costmap tile ----
  k.n_points = (int)n_points;
  tile_extent(th, w, k.R, k.t, sim_time_eff, k.rmin, k.rmax);
  // What the collision critics look at around one pose: its largest chord (a cuboid's AABB, clipped to the 2 m wide
  // search ball, must not span more than kRows cell rows: rows <= span / cell + 2) and its reach from the pose.
  double diam = 0, vnorm = 0;
  {
    double ext[16][3];       // (the corners of the box the collision critic derives count too)
    collision_extent_points(th, ext);
    for (int a = 0; a < 16; ++a) {
      vnorm = std::max(vnorm, std::sqrt(ext[a][0] * ext[a][0] + ext[a][1] * ext[a][1] + ext[a][2] * ext[a][2]));
      for (int b = a + 1; b < 16; ++b) {
        const double dx = ext[a][0] - ext[b][0], dy = ext[a][1] - ext[b][1], dz = ext[a][2] - ext[b][2];
        diam = std::max(diam, std::sqrt(dx * dx + dy * dy + dz * dz));
      }
    }
    diam += 4e-4;     // the candidate range's margin on both sides (k_score phase D1)
  }
  float cell = std::max(kn.cell_size, (float)(std::min(diam, 2.0) * 1.001 / (kRows - 2)));
  float cell_z = cell;     // z cells do not grow with the x/y cells below
  // Big shards run many 256-lane workgroups per CU and are bound by how many (trajectory,
  // step) slots fit a CU's LDS; a slot's row segments are the largest part of it, so there the
  // cells grow until a cuboid spans at most 4 rows (C3 k_score 143 -> 122 us, C4 342 -> 298 us
  // at 0.42 m).  Shards that fit one round of 512-lane workgroups keep the small cells: their
  // LDS is not the limit and bigger cells make the counting atomics collide (C2 binning
  // +3 us at 0.42 m, +7 us at 0.5 m).
  if (!kn.cell_forced && k.n_local > kn.n_cu * kMaxTile)
    cell = std::max(cell, std::min(0.5f, (float)(std::min(diam, 2.0) * 1.001 / 2.9)));
  for (;;) {
    k.gnx = std::max(1, (int)std::ceil((k.rmax[0] - k.rmin[0]) / cell));
    k.gny = std::max(1, (int)std::ceil((k.rmax[1] - k.rmin[1]) / cell));
    // Candidate runs always take every z of a row, but one cell column per (x, y) makes the
    // counting atomics of wall points collide (measured: k_bin_count 13 -> 17 us); keep z.
    k.gnz = kn.gnz_one ? 1 : std::max(1, (int)std::ceil((k.rmax[2] - k.rmin[2]) / cell_z));
    const uint64_t nc = (uint64_t)k.gnx * k.gny * k.gnz;
    if (nc <= kCapCells && k.gnx < 32000 && k.gny < 32000) { k.n_cells = (int)nc; break; }
    cell *= 1.5f;
    cell_z *= 1.5f;
  }
  k.inv_cell = 1.0f / cell;
  k.inv_cell_z = 1.0f / cell_z;
  for (int i = 0; i < 3; ++i) k.gmin[i] = k.rmin[i];
  // rows <= floor(span / cell) + 2 (span = cuboid diameter clipped to the 2 m search ball)
  k.rows_cap = std::min(kRows, (int)std::floor(std::min(diam, 2.0) * 1.001 / cell) + 2);
  {
    // box in the body frame, vertices in the push order blb brb blt flb brt frt flt frb
    // (dd_simple_trajectory_generator_theory.cpp:211-218)?  Then k_score shares the products.
    const float (*c)[3] = th.cuboid;
    const float X0 = c[0][0], X1 = c[3][0], Y0 = c[0][1], Y1 = c[1][1], Z0 = c[0][2], Z1 = c[2][2];
    const float want[8][3] = {{X0, Y0, Z0}, {X0, Y1, Z0}, {X0, Y0, Z1}, {X1, Y0, Z0},
                              {X0, Y1, Z1}, {X1, Y1, Z1}, {X1, Y0, Z1}, {X1, Y1, Z0}};
    bool box = true;
    for (int v = 0; v < 8; ++v)
      for (int a = 0; a < 3; ++a) box = box && (c[v][a] == want[v][a]);
    k.box_fast = (box && !kn.no_boxfast) ? 1 : 0;
  }
  // OBB records carry the pose only if some pair can need the 1 m radius test: a point
  // inside the box is within max|vertex| of the pose, so a cuboid that lies inside the
  // search ball never does (the min-max critic always needs it).
  k.rec_pose = (vnorm >= 0.985 || k.want_minmax) ? 1 : 0;
  {
    const long te = (long)(k.gnx + 1) * k.gny;
    k.tab_entries = (te <= kTabCap && k.n_points >= 5 && (k.want_collision || k.want_minmax) && !kn.no_tab) ? (int)te : 0;
  }

  // ---- k_score workgroup shape: trajectories per workgroup, ~one (trajectory, step) pair per lane ----
  // Per-workgroup fixed costs (staging the plan and the row-run index, ~13 barriers, the wave-0 scans) make few, fat
  // workgroups win: measured on the r02 scenes, k_score at C3 (80-step rows) 256 lanes x tile 2 / 3 / 4 -> 222 / 158 /
  // 152 us, 512 lanes x tile 6 -> 132 us; C4 (50-step rows) 256 lanes x tile 3 / 5 / 7 -> 564 / 344 / 336 us, 512 lanes
  // x tile 8 / 10 / 11 -> 347 / 304 / 320 us.  So: 512 lanes (two workgroups per CU at 4 waves per SIMD and <= 80 KB of
  // LDS each) and
  //  - a shard that fits ONE round of resident workgroups is spread evenly over them (C2: tile 8, 512 workgroups): the
  //    launch is bound by its heaviest tile's collision walk, and 512 lanes both halve it and average over more
  //    trajectories;
  //  - a bigger shard takes the largest tile whose (trajectory, step) pairs still fit the lanes (one pair per lane
  //    in D1 / D2) and whose LDS fits twice into a CU.
  // (1024-lane workgroups, one per CU, lose again: C3 143 us at tile 12, C4 390 us at tile 16.)
  // DDDMR_THREADS=256 / DDDMR_TILE keep the 256-lane shape reachable for experiments.
  int thr = 512;
  auto lds_of = [&](int t) { return plan_score_lds(k, t); };
  auto tile_for_256 = [&]() {
    // most (trajectory, step) slots resident per CU: workgroups per CU (by registers, fewer by LDS) x slots per
    // workgroup, slots <= lanes
    int t_best = 1;
    long best = 0;
    for (int t = 1; t <= kMaxTile; ++t) {
      if (t > 1 && t * s_tick > 256) break;
      const size_t need = lds_of(t) + 1024;   // + static LDS
      const long wgs = std::min<long>(DDDMR_SCORE_WPE_256, (long)((size_t)(160 * 1024) / need));
      const long resident = wgs * t * s_tick;
      if (resident >= best) { best = resident; t_best = t; }
    }
    return t_best;
  };
  int tile = 1;
  if (kn.tile_override > 0) {
    tile = std::min(kn.tile_override, kMaxTile);
    thr = kn.threads_override > 0 ? kn.threads_override : 256;
  } else if (kn.threads_override == 256) {
    thr = 256;
    tile = tile_for_256();
  } else if (k.n_local > 0) {
    const int slots512 = kn.n_cu * 2;
    const int fit = (k.n_local + slots512 - 1) / slots512;
    if (fit <= kMaxTile && fit * s_tick <= 2 * 512 && lds_of(fit) <= (size_t)80 * 1024) {
      tile = std::max(fit, 1);
    } else {
      for (int t = 2; t <= kMaxTile; ++t) {
        if (t * s_tick > 512 || lds_of(t) > (size_t)80 * 1024) break;
        tile = t;
      }
    }
  }
  while (tile > 1 && lds_of(tile) > (size_t)(160 * 1024) / 2) --tile;
  const size_t lds = lds_of(tile);
  if (lds > (size_t)kScoreLdsMax) {
    *err = "horizon needs " + std::to_string(lds) + " bytes of LDS";
    return DDDMR_ERR_CAPACITY;
  }
  k.tile = tile;
  p->thr = thr;
  p->score_lds = lds;
  p->lean = !k.want_minmax && !k.rec_pose && k.box_fast;
  // Who decodes the winner: shards that run as ONE round of workgroups let the last workgroup do it (a
  // finalize launch would cost the tick ~3 us); bigger shards run several rounds, where every workgroup's ticket
  // round trip holds a slot that the next workgroup is waiting for -- there k_finalize follows and scores the stacks too.
  // The collision walk's probe round (every lane first walks ONE item, spread evenly over the tile's list) settles
  // colliding trajectories early; when few collide it is a barrier and a scan for nothing.  Measured: 86 %
  // colliding (C3, r01 scene) k_score 114 us with / 155 us without; 25 % colliding (r02 scenes) C3 126.5 / 124.0 us,
  // C4 295.6 / 285.2 us.  Decided by the share the previous tick of the same theory and shard measured; either way
  // gives identical results.
  const bool same_as_last = fb.load_theory == theory_id && fb.load_nlocal == k.n_local;
  k.probe = kn.probe_mode >= 0 ? kn.probe_mode : ((!same_as_last || fb.collided_share > 0.5f) ? 1 : 0);
  // The prune-plan walk as the tail of the collision walk: lean launches whose pairs fit one pass of lanes, phase P on its
  // one-lane-per-pose route (more than 256 pairs), and few enough collisions that waiting for the verdicts would save
  // it nothing (fused_walk_share_max()).  A context's first tick (share 1.0) keeps the separate phase.  Either way
  // gives identical results.
  {
    const int pairs = tile * s_tick;
    p->fused_walk = (kn.fuse_walk && k.n_local > 0 && p->lean && k.want_collision && k.n_points >= 5 && k.m >= 1 && pairs <= thr &&
                     pairs > 256 && fb.collided_share <= fused_walk_share_max(pairs)) ? 1 : 0;
    p->skip_dead = (kn.skip_dead && p->fused_walk) ? 1 : 0;
  }
  const bool one_round = k.n_local <= 0 || (k.n_local + tile - 1) / tile <= kn.n_cu * (thr == 512 ? 2 : 4);
  k.final_kernel = kn.final_mode >= 0 ? kn.final_mode : (one_round ? 0 : 1);

  // How the samples travel (sample axes or explicit list).  A rank with an EMPTY shard needs them too when the context
  // exchanges winners: k_resolve decodes the global winner's command from them on every rank (rotate-in-place has two
  // samples, so rank 0 of three or more ranks owns none).
  p->upload = kUploadNone;
  if (k.n_local > 0 || exchange) {
    if (w.list_mode) {
      p->upload = kUploadList;
    } else if (w.ax.size() + w.ay.size() + w.ath.size() <= (size_t)kInlineAxes) {
      p->upload = kUploadAxesInline;          // axes ride in the kernel arguments
      k.axes_inline = 1;
      k.ay_ofs = (int)w.ax.size();
      k.ath_ofs = (int)(w.ax.size() + w.ay.size());
      std::memcpy(k.axes_inl, w.ax.data(), w.ax.size() * sizeof(float));
      std::memcpy(k.axes_inl + k.ay_ofs, w.ay.data(), w.ay.size() * sizeof(float));
      std::memcpy(k.axes_inl + k.ath_ofs, w.ath.data(), w.ath.size() * sizeof(float));
    } else {
      p->upload = kUploadAxesDev;
    }
  }

  // ---- rollout tile ----
  if (k.n_local > 0) {
    // Rollout workgroups ride along with k_bin_count.  Few, fat workgroups win: dispatching a
    // 1024-lane workgroup costs ~12 ns, which is what bounds the launch on big shards (C4:
    // 64 trajectories per workgroup 44 us, 32: 56 us, 16: 86 us), and on small ones ~128
    // workgroups are the sweet spot (C2: 16 per workgroup 14.4 us, 32: 12.1 us, 64: 13.2 us).
    // Round 2: the launch's dynamic LDS (the rollout rows, 16 bytes per pair) is allocated by EVERY workgroup of
    // k_bin_count, and a CU holds two 1024-lane workgroups at most (wave slots).  Rows sized for two per CU
    // (<= 74 KB beside ~6 KB of static LDS) keep the whole launch resident in one round at C3 (the rollout
    // workgroups used to start in two rounds: k_bin_count 28 -> ~18 us).  Within a quarter of that cap the row count
    // that fills phase B's 1024-lane passes best wins (C3: 50 x 81 pairs = 3.96 passes, C4: 80 x 51 = 3.98).
    const int s1 = s_tick + 1;
    const int rt_lds = (int)std::min<size_t>((size_t)kRolloutMax, ((size_t)74 * 1024 - 16) / ((size_t)s1 * 16));
    int rt = std::min(std::max((k.n_local + 127) / 128, 4), std::max(rt_lds, 1));
    if (rt == rt_lds && rt > 4) {
      double best_fill = 0.0;
      for (int c = rt_lds; c >= rt_lds - rt_lds / 4; --c) {
        const int items = c * s1;
        const double fill = (double)items / (double)((items + kBinThreads - 1) / kBinThreads * kBinThreads);
        if (fill > best_fill + 1e-9) { best_fill = fill; rt = c; }
      }
    }
    if (kn.rt_override > 0) rt = std::min(kn.rt_override, kRolloutMax);
    while (rt > 1 && rollout_lds_bytes(rt, s_tick) > (size_t)128 * 1024) --rt;
    k.rt = rt;
  }

  // ---- launch grids ----
  p->bin_blocks = std::max(1, std::min(2048, (k.n_points + 255) / 256));
  // one point per lane while that needs few workgroups (latency), kBinPer per lane beyond (dispatch cost)
  const int per_wg = k.n_points <= 128 * kBinThreads ? kBinThreads : kBinThreads * kBinPer;
  p->cnt_blocks = std::max(1, std::min(512, (k.n_points + per_wg - 1) / per_wg));
  p->roll_blocks = k.n_local > 0 ? (k.n_local + k.rt - 1) / k.rt : 0;
  p->roll_lds = k.n_local > 0 ? rollout_lds_bytes(k.rt, s_tick) : 0;
  // Heading rows per angular sample (rollout_kernels.hip.h, heading_rows_shared()): handed to the rollout as an argument
  // of its own.  The rows' LDS comes on top of the rollout's; a tick whose rollout workgroups would no longer sit two to
  // a CU with it (72 KB of dynamic LDS beside k_bin_count's 8 KB of static) keeps a chain per trajectory.
  p->heading_rows = 0;
  p->roll_launch_lds = p->roll_lds;
  if (kn.heading_rows && heading_rows_shared(k)) {
    const size_t with_rows = p->roll_lds + heading_rows_lds_bytes(k.max_steps, k.kind == DDDMR_THEORY_OMNI_SIMPLE);
    const size_t two_per_cu = (size_t)72 * 1024;
    if (with_rows <= (size_t)kScoreLdsMax && (with_rows <= two_per_cu || p->roll_lds > two_per_cu)) {
      p->roll_launch_lds = with_rows;
      p->heading_rows = 1;
    }
  }
  k.bin_blocks = p->cnt_blocks;
  k.roll_blocks = p->roll_blocks;
  // Load feedback: valid when the previous tick scored the same shard of the same theory
  // (its loads are indexed by local trajectory).  Otherwise this tick deals strided.
  k.n_tiles = k.n_local > 0 ? (k.n_local + tile - 1) / tile : 0;
  k.assign_groups = std::max(1, (k.n_local + kAssignPer * kBinThreads - 1) / (kAssignPer * kBinThreads));
  k.use_assign = (!kn.no_assign && k.n_tiles > 1 && k.n_local <= kAssignMax && same_as_last) ? 1 : 0;
  if (k.use_assign) k.n_tiles = (k.n_tiles + k.assign_groups - 1) / k.assign_groups * k.assign_groups;
  k.nb_tiles = k.n_tiles;
  k.r0 = 0;
  // Several rounds of resident workgroups: full workgroups for the whole rounds, ONE last round of short workgroups
  // for the rest (rollout_kernels.hip.h, tile_slot()); the lightest trajectories of the load-feedback deal land in it.
  // Built, bit-identical, measured and left OFF (DDDMR_TAIL_ROUND=1): a k_score workgroup's life is mostly fixed cost
  // (staging, ~13 barriers, scans), so 512 two-trajectory workgroups cost the C3 launch what its 171 full ones did:
  // C3 tick 156.2 -> 159.1 us, C4 337.3 -> 330.3 us (profiles/r03_tail_round.txt).
  if (!one_round && tile > 1 && kn.tail_round && k.n_local <= kAssignMax) {
    const int G = k.assign_groups;
    const long slots = (long)kn.n_cu * (thr == 512 ? 2 : 4);
    const long whole = (long)k.n_local / (slots * tile);                         // rounds of full workgroups
    const long rem = (long)k.n_local - whole * slots * tile;
    const int t2 = (int)((rem + slots - 1) / slots);                             // trajectories of a short workgroup
    if (whole >= 1 && rem > 0 && t2 < tile) {
      const int nb = (int)((whole * slots + G - 1) / G * G), ns = (int)((slots + G - 1) / G * G);
      if ((long)nb * tile + (long)ns * t2 >= k.n_local) {
        k.nb_tiles = nb;
        k.n_tiles = nb + ns;
        k.r0 = tile - t2;
      }
    }
  }
  // The deal (rollout_kernels.hip.h, deal_slot()).  The snake makes all workgroups equally heavy, which is what bounds a
  // launch of ONE round of resident workgroups.  On a shard of several rounds equal lives mean the last, partial round
  // runs a full life on a mostly empty chip (C3: 2731 workgroups on 512 slots, 171 in the sixth round); there the sorted
  // deal dispatches the heaviest tiles first and ends on the cheapest.  The tail-round layout keeps the snake.
  // DDDMR_DEAL=1 / 2 force the sorted / light-tail deal wherever there is an assignment (tests, measurements).
  {
    const bool layout_ok = k.use_assign && k.r0 == 0;
    const long slots = (long)kn.n_cu * (thr == 512 ? 2 : 4);
    p->deal = kDealSnake;
    if (kn.deal_mode < 0) { if (layout_ok && !one_round && tile > 1) p->deal = kDealSorted; }
    else if (kn.deal_mode > 0 && layout_ok) p->deal = kn.deal_mode == kDealLightTail ? kDealLightTail : kDealSorted;
    p->deal_head = (p->deal == kDealLightTail) ? (int)(((long)k.n_tiles / slots) * slots / k.assign_groups) : 0;
  }
  return DDDMR_OK;
}

}  // namespace
