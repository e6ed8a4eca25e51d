// marking_plan.hip.h -- the host side of a marking update that is arithmetic alone: the transforms and MarkParams of one
// update (make_update_frame) and plan_fused_update(): every number the kernels of
// marking_fused.hip.h are launched with.  Host code only -- no HIP runtime call, no getenv, no context -- so that
// tests/cpp/marking_plan_test.cpp can replay recorded updates through it on a machine without a GPU.
//
// Citations are lines of the reference's src/dddmr_perception_3d/plugins/multilayer_spinning_lidar.cpp.
#pragma once
#include <algorithm>
#include <cmath>

#include "marking_fused.hip.h"
#include "point_grid_plan.hip.h"   // grid_shape, host_cx / host_cy
#include "tick_plan.hip.h"         // quat_to_rot

namespace {

using namespace dddmr;

void quat_rotate_z(const double q[4], double out[3]) {   // tf2::quatRotate(q, (0, 0, 1)); q = x y z w
  // q * v
  const double ax = q[1] * 1.0, ay = -q[0] * 1.0, az = q[3] * 1.0, aw = -q[2] * 1.0;   // (w*0 + y*1 - z*0, w*0 + z*0 - x*1, w*1 + x*0 - y*0, -x*0 - y*0 - z*1)
  // (q * v) * q^-1, q^-1 = (-x, -y, -z, w)
  const double bx = -q[0], by = -q[1], bz = -q[2], bw = q[3];
  out[0] = aw * bx + ax * bw + ay * bz - az * by;
  out[1] = aw * by + ay * bw + az * bx - ax * bz;
  out[2] = aw * bz + az * bw + ax * by - ay * bx;
}

// ModelCoefficients of the plane through base_link with base z as its normal (:401-409; depth camera :568-578):
// tf2::quatRotate(q, (0, 0, 1)) and d in double, each rounded to float
void base_plane(const double T_gbl_base[7], float mc[4]) {
  const double qb[4] = {T_gbl_base[3], T_gbl_base[4], T_gbl_base[5], T_gbl_base[6]};
  double nb[3];
  quat_rotate_z(qb, nb);
  mc[0] = (float)nb[0]; mc[1] = (float)nb[1]; mc[2] = (float)nb[2];
  const double d = -T_gbl_base[0] * nb[0] - T_gbl_base[1] * nb[1] - T_gbl_base[2] * nb[2];
  mc[3] = (float)d;
}
// what an update's MarkParams take from the robot's pose: the base plane and selfClear's window in voxel keys
// (lidar :489-496, depth camera :280-287), from k's own res / hres / window / marking_height
void mark_params_pose(MarkParams& k, const double T_gbl_base[7]) {
  base_plane(T_gbl_base, k.mc);
  k.wx0 = (int)((T_gbl_base[0] - k.window) / k.res);
  k.wx1 = (int)((T_gbl_base[0] + k.window) / k.res);
  k.wy0 = (int)((T_gbl_base[1] - k.window) / k.res);
  k.wy1 = (int)((T_gbl_base[1] + k.window) / k.res);
  k.wz0 = (int)((T_gbl_base[2] - k.marking_height) / k.hres);
  k.wz1 = (int)((T_gbl_base[2] + k.marking_height) / k.hres);
}

// Eigen quaternion of a rotation matrix (row-major R), as tf2::eigenToTransform forms trans_gbl2s_'s rotation
void rot_to_quat(const double R[9], double q[4]) {
  double t = R[0] + R[4] + R[8];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
  }
}
// tf2 Matrix3x3::setRotation(q), row-major
void tf2_set_rotation(const double q[4], double R[9]) {
  const double d = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const double s = 2.0 / d;
  const double xs = q[0] * s, ys = q[1] * s, zs = q[2] * s;
  const double wx = q[3] * xs, wy = q[3] * ys, wz = q[3] * zs;
  const double xx = q[0] * xs, xy = q[0] * ys, xz = q[0] * zs;
  const double yy = q[1] * ys, yz = q[1] * zs, zz = q[2] * zs;
  R[0] = 1.0 - (yy + zz); R[1] = xy - wz; R[2] = xz + wy;
  R[3] = xy + wz; R[4] = 1.0 - (xx + zz); R[5] = yz - wx;
  R[6] = xz - wy; R[7] = yz + wx; R[8] = 1.0 - (xx + yy);
}

struct UpdateFrame {          // host-side inputs of one update besides the kernel parameters
  MarkParams k;
  double Rb[9];               // rotation of T_gbl_base
  double t_gb[3];
};

// The transforms (host, double: trans_gbl2s_af3_ = gbl2b * b2s (:236-237), its tf2 form (:238)) and the MarkParams of one
// update.  n_prev: points of the previous selfMark's observation (0 = none yet); table, pool_cap: the marking store's;
// seq: the update's sequence number; pad: MarkParams::pad.
UpdateFrame make_update_frame(const dddmr_marking_config& c, const double T_base_sensor[7], const double T_gbl_base[7], uint32_t n_obs,
                              uint32_t n_prev, uint32_t table, uint32_t pool_cap, uint32_t n_ground, uint32_t n_alive, uint32_t seq,
                              float pad) {
  UpdateFrame f{};
  MarkParams& k = f.k;
  double Rbs[9], Rs_e[9], ts[3];
  quat_to_rot(T_gbl_base, f.Rb);
  quat_to_rot(T_base_sensor, Rbs);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rs_e[3 * i + j] = f.Rb[3 * i + 0] * Rbs[0 + j] + f.Rb[3 * i + 1] * Rbs[3 + j] + f.Rb[3 * i + 2] * Rbs[6 + j];
    ts[i] = f.Rb[3 * i + 0] * T_base_sensor[0] + f.Rb[3 * i + 1] * T_base_sensor[1] + f.Rb[3 * i + 2] * T_base_sensor[2] + T_gbl_base[i];
    f.t_gb[i] = T_gbl_base[i];
  }
  double qs[4];
  rot_to_quat(Rs_e, qs);
  tf2_set_rotation(qs, k.Rs);
  quat_rotate_z(qs, k.sn);
  for (int i = 0; i < 3; ++i) k.st[i] = ts[i];
  k.sd = -ts[0] * k.sn[0] - ts[1] * k.sn[1] - ts[2] * k.sn[2];
  k.res = c.xy_resolution; k.hres = c.height_resolution; k.marking_height = c.marking_height; k.window = c.perception_window_size;
  k.fov_top = c.vertical_FOV_top; k.fov_bottom = c.vertical_FOV_bottom;
  k.ps = c.scan_effective_positive_start; k.pe = c.scan_effective_positive_end;
  k.ns = c.scan_effective_negative_start; k.ne = c.scan_effective_negative_end;
  k.ignore_ratio = c.segmentation_ignore_ratio; k.inscribed = c.inscribed_radius; k.inflation = c.inflation_radius;
  k.tol = (float)c.euclidean_cluster_extraction_tolerance;
  k.tol2 = static_cast<float>(c.euclidean_cluster_extraction_tolerance * c.euclidean_cluster_extraction_tolerance);
  k.min_cluster = c.euclidean_cluster_extraction_min_cluster_size;
  mark_params_pose(k, T_gbl_base);
  k.n_obs = n_obs;
  k.n_prev = n_prev;
  k.pad = pad;
  k.table_mask = table - 1;
  k.pool_cap = pool_cap;
  k.n_ground = n_ground;
  k.n_alive_prev = n_alive;
  k.seq = seq;
  return f;
}

// the crop box of the feed (base frame |x|,|y| <= window, z in [0, marking_height]) in the global frame, + 0.3 m
void crop_box(const dddmr_marking_config& c, const UpdateFrame& f, float lo[3], float hi[3]) {
  for (int a = 0; a < 3; ++a) { lo[a] = 3.4e38f; hi[a] = -3.4e38f; }
  for (int corner = 0; corner < 8; ++corner) {
    const double bx = (corner & 1) ? c.perception_window_size : -c.perception_window_size;
    const double by = (corner & 2) ? c.perception_window_size : -c.perception_window_size;
    const double bz = (corner & 4) ? c.marking_height : 0.0;
    for (int a = 0; a < 3; ++a) {
      const float v = (float)(f.Rb[3 * a] * bx + f.Rb[3 * a + 1] * by + f.Rb[3 * a + 2] * bz + f.t_gb[a]);
      lo[a] = std::min(lo[a], v - 0.3f);
      hi[a] = std::max(hi[a], v + 0.3f);
    }
  }
}
// grid over it
void obs_grid_shape(const dddmr_marking_config& c, const UpdateFrame& f, uint32_t cap_cells, PointGrid& g, float lo[3], float hi[3]) {
  crop_box(c, f, lo, hi);
  const float cell = std::max(0.1f, f.k.tol);
  grid_shape(g, lo, hi, cell, cell, cap_cells);
}

// What dddmr_rollout_marking_create reads from the environment, as far as planning a fused update uses it.
struct MarkKnobs {
  uint32_t grid_parts = 4;                 // DDDMR_MKF_GRIDPARTS: workgroups that build the observation grid (1, 2, 4, 8)
  bool unmark_with_groups = true;          // DDDMR_MKF_UNMARK=roots: removePCPtr blocks in the seeds' launch instead of the partitions'
  bool grid_in_lds = true;                 // DDDMR_MKF_GRID=global: counts by a count launch's global atomics instead
  uint32_t splat_parts = 0;                // DDDMR_MKF_PARTS: blocks that share a row segment's bands in the commit launch (0: estimated)
  uint32_t unmark_parts = 8;               // DDDMR_MKF_UNPARTS (tuning)
  uint32_t fuse_cells = kFuseMaxCells;     // DDDMR_MKF_CELLS: cells of the fused route's observation grid (tuning)
};

// Every number one fused update's kernels are launched with.  A launch whose blocks add up to zero is skipped.
struct FusedPlan {
  bool mark = false;            // more than 5 points: selfMark runs (:320-321)
  bool big = false;             // more than kFuseRegObs points (the count launch's form of the grid only takes kFuseRegObs)
  PointGrid obs;                // geometry and point count of the observation grid (no storage); set when `mark`
  SplatRange rg{};              // ground cells of the window + inflation radius: the nodes the node-by-node dGraph updates look at
  uint32_t n_part = 0;          // blocks that share one row segment's bands in the commit launch
  uint32_t seg_groups = 0;
  uint32_t count_blocks = 0;    // count launch (DDDMR_MKF_GRID=global only): cell counts of the observation grid
  uint32_t nb_grid = 0, nb_slots = 0;                  // grid launch: the observation grid | every store slot: window + FOV test
  uint32_t nb_clear = 0, nb_cc = 0;                    // clear launch: ray tests | union-find
  uint32_t nb_roots = 0, nb_un = 0, nb_walk = 0;       // seed launch: seeds | removePCPtr by bands | point by point
  uint32_t n_part_un = 0;                              //   blocks that share a row segment's bands of removed markings
  uint32_t nb_un_groups = 0, nb_band_groups = 0;       // partition launch: kFuseParts partitions | removePCPtr (of them by bands)
  uint32_t nb_commit = 0, nb_b = 0, nb_commit_walk = 0;   // commit launch: keepers -> pool | dGraph by bands | point by point
  uint32_t grid_launch() const { return nb_grid + nb_slots; }
  uint32_t clear_launch() const { return nb_clear + nb_cc; }
  uint32_t seed_launch() const { return nb_roots + nb_un + nb_walk; }
  uint32_t part_launch() const { return mark ? (uint32_t)kFuseParts + nb_un_groups : 0u; }
  uint32_t commit_launch() const { return nb_commit + nb_b + nb_commit_walk; }
};

// Blocks that share one row segment's bands in the commit launch: a block takes every n_part-th 256-point chunk of the
// 2 delta + 1 bands in reach, so more blocks than chunks only add blocks that read the band counts and leave (measured at
// C5M, ~110 points per band, 9 bands in reach: n_part 48 / 24 / 16 / 12 / 8 -> mark phase 80 / 68 / 68 / 66 / 67 us).
// Estimated from the observation size (at most one generator point per observation point, about half in practice).
uint32_t plan_n_part(const MarkKnobs& kn, uint32_t n_obs, uint32_t bands, int delta) {
  if (kn.splat_parts) return kn.splat_parts;
  const uint32_t per_band = std::max(1u, n_obs / 2u / std::max(1u, bands));
  const uint32_t chunks = (2u * (uint32_t)delta + 1u) * ((per_band + 255u) / 256u);
  return std::min(48u, std::max(8u, chunks + chunks / 3u));
}

// ground: the ground grid's geometry, max_row the points of its fullest (y, z) row of cells; obs_cap_cells: what the
// observation grid's storage holds; table: slots of the marking store.
FusedPlan plan_fused_update(const MarkKnobs& kn, const dddmr_marking_config& cfg, const UpdateFrame& f, const PointGrid& ground,
                            uint32_t max_row, uint32_t n_ground, uint32_t obs_cap_cells, uint32_t n_obs, uint32_t n_alive,
                            uint32_t table) {
  FusedPlan p;
  p.mark = n_obs > 5;
  p.big = n_obs > kFuseRegObs;
  const bool mark = p.mark;
  float lo[3], hi[3];
  if (mark) {
    obs_grid_shape(cfg, f, std::min(obs_cap_cells, kn.fuse_cells), p.obs, lo, hi);
    p.obs.n = n_obs;
  }
  SplatRange& rg = p.rg;
  {
    crop_box(cfg, f, lo, hi);
    const float pad = (float)cfg.inflation_radius + 0.05f;
    rg.cx0 = host_cx(ground, lo[0] - pad); rg.cx1 = host_cx(ground, hi[0] + pad);
    rg.cy0 = host_cy(ground, lo[1] - pad); rg.cy1 = host_cy(ground, hi[1] + pad);
    rg.rows = (uint32_t)(rg.cy1 - rg.cy0 + 1) * (uint32_t)ground.nz;
    rg.segs = std::max(1u, (max_row + 63u) / 64u);
    rg.delta = (int)std::floor(((float)cfg.inflation_radius + 1e-3f) * ground.inv_xy) + 1;
    rg.bands = (n_ground && (uint32_t)(rg.cy1 - rg.cy0 + 1) <= kBandMax) ? (uint32_t)(rg.cy1 - rg.cy0 + 1) : 0u;
  }
  p.n_part = plan_n_part(kn, n_obs, rg.bands, rg.delta);
  p.seg_groups = (rg.segs + 3u) / 4u;
  const uint32_t nb_band = rg.bands ? rg.rows * p.seg_groups * p.n_part : 0u;
  p.count_blocks = (mark && !kn.grid_in_lds && !p.big) ? (n_obs + 255) / 256 : 0u;
  // the observation grid is built in LDS by the first grid_parts workgroups
  p.nb_grid = mark ? ((kn.grid_in_lds || p.big) ? kn.grid_parts : 1u) : 0u;
  p.nb_slots = (table + 1023) / 1024;
  p.nb_clear = (n_alive + 3) / 4;
  p.nb_cc = mark ? (n_obs * 4 + 255) / 256 : 0;
  // (the removed markings of one update are a tenth of the new generator points: fewer, longer blocks per row)
  p.n_part_un = kn.unmark_parts;
  p.nb_roots = mark ? (n_obs + 255) / 256 : 0;
  p.nb_un = (n_alive && rg.bands) ? rg.rows * p.seg_groups * p.n_part_un : 0u;
  p.nb_walk = n_alive ? 64u : 0u;
  // removePCPtr of the cleared markings rides in the partition launch when there is one, else in the seed launch
  if (mark && kn.unmark_with_groups) { p.nb_un_groups = p.nb_un + p.nb_walk; p.nb_band_groups = p.nb_un; p.nb_un = 0; p.nb_walk = 0; }
  p.nb_commit = mark ? (n_obs + 255) / 256 : 0;
  p.nb_b = mark ? nb_band : 0u;
  p.nb_commit_walk = mark ? 256u : 1u;
  return p;
}

}  // namespace
