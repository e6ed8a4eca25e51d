// dddmr_rollout.hpp -- C++ host-side mirror of the reference's local-planner
// surface over the C-ABI (include/dddmr_rollout.h).  Header-only, no ROS, no
// HIP types: this is what a C++ caller (the patched Local_Planner, the ROS 2
// adapter of INTEGRATION.md, a unit test) includes.
//
// Names and argument meaning follow the reference:
//   base_trajectory::Trajectory      base_trajectory/include/base_trajectory/trajectory.h:47-126
//   dddmr_sys_core::PlannerState     dddmr_sys_core/include/dddmr_sys_core/dddmr_enum_states.h:46-54
//   Local_Planner::computeVelocityCommand / setPlan
//                                    local_planner/include/local_planner/local_planner.h:72-85
// (paths relative to /root/reference/src/dddmr_local_planner/ or /root/reference/src/).
#ifndef DDDMR_ROLLOUT_HPP_
#define DDDMR_ROLLOUT_HPP_

#include <array>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dddmr_rollout.h"

namespace dddmr_amd {

// dddmr_sys_core::PlannerState (same numeric values)
enum PlannerState {
  TF_FAIL = DDDMR_TF_FAIL,
  PRUNE_PLAN_FAIL = DDDMR_PRUNE_PLAN_FAIL,
  ALL_TRAJECTORIES_FAIL = DDDMR_ALL_TRAJECTORIES_FAIL,
  PERCEPTION_MALFUNCTION = DDDMR_PERCEPTION_MALFUNCTION,
  TRAJECTORY_FOUND = DDDMR_TRAJECTORY_FOUND,
  PATH_BLOCKED_WAIT = DDDMR_PATH_BLOCKED_WAIT,
  PATH_BLOCKED_REPLANNING = DDDMR_PATH_BLOCKED_REPLANNING
};

// The fields every consumer of best_traj reads (p2p_move_base.cpp:338,415,492);
// default-constructed like trajectory.cpp:34-37.
struct Trajectory {
  double xv_ = 0.0, yv_ = 0.0, thetav_ = 0.0;
  double cost_ = -1.0;
  double time_delta_ = 0.0;
  int index_ = -1;  // global sample index of the trajectory (build extension)
};

struct RolloutError : std::runtime_error {
  int code;
  RolloutError(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

// One rollout context = the trajectory generators + critics of one robot
// (Trajectory_Generators_ROS + MPC_Critics_ROS plugin sets of the reference).
class LocalPlanner {
 public:
  LocalPlanner(const std::vector<dddmr_theory_config>& theories, int device = 0,
               uint32_t max_points = 600000, uint32_t max_trajectories = 65536, uint32_t max_steps = 256,
               uint32_t max_plan_poses = 256, int rank = 0, int world_size = 1)
      : theories_(theories) {
    dddmr_rollout_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = DDDMR_ROLLOUT_ABI_VERSION;
    cfg.device = device;
    cfg.rank = rank;
    cfg.world_size = world_size;
    cfg.max_points = max_points;
    cfg.max_trajectories = max_trajectories;
    cfg.max_steps = max_steps;
    cfg.max_plan_poses = max_plan_poses;
    cfg.n_theories = (int32_t)theories_.size();
    cfg.theories = theories_.data();
    const int rc = dddmr_rollout_create(&cfg, &ctx_);
    if (rc != DDDMR_OK) throw RolloutError(rc, "dddmr_rollout_create failed (HIP device + gfx950 build required; no CPU fallback)");
  }
  ~LocalPlanner() { dddmr_rollout_destroy(ctx_); }
  LocalPlanner(const LocalPlanner&) = delete;
  LocalPlanner& operator=(const LocalPlanner&) = delete;

  // aggregate observation (global frame); PCL PointXYZI clouds pass stride 32
  void setCloud(const float* xyzi, size_t n_points, size_t stride_bytes) {
    check(dddmr_rollout_set_cloud(ctx_, xyzi, n_points, stride_bytes));
  }
  // fused local-mode perception feed (MultiLayerSpinningLidar::cbSensor)
  uint32_t setScan(const float* xyz, size_t n_points, size_t stride_bytes, const double T_base_sensor[7],
                   const double T_gbl_base[7], double perception_window_size, double marking_height) {
    uint32_t n_out = 0;
    check(dddmr_rollout_set_scan(ctx_, xyz, n_points, stride_bytes, T_base_sensor, T_gbl_base,
                                 perception_window_size, marking_height, &n_out));
    return n_out;
  }
  // depth camera as one more source of the aggregate (DepthCameraLayer::getObservation in local mode)
  void setDepthSource(int32_t source_id, const dddmr_depth_source_config& cfg) {
    check(dddmr_rollout_set_depth_source(ctx_, source_id, &cfg));
  }
  struct DepthFrameCounts { uint32_t frame, source, aggregate; };
  DepthFrameCounts setDepthFrame(int32_t source_id, const float* xyz, size_t n_points, size_t stride_bytes,
                                 const double T_base_sensor[7], const double T_gbl_base[7], int64_t stamp_ns) {
    DepthFrameCounts c{};
    check(dddmr_rollout_set_depth_frame(ctx_, source_id, xyz, n_points, stride_bytes, T_base_sensor, T_gbl_base, stamp_ns,
                                        &c.frame, &c.source, &c.aggregate));
    return c;
  }
  // depth IMAGE source: the 16UC1 image through DepthImg2PointCloud::cbDepthImg and bufferCloud on the device
  void setDepthImageSource(int32_t source_id, const dddmr_depth_source_config& cfg, const dddmr_depth_image_config& image_cfg) {
    check(dddmr_rollout_set_depth_image_source(ctx_, source_id, &cfg, &image_cfg));
  }
  struct DepthImageCounts { uint32_t camera, frame, source, aggregate; };
  DepthImageCounts setDepthImage(int32_t source_id, const uint16_t* depth_mm, size_t row_stride_bytes,
                                 const double T_base_optical[7], const double T_gbl_base[7], int64_t stamp_ns) {
    DepthImageCounts c{};
    check(dddmr_rollout_set_depth_image(ctx_, source_id, depth_mm, row_stride_bytes, T_base_optical, T_gbl_base, stamp_ns,
                                        &c.camera, &c.frame, &c.source, &c.aggregate));
    return c;
  }
  // the stage-one cloud of the source's latest image, optical frame (the node's point_cloud_from_depth topic)
  std::vector<std::array<float, 3>> getDepthImageCloud(int32_t source_id) {
    size_t n = 0;
    check(dddmr_rollout_get_depth_image_cloud(ctx_, source_id, nullptr, 0, &n));
    std::vector<std::array<float, 3>> out(n);
    if (n) check(dddmr_rollout_get_depth_image_cloud(ctx_, source_id, &out[0][0], n, &n));
    return out;
  }
  // lidar sweep features: the feature half of mcl_feature_node on a sweep source (cfg == nullptr: off); which: 0 sharp,
  // 1 less sharp, 2 flat; x y z ring per point, and optionally the points' indices in the segmented cloud
  void setLidarSweepFeatures(int32_t source_id, const dddmr_lidar_features_config* cfg) {
    check(dddmr_rollout_set_lidar_sweep_features(ctx_, source_id, cfg));
  }
  std::vector<std::array<float, 4>> getLidarSweepFeatures(int32_t source_id, int which, std::vector<uint32_t>* seg_index = nullptr) {
    size_t n = 0;
    check(dddmr_rollout_get_lidar_sweep_features(ctx_, source_id, which, nullptr, nullptr, 0, &n));
    std::vector<std::array<float, 4>> out(n);
    if (seg_index) seg_index->resize(n);
    if (n) check(dddmr_rollout_get_lidar_sweep_features(ctx_, source_id, which, &out[0][0], seg_index ? seg_index->data() : nullptr, n, &n));
    return out;
  }
  struct LidarSweepSegmented {
    std::vector<std::array<float, 3>> xyz;
    std::vector<float> range;
    std::vector<int32_t> col_ind, start_ring_index, end_ring_index;
    std::vector<uint8_t> ground_flag;
  };
  LidarSweepSegmented getLidarSweepSegmented(int32_t source_id, size_t num_vertical_scans) {
    size_t n = 0;
    check(dddmr_rollout_get_lidar_sweep_segmented(ctx_, source_id, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n));
    LidarSweepSegmented s;
    s.xyz.resize(n); s.range.resize(n); s.col_ind.resize(n); s.ground_flag.resize(n);
    s.start_ring_index.resize(num_vertical_scans); s.end_ring_index.resize(num_vertical_scans);
    check(dddmr_rollout_get_lidar_sweep_segmented(ctx_, source_id, n ? &s.xyz[0][0] : nullptr, s.range.data(), s.col_ind.data(),
                                                  s.ground_flag.data(), s.start_ring_index.data(), s.end_ring_index.data(), n, &n));
    return s;
  }
  // the frustum of a depth source (bufferCloud's second half), the two point tests and selfClear's clearing verdicts
  void setDepthFrustum(int32_t source_id, const dddmr_depth_frustum_config& cfg, const double T_gbl_sensor[7]) {
    check(dddmr_rollout_set_depth_frustum(ctx_, source_id, &cfg, T_gbl_sensor));
  }
  struct DepthFrustum { float vertices[8][3], normals[6][3], planes[6][4], origin[3]; };
  DepthFrustum getDepthFrustum(int32_t source_id) {
    DepthFrustum f{};
    check(dddmr_rollout_get_depth_frustum(ctx_, source_id, f.vertices, f.normals, f.planes, f.origin));
    return f;
  }
  // in_frustums / attach: one byte per point (isinFrustumsObservations, isAttachFRUSTUMs)
  void depthFrustumTest(const float* xyz, size_t n, size_t stride_bytes, std::vector<uint8_t>& in_frustums, std::vector<uint8_t>& attach) {
    in_frustums.assign(n, 0);
    attach.assign(n, 0);
    check(dddmr_rollout_depth_frustum_test(ctx_, xyz, n, stride_bytes, in_frustums.data(), attach.data()));
  }
  // verdict[i]: bit 0 kept, bits 1-2 branch (1 outside the frustums, 2 attached, 3 inside); engaged[i]: engagement count
  void depthClearVerdicts(double xy_resolution, double height_resolution, const int32_t* voxel_xyz, const uint32_t* offsets,
                          const float* cluster_xyz, size_t m, std::vector<uint8_t>& verdict, std::vector<uint32_t>& engaged) {
    verdict.assign(m, 0);
    engaged.assign(m, 0);
    check(dddmr_rollout_depth_clear_verdicts(ctx_, xy_resolution, height_resolution, voxel_xyz, offsets, cluster_xyz, m,
                                             verdict.data(), engaged.data()));
  }
  // the depth camera's selfMark: pcl_ground_ / pcl_map_ to the device once, then per update the clusters addPCPtr is
  // to be called with, in the reference's order
  void depthMarkCreate(const dddmr_depth_mark_config& cfg, const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                       const float* map_xyz, size_t n_map, size_t map_stride_bytes) {
    check(dddmr_rollout_depth_mark_create(ctx_, &cfg, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes));
  }
  struct DepthMarkClusters {
    std::vector<float> centroid;      // [c][3]
    std::vector<int32_t> voxel;       // [c][3]
    std::vector<uint32_t> size;       // [c] points before the 0.2 m VoxelGrid
    std::vector<uint32_t> offsets;    // [c + 1] into cluster_xyz
    std::vector<float> cluster_xyz;   // [p][3]
    float plane[4];
    dddmr_depth_mark_stats stats;
  };
  // the library's code (DDDMR_OK or a refusal: the caller then runs its CPU selfMark); buffers sized by a count-only call
  int depthMarkClusters(const double T_gbl_base[7], DepthMarkClusters& out) {
    out.stats = dddmr_depth_mark_stats{};
    int rc = dddmr_rollout_depth_mark_clusters(ctx_, T_gbl_base, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &out.stats);
    if (rc != DDDMR_OK) return rc;
    const size_t c = out.stats.n_accepted, p = out.stats.n_points;
    out.centroid.assign(3 * c + 3, 0.f);
    out.voxel.assign(3 * c + 3, 0);
    out.size.assign(c + 1, 0u);
    out.offsets.assign(c + 1, 0u);
    out.cluster_xyz.assign(3 * p + 3, 0.f);
    rc = dddmr_rollout_depth_mark_clusters(ctx_, T_gbl_base, c, p, out.centroid.data(), out.voxel.data(), out.size.data(),
                                           out.offsets.data(), out.cluster_xyz.data(), out.plane, &out.stats);
    if (rc != DDDMR_OK) return rc;
    out.centroid.resize(3 * c);
    out.voxel.resize(3 * c);
    out.size.resize(c);
    out.cluster_xyz.resize(3 * p);
    return DDDMR_OK;
  }
  // the depth camera layer on the device (store, dGraph, lethal set): the library's codes are returned, not thrown, so
  // that a caller can fall back to its CPU pass
  int depthLayerCreate(const dddmr_depth_layer_config& cfg, const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                       const float* map_xyz, size_t n_map, size_t map_stride_bytes) {
    return dddmr_rollout_depth_layer_create(ctx_, &cfg, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes);
  }
  int depthLayerUpdate(const double T_gbl_base[7], dddmr_depth_layer_stats& stats) {
    stats = dddmr_depth_layer_stats{};
    return dddmr_rollout_depth_layer_update(ctx_, T_gbl_base, &stats);
  }
  int depthLayerReset() { return dddmr_rollout_depth_layer_reset(ctx_); }
  int depthLayerDGraph(std::vector<double>& values, size_t n_ground) {
    values.assign(n_ground + 1, 0.0);
    return dddmr_rollout_depth_layer_get_dgraph(ctx_, values.data(), values.size());
  }
  int depthLayerLethal(std::vector<uint8_t>& flags, size_t n_ground) {
    flags.assign(n_ground + 1, 0);
    return dddmr_rollout_depth_layer_get_lethal(ctx_, flags.data(), flags.size());
  }
  // the alive markings with their stored pc_: voxel [m][3], offsets [m + 1], xyz [p][3]
  int depthLayerClusters(std::vector<int32_t>& voxel, std::vector<uint32_t>& offsets, std::vector<float>& xyz) {
    size_t m = 0, p = 0;
    int rc = dddmr_rollout_depth_layer_get_clusters(ctx_, nullptr, nullptr, nullptr, 0, 0, &m, &p);
    if (rc != DDDMR_OK) return rc;
    voxel.assign(3 * m + 3, 0);
    offsets.assign(m + 1, 0u);
    xyz.assign(3 * p + 3, 0.f);
    rc = dddmr_rollout_depth_layer_get_clusters(ctx_, voxel.data(), offsets.data(), xyz.data(), m, p, &m, &p);
    if (rc != DDDMR_OK) return rc;
    voxel.resize(3 * m);
    xyz.resize(3 * p);
    return DDDMR_OK;
  }
  // the particle filter's lidar likelihood (mcl_3dl's measure() for a batch of particles): the library's codes are
  // returned, not thrown, so that a caller can fall back to its CPU loop
  int mclCreate(const dddmr_mcl_config& cfg) { return dddmr_rollout_mcl_create(ctx_, &cfg); }
  int mclSetMap(const float* map_xyz, size_t n_map, size_t map_stride_bytes, const float* ground_xyz, const float* ground_normals,
                size_t n_ground, size_t ground_stride_bytes, size_t normal_stride_bytes) {
    return dddmr_rollout_mcl_set_map(ctx_, map_xyz, n_map, map_stride_bytes, ground_xyz, ground_normals, n_ground, ground_stride_bytes,
                                     normal_stride_bytes);
  }
  // flat [n][3], less_sharp [n][4], states [n][7] (pos xyz, rot xyzw, raw) -> likelihood and quality per particle
  int mclMeasure(const std::vector<float>& flat_xyz, const std::vector<float>& less_sharp_xyzi, const std::vector<float>& states,
                 std::vector<float>& likelihood, std::vector<float>& quality, dddmr_mcl_stats& stats) {
    const size_t n = states.size() / 7;
    std::vector<float> like(n), qual(n);
    stats = dddmr_mcl_stats{};
    const int rc = dddmr_rollout_mcl_measure(ctx_, flat_xyz.data(), flat_xyz.size() / 3, less_sharp_xyzi.data(), less_sharp_xyzi.size() / 4,
                                             states.data(), n, like.data(), qual.data(), &stats);
    if (rc != DDDMR_OK) return rc;
    likelihood.swap(like);
    quality.swap(qual);
    return DDDMR_OK;
  }
  // the localiser's observation (mcl_3dl's cbLeGoFeatureCloud) prepared on the device, and the measure on it where it lies
  int mclSetObservationConfig(const dddmr_mcl_observation_config* cfg) { return dddmr_rollout_mcl_set_observation_config(ctx_, cfg); }
  int mclPrepare(const float* flat_xyz, size_t n_flat, size_t flat_stride_bytes, const float* less_sharp_xyz, size_t n_less_sharp,
                 size_t less_sharp_stride_bytes, const double T_b2s[12], dddmr_mcl_observation_stats* stats = nullptr) {
    return dddmr_rollout_mcl_prepare(ctx_, flat_xyz, n_flat, flat_stride_bytes, less_sharp_xyz, n_less_sharp, less_sharp_stride_bytes, T_b2s, stats);
  }
  int mclPrepareFromSweep(int32_t source_id, const double T_b2s[12], dddmr_mcl_observation_stats* stats = nullptr) {
    return dddmr_rollout_mcl_prepare_from_sweep(ctx_, source_id, T_b2s, stats);
  }
  int mclMeasurePrepared(const std::vector<float>& states, std::vector<float>& likelihood, std::vector<float>& quality, dddmr_mcl_stats& stats) {
    const size_t n = states.size() / 7;
    std::vector<float> like(n), qual(n);
    stats = dddmr_mcl_stats{};
    const int rc = dddmr_rollout_mcl_measure_prepared(ctx_, states.data(), n, like.data(), qual.data(), &stats);
    if (rc != DDDMR_OK) return rc;
    likelihood.swap(like);
    quality.swap(qual);
    return DDDMR_OK;
  }
  // the localiser's particle set in device memory (mcl_3dl's filter step; every random number is the caller's): states
  // [n][13] in State6DOF::operator[] order, noise4 [n][4], noise rows [*][10]; the library's codes are returned, not thrown
  int mclFilterCreate(const dddmr_mcl_filter_config& cfg) { return dddmr_rollout_mcl_filter_create(ctx_, &cfg); }
  int mclFilterSetParticles(const std::vector<float>& states, const float* probability = nullptr, const float* noise4 = nullptr) {
    return dddmr_rollout_mcl_filter_set_particles(ctx_, states.data(), probability, noise4, states.size() / 13);
  }
  int mclFilterGetParticles(std::vector<float>& states, std::vector<float>& probability, std::vector<float>& bias, std::vector<float>& noise4) {
    size_t n = 0;
    int rc = dddmr_rollout_mcl_filter_get_particles(ctx_, nullptr, nullptr, nullptr, nullptr, 0, &n);
    if (rc != DDDMR_OK) return rc;
    std::vector<float> s(13 * n), p(n), b(n), z(4 * n);
    rc = dddmr_rollout_mcl_filter_get_particles(ctx_, s.data(), p.data(), b.data(), z.data(), n, &n);
    if (rc != DDDMR_OK) return rc;
    states.swap(s); probability.swap(p); bias.swap(b); noise4.swap(z);
    return DDDMR_OK;
  }
  int mclFilterPredict(const float odom_prev[7], const float odom_cur[7], double time_diff) {
    return dddmr_rollout_mcl_filter_predict(ctx_, odom_prev, odom_cur, time_diff);
  }
  int mclFilterSetNoise(const std::vector<float>& noise4) { return dddmr_rollout_mcl_filter_set_noise(ctx_, noise4.data(), noise4.size() / 4); }
  // likelihood empty: the lidar model runs on the resident poses and the prepared observation; state_prev NULL: bias 1
  int mclFilterMeasure(const std::vector<float>& likelihood, const std::vector<float>& quality, const float* state_prev,
                       dddmr_mcl_filter_estimate& estimate, dddmr_mcl_stats* stats = nullptr) {
    return dddmr_rollout_mcl_filter_measure(ctx_, likelihood.empty() ? nullptr : likelihood.data(), quality.empty() ? nullptr : quality.data(),
                                            likelihood.size(), state_prev, &estimate, stats);
  }
  int mclFilterResetInteg() { return dddmr_rollout_mcl_filter_reset_integ(ctx_); }
  int mclFilterResample(double u, const std::vector<float>& noise_rows, dddmr_mcl_filter_resample_stats* stats = nullptr) {
    return dddmr_rollout_mcl_filter_resample(ctx_, u, noise_rows.data(), noise_rows.size() / 10, stats);
  }
  int mclFilterAddNoise(const std::vector<float>& noise_rows) {
    return dddmr_rollout_mcl_filter_add_noise(ctx_, noise_rows.data(), noise_rows.size() / 10);
  }
  // the localiser's sub-maps (mcl_3dl's SubMaps): the keyframes in device memory, the radius search over their poses,
  // the warm-up (concatenation, grids, ground normals) and the swap; the library's codes are returned, not thrown
  int submapCreate(const dddmr_submap_config& cfg) { return dddmr_rollout_submap_create(ctx_, &cfg); }
  int submapAddKeyframe(const float* corner_xyz, size_t n_corner, size_t corner_stride_bytes, const float* ground_xyz, size_t n_ground,
                        size_t ground_stride_bytes, const double T_map_base[12], const double position[3], int32_t* id_out = nullptr) {
    return dddmr_rollout_submap_add_keyframe(ctx_, corner_xyz, n_corner, corner_stride_bytes, ground_xyz, n_ground, ground_stride_bytes, T_map_base,
                                             position, id_out);
  }
  int submapSelect(const double position[3], double radius, std::vector<int32_t>& ids) {
    size_t n = 0;
    int rc = dddmr_rollout_submap_select(ctx_, position, radius, nullptr, 0, &n);
    if (rc != DDDMR_OK) return rc;
    std::vector<int32_t> out(n);
    if (n) rc = dddmr_rollout_submap_select(ctx_, position, radius, out.data(), out.size(), &n);
    if (rc != DDDMR_OK) return rc;
    out.resize(n);
    ids.swap(out);
    return DDDMR_OK;
  }
  int submapWarmUp(const std::vector<int32_t>& ids, dddmr_submap_stats* stats = nullptr) {
    return dddmr_rollout_submap_warm_up(ctx_, ids.data(), ids.size(), stats);
  }
  int submapSwap() { return dddmr_rollout_submap_swap(ctx_); }
  // the static layer and the no-entry layer (static_layer.cpp:201-285, :390-415; no_entry_layer.cpp:265-283): sGraph as
  // CSR rows, the two dGraphs and their binding to the stack's host slots; the library's codes are returned, not thrown
  int staticLayerCreate(const dddmr_static_layer_config& cfg) { return dddmr_rollout_static_layer_create(ctx_, &cfg); }
  int staticLayerBuild(const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes, const float* map_xyz, size_t n_map,
                       size_t map_stride_bytes, dddmr_static_layer_stats* stats = nullptr) {
    return dddmr_rollout_static_layer_build(ctx_, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes, stats);
  }
  // row_start must hold n_ground + 1 entries on entry (the build's stats say how many nodes there are)
  int staticLayerGraph(std::vector<uint32_t>& row_start, std::vector<uint32_t>& neighbour, std::vector<float>& weight) {
    size_t n = 0;
    int rc = dddmr_rollout_static_layer_get_graph(ctx_, nullptr, nullptr, nullptr, 0, &n);
    if (rc != DDDMR_OK) return rc;
    std::vector<uint32_t> nb(n);
    std::vector<float> w(n);
    rc = dddmr_rollout_static_layer_get_graph(ctx_, row_start.data(), n ? nb.data() : nullptr, n ? w.data() : nullptr, n, &n);
    if (rc != DDDMR_OK) return rc;
    neighbour.swap(nb);
    weight.swap(w);
    return DDDMR_OK;
  }
  int staticLayerDGraph(std::vector<double>& values) { return dddmr_rollout_static_layer_get_dgraph(ctx_, values.data(), values.size()); }
  int staticLayerSetZones(const float* zone_xyz, size_t n_points, size_t stride_bytes, double inflation_distance,
                          dddmr_static_layer_stats* stats = nullptr) {
    return dddmr_rollout_static_layer_set_zones(ctx_, zone_xyz, n_points, stride_bytes, inflation_distance, stats);
  }
  int staticLayerZoneDGraph(std::vector<double>& values) { return dddmr_rollout_static_layer_get_zone_dgraph(ctx_, values.data(), values.size()); }
  int staticLayerBind(int32_t which /* 0 static, 1 no-entry */, int32_t slot) { return dddmr_rollout_static_layer_bind(ctx_, which, slot); }
  // the pre-graph global planner on the device graph (a_star_on_pre_graph.cpp:191-289; global_planner.cpp:407, :451;
  // dynamic_window_aware_global_planner.cpp:248-270); the library's codes are returned, not thrown
  int globalPlanCreate(const dddmr_global_plan_config& cfg) { return dddmr_rollout_global_plan_create(ctx_, &cfg); }
  int globalPlanSetNodeWeights(const std::vector<float>& w) { return dddmr_rollout_global_plan_set_node_weights(ctx_, w.empty() ? nullptr : w.data(), w.size()); }
  // xyz: n points of 3 floats
  int globalPlanNearest(const std::vector<float>& xyz, std::vector<uint32_t>& ids) {
    ids.assign(xyz.size() / 3, 0xFFFFFFFFu);
    return dddmr_rollout_global_plan_nearest(ctx_, xyz.data(), ids.size(), ids.data());
  }
  int globalPlanProbe(const std::vector<float>& xyz, std::vector<uint32_t>& n_ground_near, std::vector<uint8_t>& blocked) {
    n_ground_near.assign(xyz.size() / 3, 0u);
    blocked.assign(xyz.size() / 3, 0);
    return dddmr_rollout_global_plan_probe(ctx_, xyz.data(), n_ground_near.size(), n_ground_near.data(), blocked.data());
  }
  // path must have room for the paths of all queries (at most n_ground nodes each); results: one per query
  int globalPlanPlan(const std::vector<uint32_t>& start, const std::vector<uint32_t>& goal, std::vector<uint32_t>& path,
                     std::vector<dddmr_global_plan_result>& results) {
    if (start.size() != goal.size()) return DDDMR_ERR_BAD_ARG;
    results.assign(start.size(), dddmr_global_plan_result{});
    return dddmr_rollout_global_plan_plan(ctx_, start.data(), goal.data(), start.size(), path.data(), path.size(), results.data());
  }
  // prune plan poses, x y z qx qy qz qw each (output of Local_Planner::prunePlan)
  void setPlan(const double* poses_xyz_qxyzw, size_t n_poses) {
    check(dddmr_rollout_set_prune_plan(ctx_, poses_xyz_qxyzw, n_poses));
  }

  // Local_Planner::computeVelocityCommand(traj_gen_name, best_traj), the section
  // local_planner.cpp:535-587 (the caller keeps the TF / prune-plan / perception
  // guards and the perception opinions around it).
  PlannerState computeVelocityCommand(const std::string& traj_gen_name, Trajectory& best_traj,
                                      const dddmr_tick_input& in) {
    check(dddmr_rollout_tick(ctx_, traj_gen_name.c_str(), &in, &last_));
    best_traj.xv_ = last_.vx;
    best_traj.yv_ = last_.vy;
    best_traj.thetav_ = last_.wz;
    best_traj.cost_ = last_.best_cost;
    best_traj.index_ = last_.best_index;
    return static_cast<PlannerState>(last_.planner_state);
  }

  // cbSensor's stitcher_num (multilayer_spinning_lidar.cpp:185-200): later setScan() calls feed the last n raw scans
  void setStitcher(int stitcher_num) { check(dddmr_rollout_set_stitcher(ctx_, stitcher_num)); }

  // the theory's initialise() alone: the (vx, vy, wz) sample list a tick with these inputs rolls out
  std::vector<std::array<float, 3>> samples(const std::string& traj_gen_name, const dddmr_tick_input& in) {
    size_t n = 0;
    check(dddmr_rollout_samples(ctx_, traj_gen_name.c_str(), &in, nullptr, 0, &n));
    std::vector<std::array<float, 3>> out(n);
    if (n) check(dddmr_rollout_samples(ctx_, traj_gen_name.c_str(), &in, &out[0][0], n, &n));
    return out;
  }

  // ---- multi-rank hosts (one context per GPU, created with rank / world_size) ----
  const dddmr_rollout_result& lastResult() const { return last_; }
  // (a) in-library exchange: RCCL communicator owned by the context; afterwards every tick returns the GLOBAL winner
  static std::array<uint8_t, DDDMR_COMM_ID_BYTES> commUniqueId() {
    std::array<uint8_t, DDDMR_COMM_ID_BYTES> id{};
    const int rc = dddmr_rollout_comm_unique_id(id.data());
    if (rc != DDDMR_OK) throw RolloutError(rc, "dddmr_rollout_comm_unique_id failed (librccl not loadable?)");
    return id;
  }
  void commInit(const std::array<uint8_t, DDDMR_COMM_ID_BYTES>& id, int rank, int n_ranks) {
    check(dddmr_rollout_comm_init(ctx_, id.data(), rank, n_ranks));
  }
  void commDestroy() { check(dddmr_rollout_comm_destroy(ctx_)); }
  int commRanks() {
    int32_t n = 0;
    check(dddmr_rollout_comm_ranks(ctx_, &n));
    return n;
  }
  // (b) host-side exchange: min-all-reduce a 2 * n_ranks int64 vector holding every rank's winnerWords() in its
  // slots (INT64_MAX elsewhere), then resolveWords() on every rank -- exact; or the 8-byte key + resolve()
  std::array<int64_t, 2> winnerWords() const {
    std::array<int64_t, 2> w{};
    dddmr_rollout_winner_words(&last_, w.data());
    return w;
  }
  dddmr_rollout_result resolveWords(const std::vector<int64_t>& slots) {
    dddmr_rollout_result r = last_;
    check(dddmr_rollout_resolve_words(ctx_, slots.data(), (int32_t)(slots.size() / 2), &r));
    return r;
  }
  dddmr_rollout_result resolve(int64_t reduced_key) {
    dddmr_rollout_result r = last_;
    check(dddmr_rollout_resolve(ctx_, reduced_key, &r));
    return r;
  }

  // ---- global-mode marking / clearing layer of the lidar plugin (multilayer_spinning_lidar.cpp:306-746) ----
  void markingCreate(const dddmr_marking_config& cfg, const float* ground_xyz, size_t n_ground, size_t ground_stride,
                     const float* map_xyz, size_t n_map, size_t map_stride) {
    check(dddmr_rollout_marking_create(ctx_, &cfg, ground_xyz, n_ground, ground_stride, map_xyz, n_map, map_stride));
    n_ground_ = n_ground;
  }
  // one doClear_then_Mark pass on the current aggregate observation (setScan / setCloud)
  dddmr_marking_stats markingUpdate(const double T_base_sensor[7], const double T_gbl_base[7]) {
    dddmr_marking_stats st{};
    check(dddmr_rollout_marking_update(ctx_, T_base_sensor, T_gbl_base, &st));
    return st;
  }
  void markingReset() { check(dddmr_rollout_marking_reset(ctx_)); }
  std::vector<double> dGraph() {                        // get_dGraphValue(index) for index 0..n_ground
    std::vector<double> v(n_ground_ + 1);
    check(dddmr_rollout_marking_get_dgraph(ctx_, v.data(), v.size()));
    return v;
  }
  std::vector<uint8_t> lethal() {                       // lethal_map_ keys as flags
    std::vector<uint8_t> v(n_ground_ + 1);
    check(dddmr_rollout_marking_get_lethal(ctx_, v.data(), v.size()));
    return v;
  }
  std::vector<std::array<int32_t, 3>> markedVoxels() {  // alive markings (the global_marking topic's keys)
    size_t n = 0;
    check(dddmr_rollout_marking_get_voxels(ctx_, nullptr, 0, &n));
    std::vector<std::array<int32_t, 3>> v(n);
    if (n) check(dddmr_rollout_marking_get_voxels(ctx_, &v[0][0], n, &n));
    return v;
  }

  // best trajectory poses for the "best_trajectory" debug topic
  std::vector<std::array<double, 7>> bestPoses() {
    size_t n = 0;
    check(dddmr_rollout_get_best_poses(ctx_, nullptr, 0, &n));
    std::vector<std::array<double, 7>> poses(n);
    if (n) check(dddmr_rollout_get_best_poses(ctx_, &poses[0][0], n, &n));
    return poses;
  }

  // `trajectory` (accepted_only = false) / `accepted_trajectory` debug pose arrays
  std::vector<std::array<double, 7>> poseArrays(bool accepted_only) {
    size_t n = 0;
    check(dddmr_rollout_get_pose_arrays(ctx_, accepted_only ? 1 : 0, nullptr, 0, &n));
    std::vector<std::array<double, 7>> poses(n);
    if (n) check(dddmr_rollout_get_pose_arrays(ctx_, accepted_only ? 1 : 0, &poses[0][0], n, &n));
    return poses;
  }

  // PathBlockedStrategy::selfMark (path_blocked_strategy.cpp:56-100) on the current
  // aggregate observation; pcl_prune_plan: x y z intensity records as prunePlan fills
  // them (local_planner.cpp:402-430).  Returns prune_plan_blocked_ratio_ (percent).
  double pathBlockedRatio(const float* pcl_prune_plan_xyzi, size_t n_points, double check_radius,
                          dddmr_perception_opinion* opinion = nullptr) {
    double ratio = 0.0;
    int32_t op = DDDMR_OPINION_PASS;
    check(dddmr_rollout_path_blocked(ctx_, pcl_prune_plan_xyzi, n_points, check_radius, &ratio, &op, nullptr));
    if (opinion) *opinion = static_cast<dddmr_perception_opinion>(op);
    return ratio;
  }

 private:
  void check(int rc) {
    if (rc != DDDMR_OK) throw RolloutError(rc, dddmr_rollout_last_error(ctx_));
  }
  std::vector<dddmr_theory_config> theories_;
  dddmr_rollout_ctx* ctx_ = nullptr;
  dddmr_rollout_result last_{};
  size_t n_ground_ = 0;
};

}  // namespace dddmr_amd
#endif
