// localization_bridge.h -- the mcl_3dl side of the boundary: what a patched MCL3dlNode::measure calls instead of
// handing LidarMeasurementModelLikelihood::measure to pf_->measure one particle at a time.
//
//   LidarMeasurementModelLikelihood::loadConfig   (src/lidar_measurement_model_likelihood.cpp:36-69)  -> create()
//   SubMaps::swapKdTree                           (called from the lambda at src/mcl_3dl.cpp:487-489) -> setMap()
//   pf_->measure(measure_func)                    (src/mcl_3dl.cpp:476-503, include/mcl_3dl/pf.h:247-262) -> measure()
//   MCL3dlNode::cbLeGoFeatureCloud                (src/mcl_3dl.cpp:263-464) -> configureObservation(), prepareObservation()
//   ... and the measure on what it prepared       -> measurePrepared()
//
// Everything here is a template over the types it is handed (pcl::PointCloud<pcl::PointXYZI>, pcl::PointCloud<pcl::Normal>,
// mcl_3dl::State6DOF): this header includes neither PCL nor the filter, so it is compiled and run in a plain C++
// toolchain (tests/cpp/localization_bridge_test.cpp, tests/cpp/mcl_observation_bridge_test.cpp).  The filter keeps
// everything else: prediction, bias, resampling, the normalisation of the weights and sub-map loading.
//
// ready() is true only after a create AND a setMap that both returned DDDMR_OK, and goes false again on any failure of
// either (the device would answer from parameters or a map the filter no longer uses).  A failing measure() leaves the
// outputs alone and ready() as it was: the caller runs the CPU loop for that observation.
//
// prepared() is true only after a configureObservation AND a prepareObservation that both returned DDDMR_OK.  A failing
// prepareObservation clears it: the library still holds the previous sweep's observation, which is no longer the
// filter's, so the patched cbLeGoFeatureCloud runs its own code for that sweep and measure() takes its clouds.
#ifndef DDDMR_ROLLOUT_ADAPTER_LOCALIZATION_BRIDGE_H_
#define DDDMR_ROLLOUT_ADAPTER_LOCALIZATION_BRIDGE_H_

#include <cstdint>
#include <cstring>
#include <vector>

#include "dddmr_rollout.h"

namespace dddmr_rollout_adapter
{

class LocalizationBridge
{
public:
  // the likelihood.* parameters as loadConfig read them; capacities for the largest particle count the filter reaches
  // (global localisation, expansion resetting) and the largest sub-map
  int create(
    dddmr_rollout_ctx * ctx, double match_dist_min, double match_dist_flat, double radius_of_ground_search,
    int threshold_for_trusted_ground, uint32_t max_map_points, uint32_t max_ground_points, uint32_t max_particles,
    uint32_t max_observation_points = 2000, uint32_t max_ground_neighbours = 1024)
  {
    ctx_ = nullptr;
    have_map_ = false;
    have_obs_cfg_ = have_obs_ = false;           // (a create forgets the observation's configuration)
    if (!ctx) {return DDDMR_ERR_BAD_ARG;}
    dddmr_mcl_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.match_dist_min = match_dist_min; cfg.match_dist_flat = match_dist_flat;
    cfg.radius_of_ground_search = radius_of_ground_search;
    cfg.threshold_for_trusted_ground = threshold_for_trusted_ground;
    cfg.max_map_points = max_map_points; cfg.max_ground_points = max_ground_points;
    cfg.max_particles = max_particles; cfg.max_observation_points = max_observation_points;
    cfg.max_ground_neighbours = max_ground_neighbours;
    const int rc = dddmr_rollout_mcl_create(ctx, &cfg);
    if (rc != DDDMR_OK) {return rc;}
    ctx_ = ctx;                      // only after a successful create
    return DDDMR_OK;
  }
  bool ready() const {return ctx_ != nullptr && have_map_;}

  // swapKdTree: the clouds kdtree_map_current_ / kdtree_ground_current_ were built over, and normals_ground_current_
  template<class MapCloud, class GroundCloud, class NormalCloud>
  int setMap(const MapCloud & map, const GroundCloud & ground, const NormalCloud & normals)
  {
    have_map_ = false;
    if (!ctx_) {return DDDMR_ERR_STATE;}
    const size_t nm = map.points.size(), ng = ground.points.size();
    if (normals.points.size() != ng) {return DDDMR_ERR_BAD_ARG;}
    std::vector<float> nrm(3 * ng);
    for (size_t i = 0; i < ng; ++i) {
      nrm[3 * i] = normals.points[i].normal_x; nrm[3 * i + 1] = normals.points[i].normal_y; nrm[3 * i + 2] = normals.points[i].normal_z;
    }
    const int rc = dddmr_rollout_mcl_set_map(
      ctx_, nm ? &map.points[0].x : nullptr, nm, nm ? sizeof(map.points[0]) : 12, ng ? &ground.points[0].x : nullptr,
      ng ? nrm.data() : nullptr, ng, ng ? sizeof(ground.points[0]) : 12, 12);
    have_map_ = rc == DDDMR_OK;
    return rc;
  }
  // ... or the map came from the device's own sub-maps (submap_bridge.h): call this after a SubmapBridge::swapIfReady
  // that reported a swap, in place of setMap
  void mapSwappedIn() {have_map_ = ctx_ != nullptr;}

  // One observation against every particle: likelihood[i] and quality[i] belong to particles[i] (what measure_func
  // returns for it, and the result's quality).  quality_min / quality_max: match_ratio_min / match_ratio_max of
  // mcl_3dl.cpp:476-498.  State: anything with pos_.x_ .. rot_.w_ (mcl_3dl::State6DOF, or the filter's Particle::state_
  // copied out).  DDDMR_OK or the library's code; on any other code the outputs are untouched.
  template<class Cloud, class State>
  int measure(
    const Cloud & flat, const Cloud & less_sharp, const std::vector<State> & particles, std::vector<float> & likelihood,
    std::vector<float> & quality, float * quality_min = nullptr, float * quality_max = nullptr,
    dddmr_mcl_stats * stats = nullptr)
  {
    if (!ready()) {return DDDMR_ERR_STATE;}
    const size_t nf = flat.points.size(), nl = less_sharp.points.size(), n = particles.size();
    xyz_.resize(3 * nf);
    for (size_t i = 0; i < nf; ++i) {
      xyz_[3 * i] = flat.points[i].x; xyz_[3 * i + 1] = flat.points[i].y; xyz_[3 * i + 2] = flat.points[i].z;
    }
    xyzi_.resize(4 * nl);
    for (size_t i = 0; i < nl; ++i) {
      const auto & p = less_sharp.points[i];
      xyzi_[4 * i] = p.x; xyzi_[4 * i + 1] = p.y; xyzi_[4 * i + 2] = p.z; xyzi_[4 * i + 3] = p.intensity;
    }
    packStates(particles);
    like_.assign(n, 0.f);
    qual_.assign(n, 0.f);
    dddmr_mcl_stats local;
    dddmr_mcl_stats * st = stats ? stats : &local;
    const int rc = dddmr_rollout_mcl_measure(
      ctx_, nf ? xyz_.data() : nullptr, nf, nl ? xyzi_.data() : nullptr, nl, n ? states_.data() : nullptr, n,
      n ? like_.data() : nullptr, n ? qual_.data() : nullptr, st);
    if (rc != DDDMR_OK) {return rc;}
    likelihood.swap(like_);
    quality.swap(qual_);
    if (quality_min) {*quality_min = st->quality_min;}
    if (quality_max) {*quality_max = st->quality_max;}
    return DDDMR_OK;
  }

  // ---- the observation: cbLeGoFeatureCloud on the device ------------------------------------------------------------
  // params_->euc_cluster_distance_ / euc_cluster_min_size_ and the largest lists a sweep yields (their sum at most
  // create()'s max_observation_points)
  int configureObservation(
    double euc_cluster_distance, int euc_cluster_min_size, uint32_t max_flat_points, uint32_t max_less_sharp_points)
  {
    have_obs_cfg_ = have_obs_ = false;
    if (!ctx_) {return DDDMR_ERR_STATE;}
    dddmr_mcl_observation_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.euc_cluster_distance = euc_cluster_distance;
    cfg.euc_cluster_min_size = euc_cluster_min_size;
    cfg.max_flat_points = max_flat_points; cfg.max_less_sharp_points = max_less_sharp_points;
    const int rc = dddmr_rollout_mcl_set_observation_config(ctx_, &cfg);
    have_obs_cfg_ = rc == DDDMR_OK;
    return rc;
  }
  bool prepared() const {return ready() && have_obs_;}

  // The two message clouds as pcl::fromROSMsg left them (BEFORE the transform: the library applies it) and
  // trans_b2s_af3: anything with operator()(row, col) (Eigen::Affine3d).
  template<class Cloud, class Affine>
  int prepareObservation(
    const Cloud & flat, const Cloud & less_sharp, const Affine & trans_b2s, dddmr_mcl_observation_stats * stats = nullptr)
  {
    have_obs_ = false;
    if (!ctx_ || !have_obs_cfg_) {return DDDMR_ERR_STATE;}
    double T[12];
    pack(trans_b2s, T);
    const size_t nf = flat.points.size(), nl = less_sharp.points.size();
    const int rc = dddmr_rollout_mcl_prepare(
      ctx_, nf ? &flat.points[0].x : nullptr, nf, nf ? sizeof(flat.points[0]) : 12, nl ? &less_sharp.points[0].x : nullptr, nl,
      nl ? sizeof(less_sharp.points[0]) : 12, T, stats);
    have_obs_ = rc == DDDMR_OK;
    return rc;
  }
  // ... or the current features of a sweep source of the same context (dddmr_rollout_set_lidar_sweep with features
  // on): nothing crosses the bus
  template<class Affine>
  int prepareObservation(int32_t sweep_source_id, const Affine & trans_b2s, dddmr_mcl_observation_stats * stats = nullptr)
  {
    have_obs_ = false;
    if (!ctx_ || !have_obs_cfg_) {return DDDMR_ERR_STATE;}
    double T[12];
    pack(trans_b2s, T);
    const int rc = dddmr_rollout_mcl_prepare_from_sweep(ctx_, sweep_source_id, T, stats);
    have_obs_ = rc == DDDMR_OK;
    return rc;
  }

  // measure() on the prepared observation, which stays where it is; the same outputs and the same rules
  template<class State>
  int measurePrepared(
    const std::vector<State> & particles, std::vector<float> & likelihood, std::vector<float> & quality,
    float * quality_min = nullptr, float * quality_max = nullptr, dddmr_mcl_stats * stats = nullptr)
  {
    if (!prepared()) {return DDDMR_ERR_STATE;}
    const size_t n = particles.size();
    packStates(particles);
    like_.assign(n, 0.f);
    qual_.assign(n, 0.f);
    dddmr_mcl_stats local;
    dddmr_mcl_stats * st = stats ? stats : &local;
    const int rc = dddmr_rollout_mcl_measure_prepared(
      ctx_, n ? states_.data() : nullptr, n, n ? like_.data() : nullptr, n ? qual_.data() : nullptr, st);
    if (rc != DDDMR_OK) {return rc;}
    likelihood.swap(like_);
    quality.swap(qual_);
    if (quality_min) {*quality_min = st->quality_min;}
    if (quality_max) {*quality_max = st->quality_max;}
    return DDDMR_OK;
  }

private:
  template<class Affine>
  static void pack(const Affine & t, double T[12])
  {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 4; ++c) {T[4 * r + c] = t(r, c);}
    }
  }
  template<class State>
  void packStates(const std::vector<State> & particles)
  {
    const size_t n = particles.size();
    states_.resize(7 * n);
    for (size_t i = 0; i < n; ++i) {
      const State & s = particles[i];
      float * o = &states_[7 * i];
      o[0] = s.pos_.x_; o[1] = s.pos_.y_; o[2] = s.pos_.z_;
      o[3] = s.rot_.x_; o[4] = s.rot_.y_; o[5] = s.rot_.z_; o[6] = s.rot_.w_;
    }
  }

  dddmr_rollout_ctx * ctx_ = nullptr;
  bool have_map_ = false;
  bool have_obs_cfg_ = false, have_obs_ = false;
  std::vector<float> xyz_, xyzi_, states_, like_, qual_;
};

}  // namespace dddmr_rollout_adapter
#endif
