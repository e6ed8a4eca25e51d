// submap_bridge.h -- the mcl_3dl side of the sub-maps: what a patched SubMaps calls instead of concatenating clouds,
// building kd-trees and running pcl::NormalEstimation on the host.
//
//   SubMaps::readPoseGraph's loop   (src/sub_maps.cpp:126-156)   -> create(), addKeyframe()
//   SubMaps::warmUpThread           (src/sub_maps.cpp:219-298)   -> warmUp(): the radius search, then the warm-up
//   SubMaps::swapKdTree             (src/sub_maps.cpp:319-342)   -> swapIfReady()
//
// Everything here is a template over the types it is handed (pcl::PointCloud<pcl::PointXYZI>, Eigen::Affine3d,
// geometry_msgs::msg::Pose or pcl::PointXYZ): this header includes neither PCL nor Eigen, so it is compiled and run in a
// plain C++ toolchain (tests/cpp/submap_bridge_test.cpp).  It sits on the context a LocalizationBridge::create has
// prepared: the warm-up is bounded by that call's max_map_points / max_ground_points, and a new create there drops the
// store (every call here then answers DDDMR_ERR_STATE until the next create() and the keyframes are added again).
//
// warmed() is true after a warmUp that returned DDDMR_OK and until swapIfReady() has swapped it in, or a later warmUp
// failed on the device.  A warmUp the library refuses for its arguments (capacity, extent) leaves the earlier one in
// place, here as there.  swapIfReady() is what the measure's lambda calls under the reference's is_warm_up_ready_ test:
// it returns DDDMR_OK and does nothing when no warm-up is waiting.
#ifndef DDDMR_ROLLOUT_ADAPTER_SUBMAP_BRIDGE_H_
#define DDDMR_ROLLOUT_ADAPTER_SUBMAP_BRIDGE_H_

#include <cstdint>
#include <cstring>
#include <vector>

#include "dddmr_rollout.h"

namespace dddmr_rollout_adapter
{

class SubmapBridge
{
public:
  // the pose graph's size and NormalEstimation's setKSearch (sub_maps.cpp:246-252: 20)
  int create(
    dddmr_rollout_ctx * ctx, uint32_t max_keyframes, uint32_t max_store_map_points, uint32_t max_store_ground_points,
    uint32_t normal_k = 20)
  {
    ctx_ = nullptr;
    warmed_ = false;
    n_keyframes_ = 0;
    if (!ctx) {return DDDMR_ERR_BAD_ARG;}
    dddmr_submap_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.max_keyframes = max_keyframes;
    cfg.max_store_map_points = max_store_map_points; cfg.max_store_ground_points = max_store_ground_points;
    cfg.normal_k = normal_k;
    const int rc = dddmr_rollout_submap_create(ctx, &cfg);
    if (rc != DDDMR_OK) {return rc;}
    ctx_ = ctx;                      // only after a successful create
    ids_.resize(max_keyframes);
    return DDDMR_OK;
  }
  bool created() const {return ctx_ != nullptr;}
  bool warmed() const {return ctx_ != nullptr && warmed_;}
  size_t keyframes() const {return n_keyframes_;}

  // One keyframe as readPoseGraph read it: the two clouds BEFORE pcl::transformPointCloud (the library applies
  // trans_m2b), and the pose whose position goes into the pose kd-tree: anything with .x .y .z.
  // Affine: anything with operator()(row, col) (Eigen::Affine3d).
  template<class Cloud, class Affine, class Position>
  int addKeyframe(const Cloud & corner, const Cloud & ground, const Affine & trans_m2b, const Position & position, int32_t * id = nullptr)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    double T[12];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 4; ++c) {T[4 * r + c] = trans_m2b(r, c);}
    }
    const double pos[3] = {(double)position.x, (double)position.y, (double)position.z};
    const size_t nc = corner.points.size(), ng = ground.points.size();
    int32_t got = -1;
    const int rc = dddmr_rollout_submap_add_keyframe(
      ctx_, nc ? &corner.points[0].x : nullptr, nc, nc ? sizeof(corner.points[0]) : 12, ng ? &ground.points[0].x : nullptr, ng,
      ng ? sizeof(ground.points[0]) : 12, T, pos, &got);
    if (rc != DDDMR_OK) {return rc;}
    ++n_keyframes_;
    if (id) {*id = got;}
    return DDDMR_OK;
  }

  // warmUpThread: the keyframes within `radius` (sub_map_search_radius) of the robot's pose, then their warm-up.
  // No keyframe inside the radius: DDDMR_OK, nothing warmed (the reference skips the warm-up then).
  template<class Position>
  int warmUp(const Position & position, double radius, dddmr_submap_stats * stats = nullptr)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    const double pos[3] = {(double)position.x, (double)position.y, (double)position.z};
    size_t n = 0;
    int rc = dddmr_rollout_submap_select(ctx_, pos, radius, ids_.empty() ? nullptr : ids_.data(), ids_.size(), &n);
    if (rc != DDDMR_OK) {return rc;}
    if (stats) {std::memset(stats, 0, sizeof(*stats));}
    if (n == 0) {return DDDMR_OK;}
    rc = dddmr_rollout_submap_warm_up(ctx_, ids_.data(), n, stats);
    if (rc == DDDMR_OK) {
      warmed_ = true;
    } else if (rc == DDDMR_ERR_HIP) {
      warmed_ = false;               // (the device part failed: the earlier warm-up is gone)
    }
    return rc;
  }

  // swapKdTree under is_warm_up_ready_: *swapped (may be NULL) says whether the current map changed
  int swapIfReady(bool * swapped = nullptr)
  {
    if (swapped) {*swapped = false;}
    if (!ctx_) {return DDDMR_ERR_STATE;}
    if (!warmed_) {return DDDMR_OK;}
    const int rc = dddmr_rollout_submap_swap(ctx_);
    warmed_ = false;                 // (swapped in, or refused: either way nothing is waiting any more)
    if (rc == DDDMR_OK && swapped) {*swapped = true;}
    return rc;
  }

private:
  dddmr_rollout_ctx * ctx_ = nullptr;
  bool warmed_ = false;
  size_t n_keyframes_ = 0;
  std::vector<int32_t> ids_;
};

}  // namespace dddmr_rollout_adapter
#endif
