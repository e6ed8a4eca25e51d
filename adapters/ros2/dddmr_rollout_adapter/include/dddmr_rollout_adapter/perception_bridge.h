// perception_bridge.h -- the perception_3d side of the boundary: what the patches under
// adapters/ros2/patches/ call from the reference's sensor plugins.
//
//   MultiLayerSpinningLidar::cbSensor, local mode   (plugins/multilayer_spinning_lidar.cpp:177-281)  -> feedScan()
//   ... selfClear + selfMark, global mode           (:306-628; StackedPerception::doClear_then_Mark,
//                                                    src/stacked_perception.cpp:72-90)               -> MarkingLayerBridge
//   ... get_dGraphValue / updateLethalPointCloud    (:838-841, :283-304)                             -> MarkingLayerBridge
//   ImageProjection::cloudHandler's front half + cbSensor
//                          (dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp:280-314, :582-592) -> feedSweep(), sweepCloud()
//   mcl_feature_node's laser_cloud_sharp / _less_sharp / _flat
//                          (lego_loam_bor/src/featureAssociation.cpp:318-491, :1384-1405)             -> sweepFeatures()
//   the feature node's segmented_cloud_info orientation, its four clouds with point times and outlier_cloud
//                          (imageProjection.cpp:391-406, :548-558; featureAssociation.cpp:281-314, :486-514) -> sweepAssociation()
//   PathBlockedStrategy::selfMark                   (plugins/path_blocked_strategy.cpp:56-100)       -> pathBlocked()
//   DepthCameraObservationBuffer::bufferCloud, local mode
//                                    (plugins/depth_camera/depth_camera_observation_buffer.cpp:78-187) -> feedDepthFrame()
//   DepthImg2PointCloud::cbDepthImg + bufferCloud   (utils/depthimg2pointcloud_node.cpp:96-157)      -> feedDepthImage()
//   ... bufferCloud's frustum                       (depth_camera_observation_buffer.cpp:134-174)    -> feedDepthFrustum()
//   DepthCameraLayer::selfClear's decision tree     (plugins/depth_camera/depth_camera_layer.cpp:324-422) -> depthClearVerdicts()
//   DepthCameraLayer::selfMark from the aggregate on (:487-601)                                        -> depthMarkCreate(), depthMarkClusters()
//   DepthCameraLayer::selfClear + selfMark + updateLethalPointCloud with the store on the device      -> DepthLayerBridge
//
// Everything here is a template over the ROS / PCL types it is handed (geometry_msgs TransformStamped,
// pcl::PointCloud<...>): this header includes neither, so it is syntax-checked in a plain C++ toolchain
// (tests/test_adapters_cpu.py) and instantiated with the real types inside a dddmr_navigation workspace.
#ifndef DDDMR_ROLLOUT_ADAPTER_PERCEPTION_BRIDGE_H_
#define DDDMR_ROLLOUT_ADAPTER_PERCEPTION_BRIDGE_H_

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dddmr_rollout.h"
#include "dddmr_rollout_adapter/shared_context.h"

namespace dddmr_rollout_adapter
{

// geometry_msgs::msg::TransformStamped -> x y z qx qy qz qw
template<class TransformStamped>
inline void toPose7(const TransformStamped & t, double out[7])
{
  out[0] = t.transform.translation.x; out[1] = t.transform.translation.y; out[2] = t.transform.translation.z;
  out[3] = t.transform.rotation.x; out[4] = t.transform.rotation.y; out[5] = t.transform.rotation.z;
  out[6] = t.transform.rotation.w;
}

// cbSensor, is_local_planner_ = true: the raw scan in the SENSOR frame (pcl::fromROSMsg output, before any of the
// reference's transforms / PassThrough / VoxelGrid passes) goes to the device, which does all of them and keeps
// the result as the aggregate observation.  Returns the library's code; on DDDMR_OK the caller skips the CPU
// passes of this callback and SharedContext::noteDeviceFeed() tells the planner not to upload a CPU aggregate.
template<class Cloud, class TransformStamped>
inline int feedScan(
  dddmr_rollout_ctx * ctx, const Cloud & scan_sensor_frame, const TransformStamped & trans_b2s,
  const TransformStamped & trans_gbl2b, double perception_window_size, double marking_height, int stitcher_num,
  uint32_t * n_out = nullptr)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  double b2s[7], g2b[7];
  toPose7(trans_b2s, b2s);
  toPose7(trans_gbl2b, g2b);
  int rc = dddmr_rollout_set_stitcher(ctx, stitcher_num > 0 ? stitcher_num : 0);    // (the library keeps the deque of raw scans)
  if (rc != DDDMR_OK) {return rc;}
  const size_t n = scan_sensor_frame.points.size();
  rc = dddmr_rollout_set_scan(
    ctx, n ? &scan_sensor_frame.points[0].x : nullptr, n, sizeof(scan_sensor_frame.points[0]), b2s, g2b,
    perception_window_size, marking_height, n_out);
  if (rc == DDDMR_OK) {SharedContext::noteDeviceFeed();}
  return rc;
}

// The same for plugin number `source` of several sensor plugins (its position in perception_3d's `plugins:` list,
// 0 .. DDDMR_MAX_SOURCES - 1): the device keeps one feed per source and publishes their concatenation in source order,
// which is StackedPerception::aggregateObservations (src/stacked_perception.cpp:128-140).
template<class Cloud, class TransformStamped>
inline int feedScanSource(
  dddmr_rollout_ctx * ctx, int source, const Cloud & scan_sensor_frame, const TransformStamped & trans_b2s,
  const TransformStamped & trans_gbl2b, double perception_window_size, double marking_height, int stitcher_num,
  uint32_t * n_source_out = nullptr, uint32_t * n_aggregate_out = nullptr)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  double b2s[7], g2b[7];
  toPose7(trans_b2s, b2s);
  toPose7(trans_gbl2b, g2b);
  int rc = dddmr_rollout_set_stitcher_source(ctx, source, stitcher_num > 0 ? stitcher_num : 0);
  if (rc != DDDMR_OK) {return rc;}
  const size_t n = scan_sensor_frame.points.size();
  rc = dddmr_rollout_set_scan_source(
    ctx, source, n ? &scan_sensor_frame.points[0].x : nullptr, n, sizeof(scan_sensor_frame.points[0]), b2s, g2b,
    perception_window_size, marking_height, n_source_out, n_aggregate_out);
  if (rc == DDDMR_OK) {SharedContext::noteDeviceFeed();}
  return rc;
}

// ImageProjection::cloudHandler's front half and cbSensor in one call: the RAW sweep in the lidar's own frame
// (pcl::fromROSMsg output of the lidar topic, before the node's pitch removal) goes to lidar sweep source `source`,
// configured with dddmr_rollout_set_lidar_sweep_source from the node's laser.* / imageProjection.* parameters and the
// mount pitch.  The plugin's `topic` then names the raw lidar instead of segmented_cloud_pure.  trans_b2s takes the
// frame "<sensor>_pitch_removed" (the frame the node stamps its clouds with) to the base frame.  There is no stitcher
// on sweep sources.  Returns the library's code and notes a device feed on DDDMR_OK only; on any other code nothing on
// the device has changed and the caller runs its CPU path for this sweep.
template<class Cloud, class TransformStamped>
inline int feedSweep(
  dddmr_rollout_ctx * ctx, int source, const Cloud & sweep_sensor_frame, const TransformStamped & trans_b2s,
  const TransformStamped & trans_gbl2b, double perception_window_size, double marking_height,
  uint32_t * n_segmented_out = nullptr, uint32_t * n_source_out = nullptr, uint32_t * n_aggregate_out = nullptr)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  double b2s[7], g2b[7];
  toPose7(trans_b2s, b2s);
  toPose7(trans_gbl2b, g2b);
  const size_t n = sweep_sensor_frame.points.size();
  const int rc = dddmr_rollout_set_lidar_sweep(
    ctx, source, n ? &sweep_sensor_frame.points[0].x : nullptr, n, sizeof(sweep_sensor_frame.points[0]), b2s, g2b,
    perception_window_size, marking_height, n_segmented_out, n_source_out, n_aggregate_out);
  if (rc == DDDMR_OK) {SharedContext::noteDeviceFeed();}
  return rc;
}

// What the node would have published on segmented_cloud_pure for the source's latest accepted sweep, for a caller
// that still wants the topic: points in raster order, the segment's label in `intensity` (pcl::PointXYZI).
template<class Cloud>
inline int sweepCloud(dddmr_rollout_ctx * ctx, int source, Cloud & out)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  size_t n = 0;
  int rc = dddmr_rollout_get_lidar_sweep_cloud(ctx, source, nullptr, 0, &n);
  if (rc != DDDMR_OK) {return rc;}
  std::vector<float> xyzl(4 * n);
  if (n) {
    rc = dddmr_rollout_get_lidar_sweep_cloud(ctx, source, xyzl.data(), n, &n);
    if (rc != DDDMR_OK) {return rc;}
  }
  out.points.resize(n);
  for (size_t i = 0; i < n; ++i) {
    out.points[i].x = xyzl[4 * i + 0];
    out.points[i].y = xyzl[4 * i + 1];
    out.points[i].z = xyzl[4 * i + 2];
    out.points[i].intensity = xyzl[4 * i + 3];
  }
  return DDDMR_OK;
}

// What mcl_feature_node would have published on laser_cloud_sharp (which = 0), laser_cloud_less_sharp (1) or
// laser_cloud_flat (2) for the source's latest accepted sweep, once dddmr_rollout_set_lidar_sweep_features has switched
// the features on: points in the reference's push order, the ring in `intensity` (mcl_3dl's cbLeGoFeatureCloud takes
// flat and less sharp).  The config's T_out is publishCloud's trans_c2s.inverse() as a row-major 3 x 4; with Eigen:
//   Eigen::Affine3d T = tf2::transformToEigen(trans_c2s).inverse();
//   for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) cfg.T_out[4 * r + c] = T.matrix()(r, c);
// Returns the library's code; on any code but DDDMR_OK `out` is what it was.
template<class Cloud>
inline int sweepFeatures(dddmr_rollout_ctx * ctx, int source, int which, Cloud & out)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  size_t n = 0;
  int rc = dddmr_rollout_get_lidar_sweep_features(ctx, source, which, nullptr, nullptr, 0, &n);
  if (rc != DDDMR_OK) {return rc;}
  std::vector<float> xyzr(4 * n);
  if (n) {
    rc = dddmr_rollout_get_lidar_sweep_features(ctx, source, which, xyzr.data(), nullptr, n, &n);
    if (rc != DDDMR_OK) {return rc;}
  }
  out.points.resize(n);
  for (size_t i = 0; i < n; ++i) {
    out.points[i].x = xyzr[4 * i + 0];
    out.points[i].y = xyzr[4 * i + 1];
    out.points[i].z = xyzr[4 * i + 2];
    out.points[i].intensity = xyzr[4 * i + 3];
  }
  return DDDMR_OK;
}

// What the host FeatureAssociation and mapOptimization take of the source's latest accepted sweep once
// dddmr_rollout_set_lidar_sweep_association has switched the association on: cornerPointsSharp, cornerPointsLessSharp,
// surfPointsFlat and surfPointsLessFlat with ring + scan_period * relTime in `intensity` (frame 0: the association frame
// extractFeatures holds them in, what updateTransformation and publishCloudsLast read; frame 1: through the features'
// T_out, what publishCloud publishes), the three orientation fields of the cloud_info message, and outlier_cloud
// (pitch-removed frame; adjustOutlierCloud's axis change stays with the caller).  Everything is read before anything
// is written: on any code but DDDMR_OK the outputs are what they were.
template<class Cloud, class CloudInfo>
inline int sweepAssociation(
  dddmr_rollout_ctx * ctx, int source, int frame, Cloud & sharp, Cloud & less_sharp, Cloud & flat, Cloud & less_flat,
  CloudInfo & seg_msg, Cloud & outliers)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  float orient[3] = {0.f, 0.f, 0.f};
  int rc = dddmr_rollout_get_lidar_sweep_orientation(ctx, source, orient, nullptr);
  if (rc != DDDMR_OK) {return rc;}
  std::vector<float> xyzi[5];                              // the four clouds, then the outliers
  for (int which = 0; which < 5; ++which) {
    size_t n = 0;
    rc = which < 4 ? dddmr_rollout_get_lidar_sweep_association(ctx, source, which, frame, nullptr, nullptr, 0, &n) :
      dddmr_rollout_get_lidar_sweep_outliers(ctx, source, nullptr, 0, &n);
    if (rc != DDDMR_OK) {return rc;}
    xyzi[which].resize(4 * n);
    if (n) {
      rc = which < 4 ? dddmr_rollout_get_lidar_sweep_association(ctx, source, which, frame, xyzi[which].data(), nullptr, n, &n) :
        dddmr_rollout_get_lidar_sweep_outliers(ctx, source, xyzi[which].data(), n, &n);
      if (rc != DDDMR_OK) {return rc;}
      xyzi[which].resize(4 * n);
    }
  }
  Cloud * const out[5] = {&sharp, &less_sharp, &flat, &less_flat, &outliers};
  for (int which = 0; which < 5; ++which) {
    const std::vector<float> & v = xyzi[which];
    out[which]->points.resize(v.size() / 4);
    for (size_t i = 0; i < v.size() / 4; ++i) {
      out[which]->points[i].x = v[4 * i + 0];
      out[which]->points[i].y = v[4 * i + 1];
      out[which]->points[i].z = v[4 * i + 2];
      out[which]->points[i].intensity = v[4 * i + 3];
    }
  }
  seg_msg.start_orientation = orient[0];
  seg_msg.end_orientation = orient[1];
  seg_msg.orientation_diff = orient[2];
  return DDDMR_OK;
}

// DepthCameraObservationBuffer::bufferCloud for the local planner: the raw frame in the SENSOR frame (pcl::fromROSMsg
// output) goes to depth source `source` of the device, which transforms, applies the obstacle-height band, voxelises
// above 20000 points, stamps the observation with stamp_ns (the buffer's clock_->now() in nanoseconds) and purges
// stale frames.  `source` must have been configured with dddmr_rollout_set_depth_source (the buffer's
// min/max_obstacle_height and observation_persistence); sources are numbered in plugin order, the cameras of one
// layer in topic-name order (the std::map order getObservation() concatenates them in).
template<class Cloud, class TransformStamped>
inline int feedDepthFrame(
  dddmr_rollout_ctx * ctx, int source, const Cloud & frame_sensor_frame, const TransformStamped & trans_b2s,
  const TransformStamped & trans_gbl2b, int64_t stamp_ns, uint32_t * n_frame_out = nullptr,
  uint32_t * n_source_out = nullptr, uint32_t * n_aggregate_out = nullptr)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  double b2s[7], g2b[7];
  toPose7(trans_b2s, b2s);
  toPose7(trans_gbl2b, g2b);
  const size_t n = frame_sensor_frame.points.size();
  const int rc = dddmr_rollout_set_depth_frame(
    ctx, source, n ? &frame_sensor_frame.points[0].x : nullptr, n, sizeof(frame_sensor_frame.points[0]), b2s, g2b,
    stamp_ns, n_frame_out, n_source_out, n_aggregate_out);
  if (rc == DDDMR_OK) {SharedContext::noteDeviceFeed();}
  return rc;
}

// DepthImg2PointCloud::cbDepthImg and bufferCloud in one call: the 16UC1 image as sensor_msgs::msg::Image carries it
// (data = msg.data.data(), width, height, step) goes to depth image source `source`, configured with
// dddmr_rollout_set_depth_image_source from the camera_info topic and the node's parameters.  trans_b2o takes the image's
// optical frame (msg.header.frame_id) to the base frame.  width / height are checked against nothing here: the source
// was configured with them and the library refuses a step below 2 * width.  Returns the library's code and notes a
// device feed on DDDMR_OK only; on any other code nothing on the device has changed and the caller runs its CPU path
// (the node's cloud into bufferCloud) for this image.
template<class TransformStamped>
inline int feedDepthImage(
  dddmr_rollout_ctx * ctx, int source, const uint8_t * data, uint32_t width, uint32_t height, uint32_t step,
  const TransformStamped & trans_b2o, const TransformStamped & trans_gbl2b, int64_t stamp_ns,
  uint32_t * n_camera_out = nullptr, uint32_t * n_frame_out = nullptr, uint32_t * n_source_out = nullptr,
  uint32_t * n_aggregate_out = nullptr)
{
  if (!ctx || !data || width == 0 || height == 0) {return DDDMR_ERR_BAD_ARG;}
  double b2o[7], g2b[7];
  toPose7(trans_b2o, b2o);
  toPose7(trans_gbl2b, g2b);
  const int rc = dddmr_rollout_set_depth_image(
    ctx, source, reinterpret_cast<const uint16_t *>(data), step, b2o, g2b, stamp_ns, n_camera_out, n_frame_out,
    n_source_out, n_aggregate_out);
  if (rc == DDDMR_OK) {SharedContext::noteDeviceFeed();}
  return rc;
}

// The frustum half of bufferCloud: call beside feedDepthFrame / feedDepthImage with m2s = lookupTransform(global_frame_,
// origin_frame) and the buffer's FOV_W_ / FOV_V_ / min_ / max_detect_distance_.  Replaces the source's frustum; no feed
// is noted (the aggregate does not change).  Cameras are numbered in the order of their names in observation_buffers_.
template<class TransformStamped>
inline int feedDepthFrustum(
  dddmr_rollout_ctx * ctx, int source, double FOV_W, double FOV_V, double min_detect_distance,
  double max_detect_distance, const TransformStamped & trans_m2s)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  double m2s[7];
  toPose7(trans_m2s, m2s);
  dddmr_depth_frustum_config cfg;
  cfg.FOV_W = FOV_W; cfg.FOV_V = FOV_V;
  cfg.obstacle_min_range = min_detect_distance; cfg.obstacle_max_range = max_detect_distance;
  return dddmr_rollout_set_depth_frustum(ctx, source, &cfg, m2s);
}

// One marking selfClear's window loop selected: its voxel key (the three map keys) and its stored cluster pc_.
template<class Cloud>
struct DepthMarkingRef
{
  int32_t x, y, z;
  const Cloud * pc;
};

// selfClear's decision tree for the markings of the current window, on the device: kept[i] != 0 means "push to
// current_observation_ptr", 0 means removePCPtr.  The caller keeps what selfClear does around it: the early returns,
// trans_gbl2b_, the window bounds and the getXIter / lower_bound walk that collects `markings` (skipping null pc_),
// and afterwards removePCPtr / pc_current_window_ / the casting markers for the verdicts.  branch (optional) receives
// 1 outside the frustums, 2 attached, 3 inside.  On any code but DDDMR_OK nothing is written and the caller runs the
// reference's CPU loop for this pass.
template<class Cloud>
inline int depthClearVerdicts(
  dddmr_rollout_ctx * ctx, double resolution, double height_resolution,
  const std::vector<DepthMarkingRef<Cloud>> & markings, std::vector<uint8_t> & kept,
  std::vector<uint8_t> * branch = nullptr, std::vector<uint32_t> * engaged = nullptr)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  const size_t m = markings.size();
  std::vector<int32_t> voxel(3 * m);
  std::vector<uint32_t> offsets(m + 1, 0u);
  for (size_t i = 0; i < m; ++i) {
    if (!markings[i].pc) {return DDDMR_ERR_BAD_ARG;}
    voxel[3 * i] = markings[i].x; voxel[3 * i + 1] = markings[i].y; voxel[3 * i + 2] = markings[i].z;
    offsets[i + 1] = offsets[i] + static_cast<uint32_t>(markings[i].pc->points.size());
  }
  std::vector<float> xyz(3 * static_cast<size_t>(offsets[m]));
  size_t at = 0;
  for (size_t i = 0; i < m; ++i) {
    for (const auto & p : markings[i].pc->points) {
      xyz[at++] = p.x; xyz[at++] = p.y; xyz[at++] = p.z;
    }
  }
  std::vector<uint8_t> verdict(m);
  std::vector<uint32_t> eng(m);
  const int rc = dddmr_rollout_depth_clear_verdicts(
    ctx, resolution, height_resolution, voxel.data(), offsets.data(), xyz.data(), m, verdict.data(), eng.data());
  if (rc != DDDMR_OK) {return rc;}
  kept.resize(m);
  if (branch) {branch->resize(m);}
  for (size_t i = 0; i < m; ++i) {
    kept[i] = verdict[i] & 1u;
    if (branch) {(*branch)[i] = (verdict[i] >> 1) & 3u;}
  }
  if (engaged) {engaged->swap(eng);}
  return rc;
}

// The depth layer's selfMark state: pcl_ground_ and pcl_map_ (shared_data_) go to the device once, with the layer's
// resolutions and clustering parameters.  Returns the library's code.  There is no "ready" flag on this side to set too
// early: until this has returned DDDMR_OK the library answers depthMarkClusters with DDDMR_ERR_STATE and the layer runs
// its CPU selfMark.
template<class GroundCloud, class MapCloud>
inline int depthMarkCreate(
  dddmr_rollout_ctx * ctx, const GroundCloud & pcl_ground, const MapCloud & pcl_map, double resolution,
  double height_resolution, double euclidean_cluster_extraction_tolerance,
  int euclidean_cluster_extraction_min_cluster_size, double segmentation_ignore_ratio, uint32_t max_observation_points)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  dddmr_depth_mark_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.xy_resolution = resolution; cfg.height_resolution = height_resolution;
  cfg.euclidean_cluster_extraction_tolerance = euclidean_cluster_extraction_tolerance;
  cfg.euclidean_cluster_extraction_min_cluster_size = euclidean_cluster_extraction_min_cluster_size;
  cfg.segmentation_ignore_ratio = segmentation_ignore_ratio;
  cfg.max_observation_points = max_observation_points;
  const size_t ng = pcl_ground.points.size(), nm = pcl_map.points.size();
  return dddmr_rollout_depth_mark_create(
    ctx, &cfg, ng ? &pcl_ground.points[0].x : nullptr, ng, sizeof(pcl_ground.points[0]),
    nm ? &pcl_map.points[0].x : nullptr, nm, sizeof(pcl_map.points[0]));
}

// What one selfMark hands to addPCPtr, in the order the reference would call it.
template<class Cloud>
struct DepthMarkClusters
{
  struct Cluster
  {
    float cx, cy, cz;      // addPCPtr's centroid arguments
    int32_t voxel[3];      // the key addPCPtr will compute from them
    uint32_t size;         // points before the 0.2 m VoxelGrid
    Cloud cloud;           // cloud_cluster: the downsampled points
  };
  std::vector<Cluster> clusters;
  float coefficients[4];   // pcl::ModelCoefficients::values of :568-578, the same for every cluster
  dddmr_depth_mark_stats stats;
};

// selfMark from the aggregated observation on (depth_camera_layer.cpp:487-601), on the device.  The caller keeps the
// early returns and trans_gbl2b_, then walks out.clusters front to back calling
// pct_marking_->addPCPtr(cx, cy, cz, cloud, coefficients).  The two debug clouds are not produced.  Returns the library's
// code; on anything but DDDMR_OK `out` holds no cluster and the layer runs its CPU selfMark for this pass.
template<class Cloud, class TransformStamped>
inline int depthMarkClusters(dddmr_rollout_ctx * ctx, const TransformStamped & trans_gbl2b, DepthMarkClusters<Cloud> & out)
{
  out.clusters.clear();
  std::memset(&out.stats, 0, sizeof(out.stats));
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  double g2b[7];
  toPose7(trans_gbl2b, g2b);
  int rc = dddmr_rollout_depth_mark_clusters(ctx, g2b, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &out.stats);
  if (rc != DDDMR_OK) {return rc;}
  const size_t c = out.stats.n_accepted, p = out.stats.n_points;
  std::vector<float> centroid(3 * c + 3), xyz(3 * p + 3);
  std::vector<int32_t> voxel(3 * c + 3);
  std::vector<uint32_t> size(c + 1), offsets(c + 1);
  rc = dddmr_rollout_depth_mark_clusters(
    ctx, g2b, c, p, centroid.data(), voxel.data(), size.data(), offsets.data(), xyz.data(), out.coefficients, &out.stats);
  if (rc != DDDMR_OK) {return rc;}          // (a frame published between the two calls: capacity; the next pass retries)
  out.clusters.resize(out.stats.n_accepted);
  for (size_t i = 0; i < out.clusters.size(); ++i) {
    auto & cl = out.clusters[i];
    cl.cx = centroid[3 * i]; cl.cy = centroid[3 * i + 1]; cl.cz = centroid[3 * i + 2];
    cl.voxel[0] = voxel[3 * i]; cl.voxel[1] = voxel[3 * i + 1]; cl.voxel[2] = voxel[3 * i + 2];
    cl.size = size[i];
    cl.cloud.points.resize(offsets[i + 1] - offsets[i]);
    for (uint32_t j = offsets[i]; j < offsets[i + 1]; ++j) {
      auto & pt = cl.cloud.points[j - offsets[i]];
      pt.x = xyz[3 * static_cast<size_t>(j)]; pt.y = xyz[3 * static_cast<size_t>(j) + 1]; pt.z = xyz[3 * static_cast<size_t>(j) + 2];
    }
  }
  return DDDMR_OK;
}

// PathBlockedStrategy::selfMark on the device's aggregate observation.  pcl_prune_plan is
// shared_data_->pcl_prune_plan_ (pcl::PointXYZI, 32-byte records: repacked to x y z intensity).
template<class PlanCloud>
inline int pathBlocked(
  dddmr_rollout_ctx * ctx, const PlanCloud & pcl_prune_plan, double check_radius, double * blocked_ratio_percent,
  bool * path_blocked_wait)
{
  if (!ctx) {return DDDMR_ERR_BAD_ARG;}
  std::vector<float> xyzi(4 * pcl_prune_plan.points.size());
  for (size_t i = 0; i < pcl_prune_plan.points.size(); ++i) {
    const auto & p = pcl_prune_plan.points[i];
    xyzi[4 * i] = p.x; xyzi[4 * i + 1] = p.y; xyzi[4 * i + 2] = p.z; xyzi[4 * i + 3] = p.intensity;
  }
  int32_t opinion = DDDMR_OPINION_PASS;
  const int rc = dddmr_rollout_path_blocked(
    ctx, xyzi.data(), pcl_prune_plan.points.size(), check_radius, blocked_ratio_percent, &opinion, nullptr);
  if (rc == DDDMR_OK && path_blocked_wait) {*path_blocked_wait = opinion == DDDMR_OPINION_PATH_BLOCKED_WAIT;}
  return rc;
}

// The global-mode marking / clearing layer of ONE lidar plugin instance.  Mirrors what the plugin keeps:
// pct_marking_ (store + lethal_map_) and dGraph_ live on the device; host copies of the dGraph and the lethal set
// are refreshed after every update, because get_dGraphValue() is called per ground node by the global planner's
// A* (perception_3d_ros.cpp get_min_dGraphValue) and must not cost a device round trip each.
class MarkingLayerBridge
{
public:
  // resetdGraph (:831-839) / first use: pcl_ground = shared_data_->pcl_ground_ (static_ground_size_ nodes),
  // pcl_map = shared_data_->pcl_map_.  Parameters as the plugin read them in onInitialize (:58-170).
  template<class GroundCloud, class MapCloud>
  int create(
    dddmr_rollout_ctx * ctx, const dddmr_marking_config & cfg, const GroundCloud & pcl_ground, size_t static_ground_size,
    const MapCloud & pcl_map)
  {
    ctx_ = ctx;
    n_ground_ = static_ground_size;
    const size_t nm = pcl_map.points.size();
    const int rc = dddmr_rollout_marking_create(
      ctx, &cfg, n_ground_ ? &pcl_ground.points[0].x : nullptr, n_ground_, sizeof(pcl_ground.points[0]),
      nm ? &pcl_map.points[0].x : nullptr, nm, nm ? sizeof(pcl_map.points[0]) : 16);
    if (rc != DDDMR_OK) {return rc;}
    dgraph_.assign(n_ground_ + 1, cfg.max_obstacle_distance);
    lethal_.assign(n_ground_ + 1, 0);
    return DDDMR_OK;
  }
  bool ready() const {return ctx_ != nullptr;}

  // resetdGraph after create
  int reset(double max_obstacle_distance)
  {
    const int rc = dddmr_rollout_marking_reset(ctx_);
    if (rc == DDDMR_OK) {
      dgraph_.assign(n_ground_ + 1, max_obstacle_distance);
      lethal_.assign(n_ground_ + 1, 0);
    }
    return rc;
  }

  // one doClear_then_Mark pass: selfClear against the previous observation, selfMark of the observation the last
  // feedScan left on the device; then the host copies are refreshed
  template<class TransformStamped>
  int clearThenMark(const TransformStamped & trans_b2s, const TransformStamped & trans_gbl2b, dddmr_marking_stats * stats = nullptr)
  {
    double b2s[7], g2b[7];
    toPose7(trans_b2s, b2s);
    toPose7(trans_gbl2b, g2b);
    int rc = dddmr_rollout_marking_update(ctx_, b2s, g2b, stats);
    if (rc != DDDMR_OK) {return rc;}
    rc = dddmr_rollout_marking_get_dgraph(ctx_, dgraph_.data(), dgraph_.size());
    if (rc != DDDMR_OK) {return rc;}
    return dddmr_rollout_marking_get_lethal(ctx_, lethal_.data(), lethal_.size());
  }

  // Marking::get_dGraphValue(index)
  double dGraphValue(unsigned int index) const {return index < dgraph_.size() ? dgraph_[index] : 9999.0;}

  // updateLethalPointCloud (:283-304): the ground nodes of lethal_map_ as points of `out` (pcl::PointXYZI cloud)
  template<class GroundCloud, class LethalCloud>
  void lethalPointCloud(const GroundCloud & pcl_ground, LethalCloud & out) const
  {
    for (size_t i = 0; i < lethal_.size() && i < pcl_ground.points.size(); ++i) {
      if (!lethal_[i]) {continue;}
      typename LethalCloud::PointType ipt;
      ipt.x = pcl_ground.points[i].x; ipt.y = pcl_ground.points[i].y; ipt.z = pcl_ground.points[i].z;
      out.push_back(ipt);
    }
  }

  // the `global_marking` topic (pubUpdateLoop, :755-775): the reference publishes every alive marking's stored cluster
  // (its 0.2 m-downsampled points); the device stores what the dGraph is computed from instead -- the same clusters
  // projected on the robot's ground plane at 0.1 m -- so the published cloud is that: same footprints, z on the plane.
  // Fetched on demand only (call it when the topic has subscribers).
  template<class MarkingCloud>
  int markingPointCloud(MarkingCloud & out) const
  {
    size_t n = 0;
    int rc = dddmr_rollout_marking_get_points(ctx_, nullptr, nullptr, 0, &n);
    if (rc != DDDMR_OK || n == 0) {return rc;}
    std::vector<float> xyz(3 * n);
    rc = dddmr_rollout_marking_get_points(ctx_, xyz.data(), nullptr, n, &n);
    if (rc != DDDMR_OK) {return rc;}
    for (size_t i = 0; i < n; ++i) {
      typename MarkingCloud::PointType ipt;
      ipt.x = xyz[3 * i]; ipt.y = xyz[3 * i + 1]; ipt.z = xyz[3 * i + 2];
      out.push_back(ipt);
    }
    return DDDMR_OK;
  }

private:
  dddmr_rollout_ctx * ctx_ = nullptr;
  size_t n_ground_ = 0;
  std::vector<double> dgraph_;
  std::vector<uint8_t> lethal_;
};

// dddmr_marking_config from the plugin's members (names as in multilayer_spinning_lidar.h); capacities sized from the
// map: every ground node can carry a handful of markings over a long drive
inline dddmr_marking_config markingConfig(
  double resolution, double height_resolution, double marking_height, double perception_window_size,
  double vertical_FOV_top, double vertical_FOV_bottom, double scan_effective_positive_start,
  double scan_effective_positive_end, double scan_effective_negative_start, double scan_effective_negative_end,
  double euclidean_cluster_extraction_tolerance, int euclidean_cluster_extraction_min_cluster_size,
  double segmentation_ignore_ratio, double inscribed_radius, double inflation_radius, double max_obstacle_distance,
  size_t static_ground_size)
{
  dddmr_marking_config c;
  std::memset(&c, 0, sizeof(c));
  c.xy_resolution = resolution; c.height_resolution = height_resolution;
  c.marking_height = marking_height; c.perception_window_size = perception_window_size;
  c.vertical_FOV_top = vertical_FOV_top; c.vertical_FOV_bottom = vertical_FOV_bottom;
  c.scan_effective_positive_start = scan_effective_positive_start; c.scan_effective_positive_end = scan_effective_positive_end;
  c.scan_effective_negative_start = scan_effective_negative_start; c.scan_effective_negative_end = scan_effective_negative_end;
  c.euclidean_cluster_extraction_tolerance = euclidean_cluster_extraction_tolerance;
  c.euclidean_cluster_extraction_min_cluster_size = euclidean_cluster_extraction_min_cluster_size;
  c.segmentation_ignore_ratio = segmentation_ignore_ratio;
  c.inscribed_radius = inscribed_radius; c.inflation_radius = inflation_radius;
  c.max_obstacle_distance = max_obstacle_distance;
  size_t markings = 1u << 15;
  while (markings < 4 * static_ground_size && markings < (1u << 22)) {markings <<= 1;}
  c.max_markings = static_cast<uint32_t>(markings);
  c.max_cluster_points = static_cast<uint32_t>(markings * 16 > (1u << 26) ? (1u << 26) : markings * 16);
  return c;
}

// The global-mode DepthCameraLayer with its marking store, dGraph and lethal set on the device
// (the depth_layer entries of dddmr_rollout.h): what selfClear / selfMark / resetdGraph / updateLethalPointCloud / get_dGraphValue of
// a patched layer call.  ready() is true only after a create that returned DDDMR_OK and goes false again on ANY failure
// of create, reset or clearThenMark: the caller then runs its CPU pass and must not read this bridge's copies until a
// later create has succeeded (the device state no longer follows the layer's history).
class DepthLayerBridge
{
public:
  template<class GroundCloud, class MapCloud>
  int create(
    dddmr_rollout_ctx * ctx, const dddmr_depth_layer_config & cfg, const GroundCloud & pcl_ground, size_t static_ground_size,
    const MapCloud & pcl_map)
  {
    ready_ = false;
    if (!ctx) {return DDDMR_ERR_BAD_ARG;}
    const size_t nm = pcl_map.points.size();
    const int rc = dddmr_rollout_depth_layer_create(
      ctx, &cfg, static_ground_size ? &pcl_ground.points[0].x : nullptr, static_ground_size, sizeof(pcl_ground.points[0]),
      nm ? &pcl_map.points[0].x : nullptr, nm, nm ? sizeof(pcl_map.points[0]) : 16);
    if (rc != DDDMR_OK) {return rc;}
    ctx_ = ctx;
    n_ground_ = static_ground_size;
    max_obstacle_distance_ = cfg.max_obstacle_distance;
    dgraph_.assign(n_ground_ + 1, max_obstacle_distance_);
    lethal_.assign(n_ground_ + 1, 0);
    ready_ = true;
    return DDDMR_OK;
  }
  bool ready() const {return ready_;}

  // resetdGraph
  int reset()
  {
    if (!ready_) {return DDDMR_ERR_STATE;}
    const int rc = dddmr_rollout_depth_layer_reset(ctx_);
    if (rc != DDDMR_OK) {ready_ = false; return rc;}
    dgraph_.assign(n_ground_ + 1, max_obstacle_distance_);
    lethal_.assign(n_ground_ + 1, 0);
    return DDDMR_OK;
  }

  // one selfClear + selfMark pass on the observation the depth feeds left on the device, then the host copies of the
  // dGraph and the lethal flags are refreshed.  Any code but DDDMR_OK: run the CPU pass; ready() is false from then on.
  template<class TransformStamped>
  int clearThenMark(const TransformStamped & trans_gbl2b, dddmr_depth_layer_stats * stats = nullptr)
  {
    if (!ready_) {return DDDMR_ERR_STATE;}
    double g2b[7];
    toPose7(trans_gbl2b, g2b);
    dddmr_depth_layer_stats local;
    int rc = dddmr_rollout_depth_layer_update(ctx_, g2b, stats ? stats : &local);
    if (rc == DDDMR_OK) {rc = dddmr_rollout_depth_layer_get_dgraph(ctx_, dgraph_.data(), dgraph_.size());}
    if (rc == DDDMR_OK) {rc = dddmr_rollout_depth_layer_get_lethal(ctx_, lethal_.data(), lethal_.size());}
    if (rc != DDDMR_OK) {ready_ = false;}
    return rc;
  }

  // Marking::get_dGraphValue(index)
  double dGraphValue(unsigned int index) const {return index < dgraph_.size() ? dgraph_[index] : 9999.0;}

  // updateLethalPointCloud: the ground nodes of lethal_map_ as points of `out`
  template<class GroundCloud, class LethalCloud>
  void lethalPointCloud(const GroundCloud & pcl_ground, LethalCloud & out) const
  {
    for (size_t i = 0; i < n_ground_ && i < lethal_.size() && i < pcl_ground.points.size(); ++i) {
      if (!lethal_[i]) {continue;}
      typename LethalCloud::PointType ipt;
      ipt.x = pcl_ground.points[i].x; ipt.y = pcl_ground.points[i].y; ipt.z = pcl_ground.points[i].z;
      out.push_back(ipt);
    }
  }

  // the marking topic: every alive marking's stored cluster pc_ (its 0.2 m-downsampled points), as the reference
  // publishes it.  Fetched on demand only (call it when the topic has subscribers).
  template<class MarkingCloud>
  int markingPointCloud(MarkingCloud & out) const
  {
    if (!ready_) {return DDDMR_ERR_STATE;}
    size_t m = 0, p = 0;
    int rc = dddmr_rollout_depth_layer_get_clusters(ctx_, nullptr, nullptr, nullptr, 0, 0, &m, &p);
    if (rc != DDDMR_OK || p == 0) {return rc;}
    std::vector<int32_t> voxel(3 * m);
    std::vector<uint32_t> offsets(m + 1);
    std::vector<float> xyz(3 * p);
    rc = dddmr_rollout_depth_layer_get_clusters(ctx_, voxel.data(), offsets.data(), xyz.data(), m, p, &m, &p);
    if (rc != DDDMR_OK) {return rc;}
    for (size_t i = 0; i < p; ++i) {
      typename MarkingCloud::PointType ipt;
      ipt.x = xyz[3 * i]; ipt.y = xyz[3 * i + 1]; ipt.z = xyz[3 * i + 2];
      out.push_back(ipt);
    }
    return DDDMR_OK;
  }

private:
  dddmr_rollout_ctx * ctx_ = nullptr;
  bool ready_ = false;
  size_t n_ground_ = 0;
  double max_obstacle_distance_ = 9999.0;
  std::vector<double> dgraph_;
  std::vector<uint8_t> lethal_;
};

// The perception stack of a context (the stack entries of dddmr_rollout.h): what StackedPerception::doClear_then_Mark,
// get_min_dGraphValue, aggregateLethal and resetdGraph of a patched Perception3D_ROS call when the lidar layer and the
// depth camera layer both live on the device.  One pass updates every device layer on its own sensor's observation;
// the host keeps a mirror of the stacked minimum dGraph and the lethal masks and applies the pass's change list to it
// (a few hundred nodes around the robot) instead of fetching whole arrays.  When the list overflowed
// (DDDMR_ERR_CAPACITY) the two full getters resynchronise the mirror.  The layers themselves are created through
// MarkingLayerBridge::create / DepthLayerBridge::create on the SAME pcl_ground_, before create() here; their own
// clearThenMark is not called in a context that has a stack.  ready() is false after any failure that leaves the
// mirror behind the device: the caller then runs its CPU pass until a later create has succeeded.
class PerceptionStackBridge
{
public:
  int create(dddmr_rollout_ctx * ctx, const dddmr_stack_config & cfg)
  {
    ready_ = false;
    if (!ctx) {return DDDMR_ERR_BAD_ARG;}
    const int rc = dddmr_rollout_stack_create(ctx, &cfg);
    if (rc != DDDMR_OK) {return rc;}
    ctx_ = ctx;
    cfg_ = cfg;
    n_ground_ = cfg.n_ground;
    min_dgraph_.assign(n_ground_ + 1, kStart);
    mask_.assign(n_ground_ + 1, 0);
    nodes_.resize(cfg.max_changes ? cfg.max_changes : 1);
    values_.resize(nodes_.size());
    masks_.resize(nodes_.size());
    return resync();                     // the layers may hold state already
  }
  bool ready() const {return ready_;}

  // a layer whose dGraph the host computes (static layer, zone layers): values[0 .. n_ground]; shows in the next pass
  int setHostLayer(int slot, const std::vector<double> & values)
  {
    if (!ctx_ || values.size() != n_ground_ + 1) {return DDDMR_ERR_BAD_ARG;}
    return dddmr_rollout_stack_set_host_layer(ctx_, slot, values.data());
  }

  // StackedPerception::resetdGraph
  int reset()
  {
    if (!ready_) {return DDDMR_ERR_STATE;}
    const int rc = dddmr_rollout_stack_reset(ctx_);
    if (rc != DDDMR_OK) {ready_ = false; return rc;}
    return resync();
  }

  // One doClear_then_Mark pass over the device layers, then the mirror follows.  The return code is the pass's: a layer
  // that failed (its code is in stats) does not stop the mirror from following the stacked arrays, which the device
  // recomputes whatever the layers returned.  resynced (may be null): the change list overflowed and the full arrays
  // were fetched.
  template<class TransformStamped>
  int clearThenMark(
    const TransformStamped & trans_b2s, const TransformStamped & trans_gbl2b, dddmr_stack_stats * stats = nullptr,
    bool * resynced = nullptr)
  {
    if (!ready_) {return DDDMR_ERR_STATE;}
    double b2s[7], g2b[7];
    toPose7(trans_b2s, b2s);
    toPose7(trans_gbl2b, g2b);
    dddmr_stack_stats local;
    const int rc = dddmr_rollout_stack_update(ctx_, b2s, g2b, stats ? stats : &local);
    if (resynced) {*resynced = false;}
    size_t n = 0;
    int rl = dddmr_rollout_stack_get_changes(ctx_, nodes_.data(), values_.data(), masks_.data(), nodes_.size(), &n);
    if (rl == DDDMR_ERR_CAPACITY) {
      if (resynced) {*resynced = true;}
      rl = resync();
    } else if (rl == DDDMR_OK) {
      for (size_t i = 0; i < n; ++i) {
        if (nodes_[i] >= min_dgraph_.size()) {ready_ = false; return DDDMR_ERR_STATE;}
        min_dgraph_[nodes_[i]] = values_[i];
        mask_[nodes_[i]] = masks_[i];
      }
    }
    if (rl != DDDMR_OK) {ready_ = false; return rl;}
    return rc;
  }

  // StackedPerception::get_min_dGraphValue(index): the reference's start value beyond the end
  double minDGraphValue(unsigned int index) const {return index < min_dgraph_.size() ? min_dgraph_[index] : kStart;}
  uint8_t lethalMask(unsigned int index) const {return index < mask_.size() ? mask_[index] : 0;}

  // StackedPerception::aggregateLethal (:142-155): the device layers' lethal clouds one after the other in plugin order,
  // each the ground nodes whose flag is set in ascending order; a node lethal in two layers appears twice
  template<class GroundCloud, class LethalCloud>
  void aggregateLethal(const GroundCloud & pcl_ground, LethalCloud & out) const
  {
    for (int p = 0; p < cfg_.n_order; ++p) {
      if (cfg_.layer_order[p] >= DDDMR_STACK_HOST0) {continue;}
      for (size_t i = 0; i < n_ground_ && i < pcl_ground.points.size(); ++i) {
        if (!((mask_[i] >> p) & 1u)) {continue;}
        typename LethalCloud::PointType ipt;
        ipt.x = pcl_ground.points[i].x; ipt.y = pcl_ground.points[i].y; ipt.z = pcl_ground.points[i].z;
        out.push_back(ipt);
      }
    }
  }

  const std::vector<double> & minDGraph() const {return min_dgraph_;}
  const std::vector<uint8_t> & lethalMasks() const {return mask_;}

private:
  static constexpr double kStart = 99999.9;      // stacked_perception.cpp:116
  int resync()
  {
    int rc = dddmr_rollout_stack_get_min_dgraph(ctx_, min_dgraph_.data(), min_dgraph_.size());
    if (rc == DDDMR_OK) {rc = dddmr_rollout_stack_get_lethal_mask(ctx_, mask_.data(), mask_.size());}
    ready_ = rc == DDDMR_OK;
    return rc;
  }

  dddmr_rollout_ctx * ctx_ = nullptr;
  bool ready_ = false;
  dddmr_stack_config cfg_{};
  size_t n_ground_ = 0;
  std::vector<double> min_dgraph_;
  std::vector<uint8_t> mask_;
  std::vector<uint32_t> nodes_;
  std::vector<double> values_;
  std::vector<uint8_t> masks_;
};

}  // namespace dddmr_rollout_adapter
#endif
