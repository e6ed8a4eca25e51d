/*
 * dddmr_rollout.h -- C ABI of the MI355X local-planner rollout engine.
 *
 * One call (dddmr_rollout_tick) replaces the inner section of the reference's
 * Local_Planner::computeVelocityCommand
 *   (src/dddmr_local_planner/local_planner/src/local_planner.cpp:535-587):
 *   re-initialise theories -> generate all trajectories -> update critic shared
 *   data (kd-tree build) -> score every trajectory -> pick the best one.
 *
 * All paths cited below are relative to /root/reference/src/dddmr_local_planner/
 * unless they start with dddmr_perception_3d/ or dddmr_sys_core/.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; the caller owns every buffer it passes
 *     in and it only has to stay valid for the duration of the call;
 *   - every function returns 0 (DDDMR_OK) or a negative dddmr_status;
 *   - no exceptions cross this boundary, no callbacks into the caller;
 *   - a context is externally serialised exactly like the reference serialises
 *     ticks (perception mutex local_planner.cpp:498, critics mutex :577); the
 *     library additionally takes an internal mutex per call.  set_cloud /
 *     set_scan may be called from the sensor-callback thread while another
 *     thread ticks (the device cloud is triple-buffered: published / being read by
 *     a tick / free, so a producer never waits for a tick and never overwrites
 *     what one reads; producers are serialised among themselves).
 *   - the library never runs any of this on the CPU: with no usable HIP device
 *     dddmr_rollout_create fails with DDDMR_ERR_NO_DEVICE.
 */
#ifndef DDDMR_ROLLOUT_H_
#define DDDMR_ROLLOUT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDDMR_ROLLOUT_ABI_VERSION 2
#define DDDMR_MAX_CRITICS 8
#define DDDMR_NAME_LEN 64
#define DDDMR_COMM_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */

/* library status codes (return values) */
typedef enum {
  DDDMR_OK = 0,
  DDDMR_ERR_BAD_ARG = -1,
  DDDMR_ERR_NO_DEVICE = -2,
  DDDMR_ERR_HIP = -3,
  /* stacked_generator.cpp:82-91: unknown theory name is FATAL-logged and yields
     zero trajectories; here it is an explicit error. */
  DDDMR_ERR_UNKNOWN_THEORY = -4,
  DDDMR_ERR_CAPACITY = -5,
  DDDMR_ERR_STATE = -6
} dddmr_status;

/* dddmr_sys_core/include/dddmr_sys_core/dddmr_enum_states.h:46-54 (numeric
   values are part of the boundary).  The engine itself only produces
   ALL_TRAJECTORIES_FAIL or TRAJECTORY_FOUND; the other codes stay in the host
   driver (local_planner.cpp:484-524,597-607). */
typedef enum {
  DDDMR_TF_FAIL = 0,
  DDDMR_PRUNE_PLAN_FAIL = 1,
  DDDMR_ALL_TRAJECTORIES_FAIL = 2,
  DDDMR_PERCEPTION_MALFUNCTION = 3,
  DDDMR_TRAJECTORY_FOUND = 4,
  DDDMR_PATH_BLOCKED_WAIT = 5,
  DDDMR_PATH_BLOCKED_REPLANNING = 6
} dddmr_planner_state;

/* trajectory_generators.xml: the three theory plugins. */
typedef enum {
  DDDMR_THEORY_DD_SIMPLE = 0,        /* theories/dd_simple_trajectory_generator_theory.cpp */
  DDDMR_THEORY_OMNI_SIMPLE = 1,      /* theories/omni_simple_trajectory_generator_theory.cpp */
  DDDMR_THEORY_DD_ROTATE_INPLACE = 2 /* theories/dd_rotate_inplace_theory.cpp */
} dddmr_theory_kind;

/* mpc_critics.xml: the seven critic plugins. */
typedef enum {
  DDDMR_CRITIC_COLLISION = 0,          /* models/collision_model.cpp */
  DDDMR_CRITIC_COLLISION_MIN_MAX = 1,  /* models/collision_min_max_model.cpp */
  DDDMR_CRITIC_STICK_PATH = 2,         /* models/stick_path_model.cpp */
  DDDMR_CRITIC_PURE_PURSUIT = 3,       /* models/pure_pursuit_model.cpp */
  DDDMR_CRITIC_TOWARD_GLOBAL_PLAN = 4, /* models/toward_global_plan_model.cpp */
  DDDMR_CRITIC_SHORTEST_ANGLE = 5,     /* models/shortest_angle_model.cpp */
  DDDMR_CRITIC_TWIRLING = 6            /* models/twirling_model.cpp */
} dddmr_critic_kind;

/* Per-trajectory codes reported in costs[] (stacked_scoring_model.cpp:75-93:
   the first negative critic return becomes the trajectory cost). */
#define DDDMR_COST_COLLISION (-1.0)      /* collision_model.cpp:136-139 */
#define DDDMR_COST_PURE_PURSUIT_GUARD (-4.0) /* pure_pursuit_model.cpp:62-64 */
#define DDDMR_COST_NN_FAIL (-12.0)       /* toward_global_plan_model.cpp:74 */
/* Sample whose generateTrajectory() returned false (dd_simple...cpp:364-385);
   the reference never queues such a trajectory (local_planner.cpp:551-555). */
#define DDDMR_COST_NOT_GENERATED (-100.0)

/* One critic of a theory's stack.  `weight` is the plugin's ".weight"
   parameter (read by every model; unused by collision / stick_path exactly as
   in the reference), translation/orientation weights are PurePursuitModel's
   (pure_pursuit_model.cpp:50-56). */
typedef struct {
  int32_t kind; /* dddmr_critic_kind */
  int32_t reserved;
  double weight;
  double translation_weight;
  double orientation_weight;
} dddmr_critic_config;

/* One named theory = limits + params of the generator plugin
   (dd_simple...cpp:47-134, omni_simple...cpp:47-158, dd_rotate_inplace...cpp:47-129)
   + robot cuboid + the ordered critic stack bound to it through
   "<critic>.trajectory_generator" (mpc_critics/src/mpc_critics_ros.cpp:71-79). */
typedef struct {
  char name[DDDMR_NAME_LEN];
  int32_t kind; /* dddmr_theory_kind */
  int32_t use_motor_constraint;

  /* limits */
  double min_vel_x, max_vel_x;
  double min_vel_y, max_vel_y;         /* omni only */
  double min_vel_trans, max_vel_trans; /* omni only */
  double min_vel_theta, max_vel_theta;
  double acc_lim_x, acc_lim_y, acc_lim_theta;
  double deceleration_ratio;
  double max_motor_shaft_rpm, wheel_diameter, gear_ratio, robot_radius;

  /* params */
  double controller_frequency;
  double sim_time;
  double linear_x_sample, linear_y_sample, angular_z_sample;
  double sim_granularity, angular_sim_granularity;
  double rotation_speed; /* rotate-in-place only (dd_rotate_inplace_theory.cpp:127) */

  /* 8 cuboid vertices in base_link, in the reference push order
     blb, brb, blt, flb, brt, frt, flt, frb (dd_simple...cpp:211-218); the
     collision critic derives the box axes from [0]->[3], [0]->[1], [0]->[2]. */
  float cuboid[8][3];

  /* Bench-mode extensions; 0 = reference behaviour.
     bench_fixed_steps > 0: every trajectory uses exactly that many steps and
       dt = sim_time / steps (the reference's commented-out fixed variant,
       dd_simple...cpp:391-394).
     bench_no_zero_insert != 0: VelocityIterator does not insert the extra 0.0
       sample (velocity_iterator.h:63-65) so sample counts are exact powers. */
  int32_t bench_fixed_steps;
  int32_t bench_no_zero_insert;

  int32_t n_critics;
  int32_t reserved;
  dddmr_critic_config critics[DDDMR_MAX_CRITICS];
} dddmr_theory_config;

typedef struct {
  uint32_t abi_version; /* DDDMR_ROLLOUT_ABI_VERSION */
  int32_t device;       /* HIP device ordinal */
  /* Trajectory shard of this context: the context scores the
     contiguous global sample range [rank*N/world, (rank+1)*N/world).
     world_size <= 1 means the whole batch. */
  int32_t rank;
  int32_t world_size;
  uint32_t max_points;       /* capacity of the aggregate observation cloud (< 2^20) */
  uint32_t max_trajectories; /* capacity of one tick's sample list (global N, < 2^24) */
  uint32_t max_steps;        /* capacity of one trajectory's horizon (<= 4096).  A tick whose longest
                                trajectory does not fit one workgroup's LDS (about 700 poses with the
                                collision critic; the shipped configs need <= 252) fails with
                                DDDMR_ERR_CAPACITY instead of truncating */
  uint32_t max_plan_poses;   /* capacity of the prune plan (<= 512) */
  int32_t n_theories;
  int32_t reserved;
  const dddmr_theory_config* theories;
} dddmr_rollout_config;

/* Inputs of one control tick; mirrors what computeVelocityCommand copies into
   the generator and critic shared data (local_planner.cpp:528-533, 580-583). */
typedef struct {
  double robot_pose[7];  /* trans_gbl2b_: x y z qx qy qz qw */
  double robot_twist[3]; /* robot_state_.twist.twist: linear.x linear.y angular.z */
  /* perception shared data current_allowed_max_linear_speed_ (<= 0: none,
     dd_simple...cpp:260-262, omni_simple...cpp:406-411) */
  double allowed_max_linear_speed;
  /* ModelSharedData::heading_deviation_ (local_planner.cpp:262-263,295-296) */
  double heading_deviation;
} dddmr_tick_input;

typedef struct {
  int32_t planner_state;     /* DDDMR_ALL_TRAJECTORIES_FAIL or DDDMR_TRAJECTORY_FOUND */
  int32_t best_index;        /* global sample index of the winner, -1 if none */
  double best_cost;          /* -1.0 if none (local_planner.cpp:450) */
  double vx, vy, wz;         /* best_traj.{xv_,yv_,thetav_}; 0 if none (trajectory.cpp:34-37) */
  uint32_t n_samples;        /* global number of velocity samples this tick */
  uint32_t n_local;          /* samples scored by this context's shard */
  uint32_t local_begin;      /* first global sample index of the shard */
  uint32_t n_points_binned;  /* cloud points inside the local costmap tile */
  /* packed argmin key of this shard, see dddmr_rollout_pack_key */
  int64_t key;
  float device_ms;           /* HIP-event time of the tick's kernels */
  float score_ms;            /* HIP-event time of the fused rollout+critics kernel alone */
} dddmr_rollout_result;

/* Optional per-trajectory outputs of the last tick (caller-allocated). */
typedef struct {
  double* costs;      /* [n_local] accumulated cost or reject code */
  int32_t* steps;     /* [n_local] generated steps (0 = not generated) */
  float* samples;     /* [n_local][3] vx vy wz of each sample */
} dddmr_rollout_debug;

typedef struct dddmr_rollout_ctx dddmr_rollout_ctx;

/* Replaces Trajectory_Generators_ROS / MPC_Critics_ROS plugin loading
   (trajectory_generators/src/trajectory_generators_ros.cpp:45-84,
    mpc_critics/src/mpc_critics_ros.cpp:45-83). */
int dddmr_rollout_create(const dddmr_rollout_config* cfg, dddmr_rollout_ctx** out);
void dddmr_rollout_destroy(dddmr_rollout_ctx* ctx);

/* Aggregate observation in the global frame = output of
   StackedPerception::aggregateObservations
   (dddmr_perception_3d/src/stacked_perception.cpp:128-140).  xyzi points at
   n_points records, stride_bytes apart, each starting with float x,y,z
   (PCL PointXYZI: stride 32; packed xyzi: 16; packed xyz: 12). */
int dddmr_rollout_set_cloud(dddmr_rollout_ctx* ctx, const float* xyzi,
                            size_t n_points, size_t stride_bytes);

/* Fused local-mode perception feed = MultiLayerSpinningLidar::cbSensor
   (dddmr_perception_3d/plugins/multilayer_spinning_lidar.cpp:177-281):
   sensor->base transform, PassThrough crop |x|,|y| <= window, 0 <= z <= height,
   0.1 m VoxelGrid centroid downsample, base->global transform; the result
   becomes the aggregate observation without leaving the device.
   T_* are x y z qx qy qz qw. */
int dddmr_rollout_set_scan(dddmr_rollout_ctx* ctx, const float* xyz, size_t n_points,
                           size_t stride_bytes, const double T_base_sensor[7],
                           const double T_gbl_base[7], double perception_window_size,
                           double marking_height, uint32_t* n_out_points);

/* cbSensor's stitcher (multilayer_spinning_lidar.cpp:185-200, parameter `stitcher_num`): with
   stitcher_num > 0 every dddmr_rollout_set_scan feeds the last stitcher_num RAW scans, oldest first,
   through the CURRENT transforms (exactly what the reference does: the queued scans are not
   re-registered).  0 switches it off and empties the queue.  The queued scans together must fit
   max_points. */
int dddmr_rollout_set_stitcher(dddmr_rollout_ctx* ctx, int32_t stitcher_num);

/* Several sensors on one aggregate: StackedPerception::aggregateObservations
   (dddmr_perception_3d/src/stacked_perception.cpp:128-140) concatenates every sensor plugin's
   current observation, in plugin order.  source_id = the sensor's position in that order
   (0 .. DDDMR_MAX_SOURCES - 1); each call runs that sensor's cbSensor on the device and the aggregate
   becomes the concatenation, in source order, of every source's LATEST observation (a source that has
   not reported yet contributes nothing).  *n_source_points / *n_aggregate_points (either may be NULL)
   receive the two sizes.  The first call with a source id switches the context to this mode; plain
   dddmr_rollout_set_scan then means source 0.  The observations together must fit max_points: a scan
   whose observation does not fit beside the other sources' is refused with DDDMR_ERR_CAPACITY, and since
   the source's one buffer is overwritten by then, that source is left EMPTY and the aggregate is
   republished from the other sources.  They feed on as before, and the refused source works again as
   soon as its observation fits. */
#define DDDMR_MAX_SOURCES 4
int dddmr_rollout_set_scan_source(dddmr_rollout_ctx* ctx, int32_t source_id, const float* xyz,
                                  size_t n_points, size_t stride_bytes, const double T_base_sensor[7],
                                  const double T_gbl_base[7], double perception_window_size,
                                  double marking_height, uint32_t* n_source_points,
                                  uint32_t* n_aggregate_points);
int dddmr_rollout_set_stitcher_source(dddmr_rollout_ctx* ctx, int32_t source_id, int32_t stitcher_num);

/* Depth camera as one more source of the aggregate = the local-mode side of DepthCameraLayer
   (dddmr_perception_3d/plugins/depth_camera/): what getObservation() (depth_camera_layer.cpp:618-663)
   hands the local planner.  Per frame, DepthCameraObservationBuffer::bufferCloud
   (depth_camera_observation_buffer.cpp:78-187) runs on the device: sensor->base transform, keep
   min_obstacle_height <= z <= max_obstacle_height (no x/y window, no range filter), only if more than
   20000 points survive a 0.05 m VoxelGrid centroid downsample in the base frame, base->global transform
   with the transform of THIS frame.  The observation is stamped stamp_ns (the caller's clock->now())
   truncated to whole microseconds, and purgeStaleObservations (:203-231) is applied literally with
   last_updated_ = stamp_ns: observation_persistence_ns == 0 keeps the newest frame only, otherwise a
   frame leaves when stamp_ns - its_stamp_truncated_to_us > observation_persistence_ns (int64, strict >).
   The source's observation = its alive frames, oldest first (older frames keep the global coordinates
   of their arrival); the aggregate = all sources in source order, as for dddmr_rollout_set_scan_source.
   The order of points inside one frame is unspecified.

   A raw frame is bounded by max_frame_points, not by max_points; the sources' observations together
   must fit max_points.  DDDMR_ERR_CAPACITY: frame > max_frame_points, more than max_frames observations
   alive, or the aggregate > max_points.  DDDMR_ERR_BAD_ARG: bad source id / stride, a frame for an
   unconfigured source, a depth call on a source that has been fed scans or given a stitcher, and
   dddmr_rollout_set_scan_source / set_stitcher_source on a depth source.  A failed call changes nothing:
   the source's frames, every source's size and the published aggregate stay what they were.
   dddmr_rollout_set_depth_source on a configured source empties it (the aggregate is republished without
   its points).  Configuring a depth source switches the context to the several-sensors mode: plain
   dddmr_rollout_set_scan then means source 0.

   Differences from the reference, on purpose: a record with ANY non-finite coordinate is dropped (as
   dddmr_rollout_set_scan does); the reference drops NaN z only and would keep a finite-z point with an
   infinite x.  Base-frame coordinates must stay within +-52 km (2^20 voxels of 0.05 m per axis).
   Limitation: dddmr_rollout_marking_update reads the context's aggregate as "the lidar observation";
   a context that feeds a marking layer must not carry depth sources. */
typedef struct {
  double min_obstacle_height, max_obstacle_height;
  int64_t observation_persistence_ns; /* 0 = newest frame only; the seconds -> Duration conversion stays with the caller */
  uint32_t max_frame_points;          /* raw points per frame, e.g. 848 * 480 */
  uint32_t max_frames;                /* observations alive at once */
} dddmr_depth_source_config;

int dddmr_rollout_set_depth_source(dddmr_rollout_ctx* ctx, int32_t source_id,
                                   const dddmr_depth_source_config* cfg);
/* *n_frame_points: points of this frame's observation; *n_source_points: the source's alive frames
   together; *n_aggregate_points: the published aggregate (each may be NULL). */
int dddmr_rollout_set_depth_frame(dddmr_rollout_ctx* ctx, int32_t source_id, const float* xyz,
                                  size_t n_points, size_t stride_bytes, const double T_base_sensor[7],
                                  const double T_gbl_base[7], int64_t stamp_ns, uint32_t* n_frame_points,
                                  uint32_t* n_source_points, uint32_t* n_aggregate_points);

/* Depth IMAGE sources: the image as the camera publishes it goes to the device, which does what the
   reference's own node in front of the layer does (DepthImg2PointCloud::cbDepthImg,
   dddmr_perception_3d/utils/depthimg2pointcloud_node.cpp:96-157) and then bufferCloud as above, in one call.
   Stage one, per image: 16UC1 only (the node reads unsigned shorts whatever the encoding says), rows may
   be padded; float cx = K[2], cy = K[5], fx = 1 / K[0], fy = 1 / K[4] (double division, float result);
   for v = 0, step, ... < height and u = 0, step, ... < width: float z = d * 0.001 (double product), the
   pixel is skipped when (double)z > max_distance, else x = ((float)u - cx) * z * fx,
   y = ((float)v - cy) * z * fy in float, nothing fused; then pcl::VoxelGrid with leaf_size in the optical
   frame (membership floor(p * (1.0f / (float)leaf_size)), centroid = sum / count; the device sums in
   double).  The order of the points is unspecified.  Stage two: exactly what dddmr_rollout_set_depth_frame
   does with a cloud, applied to stage one's centroids, T_base_optical taking them to the base frame.
   Every rule stated above for cloud frames holds for images.

   A pixel of depth 0 is KEPT, as the node keeps it (it only tests isnan(z) || z > max_distance): every
   pixel without a return becomes the point (0, 0, 0) of the optical frame, all of them end in one voxel,
   and only the height band removes that point, when the camera sits outside the band.
   Difference from the reference, on purpose: with DDDMR_DEPTH_IMAGE_DROP_ZERO such pixels are dropped.
   pcl::VoxelGrid returns its input unchanged when its voxel box has more than INT_MAX cells; that is not
   restated: dddmr_rollout_set_depth_image_source refuses (DDDMR_ERR_BAD_ARG) any intrinsics, max_distance
   and leaf_size whose worst-case frustum box (every pixel anywhere between depth 0 and
   min(max_distance, 65.535 m)) could reach 2^31 cells or 2^20 cells from the origin along an axis.

   A source is configured either for clouds (dddmr_rollout_set_depth_source) or for images; feeding it the
   other kind is DDDMR_ERR_BAD_ARG, as are sample_step 0, unknown flags, a row stride below 2 * width and
   a max_frame_points (of dddmr_depth_source_config: for an image source it bounds the sampled pixels)
   below ceil(height / sample_step) * ceil(width / sample_step).  Re-configuring a source with either
   call empties it. */
#define DDDMR_DEPTH_IMAGE_DROP_ZERO 1u
typedef struct {
  uint32_t width, height;        /* pixels */
  double fx, fy, cx, cy;         /* CameraInfo K[0], K[4], K[2], K[5] */
  double max_distance;           /* node parameter, default 4.0 (shipped launch: 6.0) */
  double leaf_size;              /* node parameter, default 0.05 */
  uint32_t sample_step;          /* node parameter, default 2 (shipped launch: 4); >= 1 */
  uint32_t flags;                /* DDDMR_DEPTH_IMAGE_* */
} dddmr_depth_image_config;

int dddmr_rollout_set_depth_image_source(dddmr_rollout_ctx* ctx, int32_t source_id,
                                         const dddmr_depth_source_config* cfg,
                                         const dddmr_depth_image_config* image_cfg);
/* depth_mm: height rows of row_stride_bytes, width uint16 millimetres each.  *n_camera_points: stage
   one's points (what the node would publish); the other counts as for dddmr_rollout_set_depth_frame
   (each may be NULL). */
int dddmr_rollout_set_depth_image(dddmr_rollout_ctx* ctx, int32_t source_id, const uint16_t* depth_mm,
                                  size_t row_stride_bytes, const double T_base_optical[7],
                                  const double T_gbl_base[7], int64_t stamp_ns, uint32_t* n_camera_points,
                                  uint32_t* n_frame_points, uint32_t* n_source_points,
                                  uint32_t* n_aggregate_points);
/* The stage-one cloud of the source's latest accepted image, optical frame, packed x y z: the node's
   point_cloud_from_depth topic.  xyz_out == NULL only reports *n_points. */
int dddmr_rollout_get_depth_image_cloud(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyz_out,
                                        size_t capacity, size_t* n_points);

/* Lidar SWEEP sources: the raw sweep as the lidar publishes it goes to the device, which does what the reference's
   own node in front of the lidar plugins does and then cbSensor, in one call (additions to ABI version 2; no
   existing struct or entry changes).  Every shipped configuration points its multilayer_spinning_lidar plugins at
   the topic segmented_cloud_pure, which ImageProjection::cloudHandler produces
   (dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp:280-314; line numbers below are that file's).

   Stage one, per sweep, with the casts of the member types (imageProjection.h:67-107): the parameters are stored
   into float members; _ang_resolution_X = (M_PI * 2) / H, _ang_resolution_Y = DEG_TO_RAD * (top - bottom) /
   float(V - 1) and _ang_bottom = -(bottom - 0.1) * DEG_TO_RAD are computed in double and stored as floats;
   tan(_segment_theta), sin(alpha) and cos(alpha) are taken once with the float overloads.
     pitch removal (:297-303)   q.setRPY(0, sensor_mount_angle, 0) as an Affine3d, pcl::transformPointCloud: double
                                multiply-add, float result, nothing fused.
     projection (:328-382)      range = float sqrt of float products; rowIdn = int((asin(z / range) + _ang_bottom) /
                                _ang_resolution_Y), truncated toward zero (quotients in (-1, 0) land in row 0);
                                columnIdn = int(-round(atan2(x, y) / _ang_resolution_X) + H * 0.5), one -= H wrap;
                                the bounds tests and minimum <= range <= maximum come before the pixel is written;
                                among several points of one pixel the LAST in input order wins.
     ground (:415-443, :519-526) for i < ground_scan_index, pixels (i, j) and (i + 1, j): float
                                atan2(dZ, sqrt(dX^2 + dY^2 + dZ^2)), ground when (angle + sensor_mount_angle) <=
                                10 * DEG_TO_RAD in double; an empty pixel holds NaN and makes no ground pair; a
                                ground pair marks both pixels.  label = -1 where a pixel is ground or empty.
     segments (:538-540, :595-679) neighbours (0,-1) (-1,0) (1,0) (0,1), columns wrap, rows do not; two pixels join
                                when d2 * sin(alpha) / (d1 - d2 * cos(alpha)) > tan(theta) in float, d1 / d2 the
                                larger / smaller range.  Each BFS fills one connected component; it is valid with
                                >= 30 pixels, or with >= segment_valid_point_num pixels on >= segment_valid_line_num
                                lines, where the seed's row counts only if the component has a second pixel in it
                                (lineCountFlag is set for pushed neighbours only).  Valid components are numbered
                                1, 2, ... in the raster order of their first pixels; invalid ones get 999999.
     output (:582-592)          the pixels with 0 < label != 999999 in raster order: x y z of the pitch-removed point
                                and the label as a float, 16 bytes per point = the topic segmented_cloud_pure.
   Stage two: exactly what dddmr_rollout_set_scan_source does with a cloud, applied to stage one's x y z without the
   cloud leaving the device.  T_base_sensor takes the frame "<sensor>_pitch_removed" (the frame the node stamps) to
   the base.  Every rule stated for scan sources holds; a sweep source counts as a lidar source for
   dddmr_rollout_marking_update and the perception stack.

   Differences from the reference, on purpose: a record with ANY non-finite coordinate is dropped
   (removeNaNFromPointCloud trusts is_dense); a point whose row quotient is not a number (range 0) is dropped (the
   reference converts NaN to int); an empty sweep yields an empty cloud (the reference reads points.front()).
   Left out: the patched ground cloud and its VoxelGrid (:450-514, it feeds mapping), the projected image, and the
   stitcher on sweep sources.  segmented_cloud and _seg_msg's arrays come with the sweep's features
   (dddmr_rollout_set_lidar_sweep_features below), findStartEndAngle and outlier_cloud with the sweep's association
   (dddmr_rollout_set_lidar_sweep_association), each off unless asked for.

   A source is configured for scans, for sweeps or for depth; feeding it another kind is DDDMR_ERR_BAD_ARG, as are
   dddmr_rollout_set_stitcher_source on a sweep source (a limit of this version), V < 2, H < 4, ground_scan_index >= V,
   top <= bottom, minimum range >= maximum range and unknown flags.  DDDMR_ERR_CAPACITY: V > 128, H > 4096,
   V * H > 2^19 or max_sweep_points > 2^20 at configuration; n_points > max_sweep_points or the aggregate exceeding
   max_points at a sweep.  A failed call changes nothing.  Re-configuring a source empties it. */
typedef struct {
  uint32_t num_vertical_scans, num_horizontal_scans;   /* laser.num_vertical_scans / num_horizontal_scans */
  double vertical_angle_bottom, vertical_angle_top;    /* degrees, as the YAML gives them */
  uint32_t ground_scan_index;                          /* < num_vertical_scans */
  double segment_theta;                                /* degrees */
  uint32_t segment_valid_point_num, segment_valid_line_num;
  double minimum_detection_range, maximum_detection_range;
  double sensor_mount_angle;     /* radians: the pitch the node reads from base->sensor (:212-214); the lookup stays with the caller */
  uint32_t max_sweep_points;     /* raw points per sweep */
  uint32_t flags;                /* 0 */
} dddmr_lidar_sweep_config;

int dddmr_rollout_set_lidar_sweep_source(dddmr_rollout_ctx* ctx, int32_t source_id,
                                         const dddmr_lidar_sweep_config* cfg);
/* *n_segmented: stage one's points (what the node would publish); *n_source_points / *n_aggregate_points as for
   dddmr_rollout_set_scan_source (each may be NULL). */
int dddmr_rollout_set_lidar_sweep(dddmr_rollout_ctx* ctx, int32_t source_id, const float* xyz, size_t n_points,
                                  size_t stride_bytes, const double T_base_sensor[7], const double T_gbl_base[7],
                                  double perception_window_size, double marking_height, uint32_t* n_segmented,
                                  uint32_t* n_source_points, uint32_t* n_aggregate_points);
/* Stage one's results for the source's latest accepted sweep; before the first one: zero points, an empty image.
   DDDMR_ERR_STATE on a source that is not a sweep source.  get_lidar_sweep_cloud: x y z label, 16 bytes per point;
   xyzl_out == NULL only reports *n_points.  get_lidar_sweep_image: V * H pixels each, row-major; FLT_MAX in the range
   image means empty, the ground mask is 1 for ground and 0 otherwise; each output may be NULL. */
int dddmr_rollout_get_lidar_sweep_cloud(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyzl_out, size_t capacity,
                                        size_t* n_points);
int dddmr_rollout_get_lidar_sweep_image(dddmr_rollout_ctx* ctx, int32_t source_id, float* range_out,
                                        int32_t* label_out, int8_t* ground_out, size_t capacity_pixels);

/* Lidar sweep FEATURES: the feature half of the reference's mcl_feature_node on a sweep source (additions to ABI
   version 2; no existing struct or entry changes; a sweep source whose features were never switched on runs exactly
   the launches it ran before).  In localisation mode the reference runs ImageProjection and the first four steps of
   FeatureAssociation::runFeatureAssociation (dddmr_lego_loam/lego_loam_bor/src/featureAssociation.cpp:1506-1514) and
   publishes laser_cloud_sharp / _less_sharp / _flat / _less_flat; mcl_3dl's cbLeGoFeatureCloud uses flat and less
   sharp, which dddmr_rollout_mcl_measure takes.  With features on, each accepted dddmr_rollout_set_lidar_sweep also
   yields, without a host wait of its own (line numbers: imageProjection.cpp for the first item, featureAssociation.cpp
   after it; float where the member is float, double where the literal is double, nothing fused):
     segmented cloud (imageProjection.cpp:542-580)  pixels in raster order with label > 0 or ground, without label
                                999999 (the outlier cloud is left out) and without the ground pixels with j % 5 != 0 &&
                                j > 5 && j < H - 5; per point the ground flag, the column, the range and the
                                pitch-removed point; per row start_ring_index = count_before - 1 + 5 and
                                end_ring_index = count_after - 1 - 5 (an empty row: start > end).
     smoothness (:318-341)      for 5 <= i < n - 5 the ten neighbours' ranges and -range[i] * 10 summed left to right
                                in float, in the source's order; curvature = d * d.
     occlusion (:343-379)       for 5 <= i < n - 6, columnDiff < 10: float differences against the double 0.3 mark
                                i - 5 .. i or i + 1 .. i + 6; both neighbour differences above the double 0.02 * range
                                mark i.  The marks cross ring boundaries.
     extraction (:381-491)      per ring six sixths sp .. ep with the source's integer divisions, sp >= ep skips one;
                                std::sort covers [sp, ep) and both walks include k = ep, whose slot is
                                {curvature[ep], ep}.  Edge walk, descending: not picked, curvature > edge_threshold,
                                not ground; candidates 1-2 are sharp and less sharp, 3-20 less sharp, the 21st breaks.
                                Flat walk, ascending: not picked, curvature < surf_threshold, ground; the 4th is
                                pushed and breaks before it suppresses.  A pick suppresses ind +- 1 .. 5 up to the
                                first step whose column difference is > 10, across sixths and one index before the
                                ring's first point.  The cloudLabel / less-flat loop and its VoxelGrid are left out.
     output (:281-314, :1384-1405) the camera-frame point (y, z, x) of the segmented point through T_out as
                                pcl::transformPointCloud(Affine3d) applies it (double multiply-add, float result);
                                the fourth float is the ring, float(int(intensity)); order = the reference's push
                                order: ring, sixth, walk order.
   T_out is publishCloud's trans_c2s.inverse(), row-major 3 x 4; the caller computes it (Eigen / NumPy).

   Differences from the reference, on purpose.  Every sweep behaves like the FIRST sweep of a freshly constructed
   FeatureAssociation: the reference never rewrites slot 4 of cloudSmoothness (ring 0's sp, below calculateSmoothness's
   range) and carries its sorted leftover from sweep to sweep; here slot 4 is {0.0f, ind 0} every time, so a ground
   point at segment index 0 is ring 0's first flat pick unless it is occlusion-marked.  Equal curvatures sort by
   ascending index (std::sort leaves their order undefined).  Left out HERE: the relTime part of the intensity,
   findStartEndAngle and less flat (mcl_3dl overwrites or ignores the intensity and never reads less flat); they come
   with dddmr_rollout_set_lidar_sweep_association below, and these entries stay as they are with it on.  What
   cbLeGoFeatureCloud does with the lists (VoxelGrid, normals, clusters) is dddmr_rollout_mcl_prepare_from_sweep,
   which reads them where they lie.

   The features are part of the sweep's double-buffered result: built beside the current one and swapped in only when
   the aggregate accepted the sweep, so after a refused sweep the getters return the previous sweep's.  cfg == NULL
   switches them off; new parameters on a source that has them on hold from the next sweep.  Re-configuring the sweep
   source switches them off.  DDDMR_ERR_BAD_ARG: a non-finite or negative threshold, a non-finite T_out entry, unknown
   flags, `which` outside 0 .. 2.  DDDMR_ERR_STATE: not a sweep source, or its features are off.  The getters follow
   the sweep getters: NULL outputs only report the count (each output may be NULL on its own), DDDMR_ERR_CAPACITY
   when a point output is wanted and capacity is below the count, a failed call changes nothing.  start / end ring
   indices: num_vertical_scans entries each.  Before the first sweep: zero points. */
typedef struct {
  double edge_threshold, surf_threshold; /* featureAssociation.*; stored into float members as the node does */
  double T_out[12];                      /* row-major 3x4, applied to the camera-frame point: publishCloud's
                                            trans_c2s.inverse(); the caller computes it (Eigen / NumPy) */
  uint32_t flags;                        /* 0 */
} dddmr_lidar_features_config;

int dddmr_rollout_set_lidar_sweep_features(dddmr_rollout_ctx* ctx, int32_t source_id,
                                           const dddmr_lidar_features_config* cfg); /* NULL: off */
int dddmr_rollout_get_lidar_sweep_segmented(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyz, float* range,
                                            int32_t* col_ind, uint8_t* ground_flag, int32_t* start_ring_index,
                                            int32_t* end_ring_index, size_t capacity, size_t* n);
/* which: 0 sharp, 1 less sharp, 2 flat.  xyzr_out: x y z ring, 16 bytes per point; seg_index_out: the point's index in
   the segmented cloud. */
int dddmr_rollout_get_lidar_sweep_features(dddmr_rollout_ctx* ctx, int32_t source_id, int which, float* xyzr_out,
                                           uint32_t* seg_index_out, size_t capacity, size_t* n_points);

/* Lidar sweep ASSOCIATION: the rest of the front half of LeGO-LOAM's feature node on a sweep source whose features
   are on (additions to ABI version 2; no existing struct or entry changes; with the association off a sweep launches
   exactly what it launched before and every other output is byte-equal).  It is what the host FeatureAssociation and
   mapOptimization take besides the three feature lists when odom_type is "laser_odometry" or the node maps.  Line
   numbers: dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp (ip) and src/featureAssociation.cpp (fa).
     orientation (ip:391-406, findStartEndAngle)  start = -atan2f(y, x) of the first record of the pitch-removed cloud,
                                end = -atan2f(y, x) of the last one + 2 * M_PI; end - start > 3 * M_PI takes 2 * M_PI off,
                                < M_PI adds it; diff = end - start.  The three are float32 message fields: atan2f and
                                the differences are float, M_PI sums and comparisons double, each stored back into the
                                float.  First and last are the first and last records the ingest keeps as finite (it
                                drops non-finite records on purpose).  An empty sweep: zeros.
     point times (fa:281-314, adjustDistortion, the part the features leave out)  per segmented point, in index order:
                                ori = -atan2f(seg.y, seg.x) in float; while halfPassed is false, ori < start - M_PI / 2
                                adds 2 * M_PI, ori > start + M_PI * 3 / 2 takes it off (double comparisons, the sum
                                rounded to float), and ori - start > M_PI sets halfPassed for the points BEHIND this one;
                                then ori += 2 * M_PI, ori < end - M_PI * 3 / 2 adds 2 * M_PI, ori > end + M_PI / 2 takes
                                it off.  relTime = (ori - start) / diff in float; intensity = float(double(ring) +
                                scan_period * double(relTime)).  half_index is the index at which the flag flips
                                (the last point of the first branch), the number of segmented points when it never does.
     less flat (fa:486-514)     per ring the segment indices k of [sp, ep], ep included, of every sixth that was not
                                skipped, with cloudLabel[k] <= 0 (not one of the ring's sharp or less-sharp picks; labels
                                never written are 0, as for the features), ascending; then pcl::VoxelGrid, leaf 0.2
                                (fa:124), on the ring's candidates in the association frame: inverse leaf 1 / 0.2f in
                                float, floor, min_b from the ring's own candidates, output in voxel-index order
                                x + y dx + z dx dy, points of a voxel summed in input order in float and divided by the
                                count; the intensity is averaged the same way (an assumption).  PCL's
                                overflow rule: with d = int64((max - min) * inverse_leaf) + 1 per axis, dx * dy * dz
                                above INT32_MAX hands the ring's candidates through unchanged.  Rings in ring order.
     outliers (ip:548-558)      pixels with label 999999, row > ground_scan_index and col % 5 == 0 in raster order: the
                                pitch-removed point, intensity float(double(float(row)) + double(float(col)) / 10000.0)
                                (ip:376).  adjustOutlierCloud's axis change stays with the caller.
     the four clouds            sharp, less sharp, flat (the features' lists, the same points in the same order) and
                                less flat, frame 0: the association frame, (y, z, x) of the segmented point untransformed,
                                as extractFeatures holds them; frame 1: through the features' T_out as publishCloud
                                publishes them (fa:1401-1404; transformPointCloud carries the intensity through).  The
                                intensity is the point time; for less flat the voxel's average.
   Left out: updateTransformation and everything behind it (the scan matcher), the patched ground, the projected image.

   It is part of the sweep's double-buffered result as the features are: it holds from the next sweep, and after a
   refused sweep the getters return the previous sweep's.  enable == 0, switching the features off and re-configuring
   the source switch it off.  DDDMR_ERR_STATE: not a sweep source, its features are off, or (getters) the association
   is off.  DDDMR_ERR_BAD_ARG: a scan_period that is negative or not finite, `which` outside 0 .. 3, `frame` outside
   0 .. 1.  The getters follow the feature getters: NULL outputs only report the count, DDDMR_ERR_CAPACITY when an
   output is wanted and capacity is below the count, a failed call changes nothing, before the first sweep zero points
   (orientation: zeros, half_index 0).  get_lidar_sweep_times: one intensity per segmented point.  seg_index_out: the
   point's index in the segmented cloud; for less flat the lowest index that went into the voxel.  16 bytes per point. */
int dddmr_rollout_set_lidar_sweep_association(dddmr_rollout_ctx* ctx, int32_t source_id, int32_t enable,
                                              double scan_period);
int dddmr_rollout_get_lidar_sweep_orientation(dddmr_rollout_ctx* ctx, int32_t source_id, float out[3],
                                              int32_t* half_index);
int dddmr_rollout_get_lidar_sweep_times(dddmr_rollout_ctx* ctx, int32_t source_id, float* intensity_out,
                                        size_t capacity, size_t* n);
/* which: 0 sharp, 1 less sharp, 2 flat, 3 less flat; frame: 0 association, 1 through T_out */
int dddmr_rollout_get_lidar_sweep_association(dddmr_rollout_ctx* ctx, int32_t source_id, int which, int frame,
                                              float* xyzi_out, uint32_t* seg_index_out, size_t capacity, size_t* n);
int dddmr_rollout_get_lidar_sweep_outliers(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyzi_out, size_t capacity,
                                           size_t* n);

/* Depth camera frustums and selfClear's clearing verdicts: the global-mode side of DepthCameraLayer, first slice
   (additions to ABI version 2; no existing struct or entry changes).

   dddmr_rollout_set_depth_frustum is the second half of DepthCameraObservationBuffer::bufferCloud
   (depth_camera_observation_buffer.cpp:134-174): call it once per frame beside dddmr_rollout_set_depth_frame /
   _set_depth_image with m2s = lookupTransform(global, origin_frame), which the reference looks up on its own (it is
   not derived from the frame call's transforms).  It REPLACES the source's frustum (the reference's tests only read
   observations.back()): findFrustumVertex (depth_camera_observation.cpp:114-127: d * tan(FOV / 2.0) in double, rounded
   into floats, order TLNear TRNear BLNear BRNear TLFar TRFar BLFar BRFar), pcl::transformPointCloud by the Affine3d of
   m2s (double multiply-add, float result), findFrustumNormal (:130-200, order near right bottom left far top),
   findFrustumPlane (:202-239), BRNear_ = vertex 3, TLFar_ = vertex 4, origin_ = m2s' translation (kept in double;
   dddmr_rollout_get_depth_frustum reports it rounded to float).  FOV_W / FOV_V in radians, inside (0, pi);
   0 < obstacle_min_range < obstacle_max_range (the plugin's parameter names; the reference's min_ / max_detect_distance_).
   DDDMR_ERR_STATE: the source is not a depth source (get: or has no frustum).  A refused call changes nothing.
   Re-configuring a source (dddmr_rollout_set_depth_source / _set_depth_image_source) drops its frustum with its frames.

   dddmr_rollout_depth_frustum_test: FrustumUtils::isinFrustumsObservations and isAttachFRUSTUMs (frustum_utils.cpp:124-290)
   for n points (records stride_bytes apart, float x y z first), one byte per point each (either output may be NULL),
   over the frustums of ALL depth sources in source order.  The reference iterates a std::map keyed by the source's
   name, so the caller numbers its depth sources in the order of their names.  The arithmetic is the reference's: every
   operand of the six `test` dot products, of the plane distance and of its fabs / sqrt is a float, so they are float
   expressions (`test` is widened to double only for `< 0`; fabs / sqrt are the float overloads, oracle/ASSUMPTIONS.md
   row 18); hypot(float - double, float - double) < max_detect_distance_ + 0.5 is double; dis2rej = (float)0.12.
   isAttachFRUSTUMs is decided by the first plane of the first source that attaches: true unless another source holds
   the point inside its frustum and unattached (isInsideFRUSTUMwoAttach); later planes and sources are not asked.

   dddmr_rollout_depth_clear_verdicts: the decision tree of DepthCameraLayer::selfClear (depth_camera_layer.cpp:324-422)
   for m markings the caller selected from its own pct_marking_ map (getXIter / lower_bound stay with the caller).
   Marking i has the voxel key voxel_xyz[i] and the stored cluster (pc_) cluster_xyz[offsets[i] .. offsets[i + 1]),
   packed x y z; offsets[0] = 0, offsets non-decreasing.  pt = (x * xy_resolution, y * xy_resolution,
   z * height_resolution), int times double rounded to float.  The observation is the concatenation of the DEPTH
   sources' alive frames as the context holds them now (aggregatePointCloudFromObservations; lidar sources of the same
   context do not enter); with <= 5 points it counts as clear and nothing is searched (:258-264).
     pt in no frustum (the branch at :333; its comment says the opposite): kept iff radiusSearch(pt, 0.05, 1) > 0.
     otherwise, attached (isAttachFRUSTUMs) or not, the same test: removed when the observation is clear, else
     engage = cluster points with radiusSearch(point, 0.01, 1) > 0, kept iff 1.0 * engage / size > 0.1 (double).
   radiusSearch is FLANN's float squared distance against static_cast<float>(r * r), strict < (oracle/ASSUMPTIONS.md row 1).
   verdict_out[i]: bit 0 = kept (the marking would be pushed to current_observation_ptr; 0 = removePCPtr), bits 1-2 =
   the branch that decided: 1 outside the frustums, 2 attached, 3 inside.  engaged_out[i] (may be NULL) = the
   engagement count where the branch computes one, else 0.  DDDMR_ERR_BAD_ARG when a marking reaches the ratio with
   an empty cluster (the reference would divide by zero); no output is written then.

   Both calls: DDDMR_ERR_STATE without a depth source or while a depth source has no frustum yet (the reference returns
   early until isFirstScanReady() of every buffer).  Both may be called between dddmr_rollout_tick_begin and _tick_end
   and give the same answer as outside: they work on the feeds' stream and read the depth sources, which a tick never
   touches.  They are serialised with the feeds (one producer at a time).  The observation grid is rebuilt only when a
   depth source has published since the last verdict call; dddmr_rollout_depth_clear_launches reports how many device
   operations (kernels, memsets, copies) the last verdict call enqueued.  Each call makes one host wait. */
typedef struct {
  double FOV_W, FOV_V;                            /* radians */
  double obstacle_min_range, obstacle_max_range;  /* metres */
} dddmr_depth_frustum_config;

int dddmr_rollout_set_depth_frustum(dddmr_rollout_ctx* ctx, int32_t source_id, const dddmr_depth_frustum_config* cfg,
                                    const double T_gbl_sensor[7]);
/* any output may be NULL */
int dddmr_rollout_get_depth_frustum(dddmr_rollout_ctx* ctx, int32_t source_id, float vertices[8][3], float normals[6][3],
                                    float planes[6][4], float origin[3]);
int dddmr_rollout_depth_frustum_test(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                                     uint8_t* in_frustums_out, uint8_t* attach_out);
int dddmr_rollout_depth_clear_verdicts(dddmr_rollout_ctx* ctx, double xy_resolution, double height_resolution,
                                       const int32_t* voxel_xyz /* [m][3] */, const uint32_t* offsets /* [m + 1] */,
                                       const float* cluster_xyz /* [offsets[m]][3] */, size_t m,
                                       uint8_t* verdict_out /* [m] */, uint32_t* engaged_out /* [m], may be NULL */);
int dddmr_rollout_depth_clear_launches(dddmr_rollout_ctx* ctx, uint32_t* launches_last_call);

/* Depth camera selfMark: the clusters addPCPtr is to be called with (additions to ABI version 2; no existing struct or
   entry changes).  The host keeps pct_marking_, addPCPtr and its dGraph; nothing is stored on the device between calls.

   dddmr_rollout_depth_mark_create copies pcl_ground_ and pcl_map_ to the device once and builds their search grids (the
   inputs of dddmr_rollout_marking_create; n_map may be 0).  It is independent of dddmr_rollout_marking_create: a context
   may have either, both or neither.  Calling it again replaces the state, which is freed with the context.
   DDDMR_ERR_BAD_ARG: a resolution or the tolerance is not positive and finite, a negative minimum cluster size,
   max_observation_points 0, a bad pointer / stride; DDDMR_ERR_CAPACITY: max_observation_points above 2^20;
   DDDMR_ERR_STATE: a dddmr_rollout_tick_begin is pending.  A refused call leaves the earlier state in place.

   dddmr_rollout_depth_mark_clusters is one DepthCameraLayer::selfMark from depth_camera_layer.cpp:487 on (the early
   returns above it stay with the caller, except isFirstScanReady: DDDMR_ERR_STATE before depth_mark_create, without
   a depth source or while a depth source has no frustum).  The observation is the DEPTH sources' alive frames in source
   order, exactly the one dddmr_rollout_depth_clear_verdicts searches; lidar sources of the context stay out.  With
   <= 5 points (:491) the call returns DDDMR_OK with n_accepted = 0; with more than max_observation_points,
   DDDMR_ERR_CAPACITY.  Then, as the reference does it:
     1. pcl::extractEuclideanClusters (oracle/ASSUMPTIONS.md rows 1, 2, 9): FLANN's float squared distance against
        static_cast<float>(tol * tol), strict <; clusters in order of their lowest point index, each cluster's indices
        ascending; kept iff min_cluster_size <= size (the maximum is the observation's size).
     2. the outputs follow std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters) (row 10), replayed on the
        host over the kept clusters' sizes in creation order: a caller that walks them front to back and calls addPCPtr
        ends with the reference's map, contested voxels included.
     3. centroid: float running sums of x, y, z in ascending point index, each divided by (float)size.
     4. dropped if a ground node lies within 0.1 of the centroid (:539; the lidar layer uses 0.05).
     5. pcl::VoxelGrid at 0.2 m (rows 7, 8): cell floorf(p * (1.0f / 0.2f)), output in voxel index order (x fastest), each
        point the float sum of its voxel's points in input order divided by the count.  This is cloud_cluster, the pc_ the
        verdict call is later fed.
     6. static map (:552-562): with segmentation_ignore_ratio <= 0.999 the loop searches with the CENTROID (radius 0.1) for
        every downsampled point and breaks once hit > size * ratio; kept iff hit <= size * ratio (size_t against double).
     7. isinFrustumsObservations(centroid) on the raw float centroid (:591), not on the voxel centre.
   Per accepted cluster i: centroid_out[i], voxel_out[i] = ((int)(cx / xy_resolution), (int)(cy / xy_resolution),
   (int)(cz / height_resolution)) (float divided by double, truncated, as addPCPtr does), size_out[i] = its size before
   downsampling, cluster_xyz_out[offsets_out[i] .. offsets_out[i + 1]) = its downsampled points.  plane_out = the
   ModelCoefficients of :568-578 (tf2::quatRotate(q, (0, 0, 1)) and d in double, rounded to float), the same for all.
   stats is always required.  The other outputs are all given or all NULL ("count only": stats alone is filled).  Too small
   a capacity: DDDMR_ERR_CAPACITY with stats filled (n_accepted, n_points are what is needed) and no other output written.
   A refused call changes nothing a later call can see.  One host wait; the call runs on the feeds' stream, serialised
   with the feeds, and may be made between dddmr_rollout_tick_begin and _tick_end with the serial answer.  It shares the
   observation grid of the verdict call: the two together rebuild it at most once per published frame. */
typedef struct {
  double xy_resolution, height_resolution;                 /* the layer's, for the voxel key only */
  double euclidean_cluster_extraction_tolerance;           /* plugin default 0.1 */
  int32_t euclidean_cluster_extraction_min_cluster_size;   /* plugin default 1 */
  int32_t reserved;
  double segmentation_ignore_ratio;
  uint32_t max_observation_points;                          /* depth observation the scratch is sized for */
  uint32_t reserved2;
} dddmr_depth_mark_config;

typedef struct {
  uint32_t n_observation;       /* points of the depth observation clustered */
  uint32_t n_clusters;          /* clusters extractEuclideanClusters returns (min size applied) */
  uint32_t n_ground_rejected;   /* centroid within 0.1 m of a ground node (:539) */
  uint32_t n_static_rejected;   /* hit > size * segmentation_ignore_ratio (:562) */
  uint32_t n_outside_frustums;  /* passed both, isinFrustumsObservations(centroid) false (:591) */
  uint32_t n_accepted;          /* clusters written */
  uint32_t n_points;            /* 0.2 m downsampled points written (= offsets[n_accepted]) */
  uint32_t launches;            /* device operations the call enqueued */
} dddmr_depth_mark_stats;

int dddmr_rollout_depth_mark_create(dddmr_rollout_ctx* ctx, const dddmr_depth_mark_config* cfg, const float* ground_xyz,
                                    size_t n_ground, size_t ground_stride_bytes, const float* map_xyz, size_t n_map,
                                    size_t map_stride_bytes);
int dddmr_rollout_depth_mark_clusters(dddmr_rollout_ctx* ctx, const double T_gbl_base[7], size_t capacity_clusters,
                                      size_t capacity_points, float* centroid_out /* [c][3] */, int32_t* voxel_out /* [c][3] */,
                                      uint32_t* size_out /* [c] */, uint32_t* offsets_out /* [c + 1] */,
                                      float* cluster_xyz_out /* [p][3] */, float plane_out[4], dddmr_depth_mark_stats* stats);

/* Depth camera layer on the device: marking store, dGraph and lethal set (additions to ABI version 2; no existing
   struct or entry changes).  One dddmr_rollout_depth_layer_update is one selfClear + selfMark + updateLethalPointCloud
   pass of the global-mode DepthCameraLayer (stacked_perception.cpp:82-88) with pct_marking_, its dGraph and lethal_map_
   kept in device memory between calls: only parameters go in and counters come out.

   dddmr_rollout_depth_layer_create takes the inputs of dddmr_rollout_depth_mark_create plus the layer's window, radii and
   capacities.  It is independent of depth_mark_create and of marking_create: a context may have any of them (dddmr_rollout_marking_update
   takes the whole aggregate, depth points included, as the lidar observation: a context with both kinds of sensors
   updates its layers through dddmr_rollout_stack_update, which gives each layer its own sensor's observation).  DDDMR_ERR_BAD_ARG: a
   resolution, the tolerance, the inflation radius, the window or the marking height is not positive and finite, a
   negative minimum cluster size, a capacity of 0, a bad pointer / stride; DDDMR_ERR_CAPACITY: max_observation_points
   above 2^20 or max_markings above 2^24; DDDMR_ERR_STATE: a dddmr_rollout_tick_begin is pending.  A refused call leaves
   the earlier state in place; a successful one replaces it (empty store, dGraph = max_obstacle_distance).

   dddmr_rollout_depth_layer_update runs on the feeds' stream, serialised with the feeds, and may be made between
   dddmr_rollout_tick_begin and _tick_end with the serial answer.  DDDMR_ERR_STATE before depth_layer_create, without a
   depth source or while a depth source has no frustum (the isFirstScanReady returns of depth_camera_layer.cpp:266-269 /
   :482-485; the other early returns stay with the caller).  More than max_observation_points: DDDMR_ERR_CAPACITY,
   nothing changed.
     selfClear (:252-426) against the CURRENT aggregated depth observation (the one depth_clear_verdicts searches, its
       grid rebuilt at most once per published frame; the lidar layer uses the previous one).  The window is in voxel
       keys, half open because of lower_bound: x, y in [(int)((t -+ perception_window_size) / xy_resolution)), z in
       [(int)((t.z -+ marking_height) / height_resolution)), double division, truncated.  Only alive markings
       (pc_ != nullptr) are looked at.  The verdict per marking is exactly dddmr_rollout_depth_clear_verdicts' (an
       observation of <= 5 points clears everything in the window); it reads the voxel key and the stored pc_ from the
       device store.
     removePCPtr (cluster_marking.cpp:125-138) for every marking not kept: every node of its nodes_of_min_distance_ gets
       clearValue(node, 9999.0), whether or not another alive marking covers the node, and leaves the lethal set where
       this marking's stored distance is <= inscribed_radius.  nodes_of_min_distance_ is recomputed from the marking's
       stored generator points.
     selfMark (:487-601): the pipeline of dddmr_rollout_depth_mark_clusters (with <= 5 observation points nothing is
       marked although selfClear ran).  Every accepted cluster then goes through addPCPtr (:100-123): the voxel slot
       (int)(c / resolution) is created or found; its pc_ (the 0.2 m cloud) and generator points are replaced by this
       cluster's, without a clearValue of the old ones; generator points = ProjectInliers on the plane of :568-578
       (float, Eigen's reduction order (a0 + a2) + (a1 + a3), the normal normalised) then the 0.1 m VoxelGrid; for
       every ground node within inflation_radius of one (FLANN float distance, strict <): setValue(node,
       sqrtf(dx^2 + dy^2)) as a minimum in double, lethal where <= inscribed_radius.  EVERY accepted cluster
       contributes to the dGraph and the lethal set, the losers of a contested voxel included.  A contested voxel keeps
       the cluster the reference processes last: std::sort(rbegin, rend) by size (oracle/ASSUMPTIONS.md row 10) -- a
       device priority (smaller size, then higher index) and, only in updates that have a contested voxel, the host's
       replay of that very sort (the code depth_mark_clusters orders its outputs with).
     updateLethalPointCloud is dddmr_rollout_depth_layer_get_lethal: ground points whose flag is set.
   Housekeeping as in the lidar layer: a cleared voxel keeps its key until half the table holds keys (then the alive
   markings move to a fresh table); overwritten pc_ / generator ranges are pool garbage until the pool is half used
   (then it is compacted).  DDDMR_ERR_CAPACITY from an update: the store (max_markings) or the pool (max_cluster_points)
   overflowed, or a cluster point lies beyond the VoxelGrid key range around the robot.  The update has then run to its
   end: selfClear is complete, every accepted cluster has contributed to the dGraph and the lethal set, but a cluster
   that found no slot or no pool space is not stored, so a later selfClear cannot take its contribution back; its voxel
   is not alive afterwards, ALSO where a marking stored by an earlier update was alive on that voxel: that marking is
   gone without a clearValue.  dddmr_rollout_depth_layer_reset recovers a usable, empty layer.
   An update makes ONE host wait, a second one only when two accepted clusters contest a voxel (stats.host_waits).

   The getters take the same lock and order themselves after the update's stream.  get_voxels: the alive markings' voxel
   keys (xyz_out NULL: count only).  get_clusters: the alive markings with their stored pc_, voxel_out[i] and
   xyz_out[offsets_out[i] .. offsets_out[i + 1]); all outputs NULL: counts only; too small a capacity:
   DDDMR_ERR_CAPACITY with the counts filled.  Order: by store slot.  get_dgraph: n_ground + 1 doubles; get_lethal: one
   byte per ground node (n_ground + 1, the last unused). */
typedef struct {
  double xy_resolution, height_resolution;
  double marking_height, perception_window_size;
  double euclidean_cluster_extraction_tolerance;           /* plugin default 0.1 */
  int32_t euclidean_cluster_extraction_min_cluster_size;   /* plugin default 1 */
  int32_t reserved;
  double segmentation_ignore_ratio;
  double inscribed_radius, inflation_radius, max_obstacle_distance;
  uint32_t max_observation_points;                          /* depth observation the scratch is sized for */
  uint32_t max_markings;                                    /* voxels of the store */
  uint32_t max_cluster_points;                              /* pool: stored pc_ + generator points */
  uint32_t reserved2;
} dddmr_depth_layer_config;

typedef struct {
  uint32_t n_observation;       /* points of the depth observation */
  uint32_t n_in_window;         /* alive markings selfClear looked at */
  uint32_t n_cleared;           /* of them removed */
  uint32_t n_clusters;          /* clusters extractEuclideanClusters returns (min size applied) */
  uint32_t n_accepted;          /* addPCPtr calls */
  uint32_t n_contested;         /* of them on a voxel another cluster of this update had already claimed */
  uint32_t n_alive;             /* alive markings after the update */
  uint32_t gc_runs;             /* store rehash / pool compaction done by this update */
  uint32_t launches;            /* device operations the update enqueued; approximate: the library's own launches are
                                   counted, rocPRIM's sorts and scans are entered with an estimate */
  uint32_t host_waits;
} dddmr_depth_layer_stats;

int dddmr_rollout_depth_layer_create(dddmr_rollout_ctx* ctx, const dddmr_depth_layer_config* cfg, const float* ground_xyz,
                                     size_t n_ground, size_t ground_stride_bytes, const float* map_xyz, size_t n_map,
                                     size_t map_stride_bytes);
int dddmr_rollout_depth_layer_update(dddmr_rollout_ctx* ctx, const double T_gbl_base[7], dddmr_depth_layer_stats* stats);
/* resetdGraph: empty store, dGraph = max_obstacle_distance */
int dddmr_rollout_depth_layer_reset(dddmr_rollout_ctx* ctx);
int dddmr_rollout_depth_layer_get_voxels(dddmr_rollout_ctx* ctx, int32_t* xyz_out /* [capacity][3] */, size_t capacity, size_t* n);
int dddmr_rollout_depth_layer_get_clusters(dddmr_rollout_ctx* ctx, int32_t* voxel_out /* [m][3] */, uint32_t* offsets_out /* [m + 1] */,
                                           float* xyz_out /* [p][3] */, size_t cap_markings, size_t cap_points,
                                           size_t* n_markings, size_t* n_points);
int dddmr_rollout_depth_layer_get_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity);
int dddmr_rollout_depth_layer_get_lethal(dddmr_rollout_ctx* ctx, uint8_t* flags_out, size_t capacity);

/* Copy the current aggregate observation back (debug / parity of set_scan). */
int dddmr_rollout_get_cloud(dddmr_rollout_ctx* ctx, float* xyzi_out, size_t capacity,
                            size_t* n_points);

/* Prune plan = output of Local_Planner::prunePlan (local_planner.cpp:374-445);
   poses are x y z qx qy qz qw in the global frame. */
int dddmr_rollout_set_prune_plan(dddmr_rollout_ctx* ctx, const double* poses_xyz_qxyzw,
                                 size_t n_poses);

/* Perception opinions (dddmr_perception_3d/include/perception_3d/sensor.h, PerceptionOpinion). */
typedef enum {
  DDDMR_OPINION_PASS = 0,
  DDDMR_OPINION_PATH_BLOCKED_WAIT = 1
} dddmr_perception_opinion;

/* PathBlockedStrategy::selfMark
   (dddmr_perception_3d/plugins/path_blocked_strategy.cpp:56-100) on the current aggregate
   observation: plan_xyzi is pcl_prune_plan_ as Local_Planner::prunePlan fills it
   (local_planner.cpp:402-430: n_points records x,y,z,intensity, backward points tagged
   intensity < 0).  *blocked_ratio_percent = blocked forward points / n_points * 100,
   *opinion = PATH_BLOCKED_WAIT when that is > 0 (computeVelocityCommand then returns
   dddmr_sys_core::PATH_BLOCKED_WAIT, local_planner.cpp:597-602).  blocked_flags (may be
   NULL) receives one byte per plan point.  Replaces the second per-tick kd-tree build on
   the observation (:68-70). */
int dddmr_rollout_path_blocked(dddmr_rollout_ctx* ctx, const float* plan_xyzi, size_t n_points,
                               double check_radius, double* blocked_ratio_percent, int32_t* opinion,
                               uint8_t* blocked_flags);

/* The theory's initialise() alone (dd_simple...cpp:236-295, omni_simple...cpp:260-332,
   dd_rotate_inplace_theory.cpp:229-274): the velocity samples a tick with these inputs rolls out, in
   generation order, samples_out[n][3] = vx vy wz.  Host-only (no device work); call with NULL for the
   count.  An iterator-protocol adapter (hasMoreTrajectories / nextTrajectory) needs the list before the
   batch has been scored. */
int dddmr_rollout_samples(dddmr_rollout_ctx* ctx, const char* theory_name, const dddmr_tick_input* in,
                          float* samples_out, size_t capacity, size_t* n_samples);

/* One control tick for the named theory. */
int dddmr_rollout_tick(dddmr_rollout_ctx* ctx, const char* theory_name,
                       const dddmr_tick_input* in, dddmr_rollout_result* out);

/* Split form of dddmr_rollout_tick for hosts that want to overlap their own work
   (e.g. the previous tick's all-reduce) with the GPU: tick_begin enqueues the
   tick and returns at once, tick_end waits for it and fills the result.  Exactly
   one tick may be pending per context; set_prune_plan / tick / get_* return
   DDDMR_ERR_STATE while one is.  set_cloud / set_scan stay allowed, any number of
   times, from any thread (they fill a free buffer; the pending tick keeps the
   observation it started with).  dddmr_rollout_tick == tick_begin + tick_end. */
int dddmr_rollout_tick_begin(dddmr_rollout_ctx* ctx, const char* theory_name,
                             const dddmr_tick_input* in);
int dddmr_rollout_tick_end(dddmr_rollout_ctx* ctx, dddmr_rollout_result* out);

/* Multi-rank hosts: every rank ticks its shard, then ONE small min all-reduce
   picks the global winner and every rank resolves its command from the index.

   Exact form (use this one): rank r contributes two int64 words, dddmr_rollout_winner_words
   = { bit pattern of its best cost, -best_index } (INT64_MAX, INT64_MAX when its shard has no
   acceptable trajectory).  All-reduce with MIN a vector of 2*n_ranks words in which rank r fills
   slots [2r, 2r+1] and leaves INT64_MAX elsewhere (16*n_ranks bytes, latency-bound), then call
   dddmr_rollout_resolve_words on every rank: minimum cost compared as full doubles, equal costs
   -> highest index, exactly the reference's `<=` scan over the whole batch
   (local_planner.cpp:456-463).

   8-byte form: min-reduce result.key (dddmr_rollout_pack_key) and call dddmr_rollout_resolve.
   The key carries the top 40 bits of the cost, so across ranks costs closer than 3.7e-9
   relative resolve to the higher index; inside one shard the winner is always exact. */
int dddmr_rollout_resolve(dddmr_rollout_ctx* ctx, int64_t reduced_key,
                          dddmr_rollout_result* inout);
void dddmr_rollout_winner_words(const dddmr_rollout_result* r, int64_t words[2]);
int dddmr_rollout_resolve_words(dddmr_rollout_ctx* ctx, const int64_t* words, int32_t n_ranks,
                                dddmr_rollout_result* inout);

/* In-library exchange (SURVEY.md 8b "Context owns ... RCCL communicators", 8e): a C++ host needs no
   collective code of its own.  One rank calls dddmr_rollout_comm_unique_id (ncclGetUniqueId) and
   hands the 128 bytes to the others by any means it has; every rank then calls
   dddmr_rollout_comm_init with the rank / n_ranks its context was created with (collective:
   ncclCommInitRank, one process per GPU, RCCL over xGMI).  From then on every tick of the context
   runs, on the context's stream, k_score -> ONE ncclAllReduce(ncclInt64, ncclMin) of the 2*n_ranks
   slot vector described above -> a resolve kernel, and dddmr_rollout_tick / tick_end return the
   GLOBAL winner (best_index, exact best_cost, command) on every rank; `key` is the global winner's
   packed key, n_local / local_begin still describe the shard.  All ranks must tick in lockstep (same
   theory, same inputs): the all-reduce is a collective.  librccl is loaded at run time
   (DDDMR_RCCL_LIB overrides the search), so hosts that never call this need no RCCL.
   dddmr_rollout_comm_destroy returns the context to single-rank results (the host-side
   resolve_words path keeps working either way). */
int dddmr_rollout_comm_unique_id(uint8_t id_out[DDDMR_COMM_ID_BYTES]);
int dddmr_rollout_comm_init(dddmr_rollout_ctx* ctx, const uint8_t id[DDDMR_COMM_ID_BYTES],
                            int32_t rank, int32_t n_ranks);
int dddmr_rollout_comm_destroy(dddmr_rollout_ctx* ctx);
/* HIP devices this process sees (hipGetDeviceCount): what a multi-GPU host places its contexts by
   (`cfg.device`); the reference has no counterpart (one CPU process per robot). */
int dddmr_rollout_device_count(int32_t* n_out);
/* Ranks of the context's exchange as the communicator itself reports them (ncclCommCount), 0 without
   one: what a multi-GPU run prints next to its numbers. */
int dddmr_rollout_comm_ranks(dddmr_rollout_ctx* ctx, int32_t* n_ranks_out);
/* Single-device rehearsal of the exchange (RCCL refuses two ranks on one GPU): the context, created
   as rank r of W, runs the same k_score -> slot vector -> resolve-kernel sequence on its stream with
   the all-reduce replaced by a device copy of its own send vector; the peers' (cost bits, -index)
   pairs (dddmr_rollout_winner_words of their ticks) are written into it by the host.  Exercises
   exactly the device code a W-rank communicator runs, including ranks whose shard is empty. */
int dddmr_rollout_comm_loopback(dddmr_rollout_ctx* ctx);
int dddmr_rollout_comm_loopback_set_peer(dddmr_rollout_ctx* ctx, int32_t peer_rank, const int64_t words[2]);

/* Per-trajectory outputs of the last tick (any pointer may be NULL). */
int dddmr_rollout_get_debug(dddmr_rollout_ctx* ctx, dddmr_rollout_debug* dbg);

/* How the last launched tick rolled its headings out: 1 one row of headings per angular sample, shared by the
   sample's trajectories (grid ticks with a fixed step count whose shard holds enough members of every angular
   sample; DDDMR_HEADING_ROWS=0 at create switches it off), 0 a heading chain per trajectory, -1 before any tick.
   Both give the same bits; tests use this to know which path they compared. */
int dddmr_rollout_heading_rows(dddmr_rollout_ctx* ctx);

/* How the last launched tick searched the prune plan for the path critics: 1 as the tail of the collision walk, wave
   by wave with no barrier in between, for every (trajectory, step) pair (lean 512-lane launches with more than 256 and at most 512 pairs a workgroup, a cloud of
   at least 5 points, a plan, and a previous tick of which at most 1 - 256 / pairs of the trajectories collided;
   DDDMR_FUSE_WALK=0 at create switches it off), 0 as a phase of its own for the surviving trajectories, -1 before any
   tick.  Both give the same bits; tests use this to know which path they compared. */
int dddmr_rollout_fused_walk(dddmr_rollout_ctx* ctx);

/* Which optional paths the last launched tick's k_score took, as bits: bit 0 = the fused plan walk and the StickPath
   sums left out the trajectories the collision walk had rejected (fused ticks only; DDDMR_SKIP_DEAD=0 at create
   switches it off).  0 on a tick that is not fused or has an empty shard, -1 before any tick.  Either way gives the
   same bits; tests use this to know which path they compared. */
int dddmr_rollout_score_paths(dddmr_rollout_ctx* ctx);

/* How the last launched tick's load-feedback assignment dealt the trajectories to k_score's workgroups: 0 in snake
   order, every workgroup equally heavy (shards that run as one round of resident workgroups, ticks without an
   assignment, DDDMR_DEAL=0 at create), 1 sorted, workgroup b holds the b-th heaviest trajectories (shards of several
   rounds, DDDMR_DEAL=1 wherever there is an assignment), 2 the light-tail variant (DDDMR_DEAL=2 only), -1 before any
   tick.  Every deal gives the same bits; tests use this to know which one they compared. */
int dddmr_rollout_deal(dddmr_rollout_ctx* ctx);

/* The assignment of the last tick and the loads it filed, [n_local] each (either pointer may be NULL; call with both
   NULL for the count): assign_out[slot] = local trajectory, slot = member * workgroups + workgroup; load_out[i] = the
   load word trajectory i filed for the NEXT tick's deal.  *assigned (may be NULL) = 1 if the tick dealt by load
   feedback, 0 if it took the trajectories strided (assign_out is then the identity). */
int dddmr_rollout_get_deal(dddmr_rollout_ctx* ctx, uint32_t* assign_out, uint32_t* load_out, size_t capacity,
                           size_t* n_local, int32_t* assigned);

/* Debug pose arrays of the last tick, poses_out[n][7] x y z qx qy qz qw, trajectory by
   trajectory in sample order, poses in step order: which = 0 the `trajectory` topic
   (every generated trajectory, local_planner.cpp:549-569), which = 1 the
   `accepted_trajectory` topic (cost_ >= 0, local_planner.cpp:461-470).  Call with
   poses_out == NULL to get the count.  Computed on demand from the rollout state the
   tick left on the device; nothing is copied unless this is called. */
int dddmr_rollout_get_pose_arrays(dddmr_rollout_ctx* ctx, int32_t which, double* poses_out,
                                  size_t capacity, size_t* n_poses);

/* Best trajectory poses of the last tick for visualisation
   (local_planner.cpp:472-478): poses_out[n][7] x y z qx qy qz qw. */
int dddmr_rollout_get_best_poses(dddmr_rollout_ctx* ctx, double* poses_out,
                                 size_t capacity, size_t* n_poses);

/* Cuboids of the best trajectory, vertices_out[n][8][3] floats in the vertex order of the theory's
   cuboid: base_trajectory::Trajectory::getCuboid(i) of every pose (trajectory.cpp:52-54, filled at
   dd_simple...cpp:443).  The reference collects them for a `trajectory_cuboids` debug cloud whose
   publication is commented out (local_planner.cpp:118,454,572-573,631); its `robot_cuboid` topic is a
   static marker built from the YAML vertices (:159-190,364-367) and needs no compute. */
int dddmr_rollout_get_best_cuboids(dddmr_rollout_ctx* ctx, float* vertices_out, size_t capacity_poses,
                                   size_t* n_poses);

/* Argmin key: min over keys == minimum cost, ties -> highest index (the
   reference's `<=` scan keeps the LAST minimal trajectory,
   local_planner.cpp:460-463).  cost < 0 (rejected) or cost > 9999999 (the scan's
   initial minimum_cost, :452: never accepted) -> INT64_MAX. */
int64_t dddmr_rollout_pack_key(double cost, uint32_t global_index);
int32_t dddmr_rollout_key_index(int64_t key); /* -1 for the "none" key */

/* ---------------------------------------------------------------------------------------------
   Global-mode marking / clearing layer: MultiLayerSpinningLidar::selfClear /
   selfMark with is_local_planner = false
   (dddmr_perception_3d/plugins/multilayer_spinning_lidar.cpp:306-628, isinLidarObservation :682-746,
   getCastingPointCloud :630-651) and the cluster store Marking::addPCPtr / removePCPtr /
   computeMinDistanceFromObstacle2GroundNodes (plugins/cluster_marking.cpp:49-138) with its
   DynamicGraph (src/graph/dynamic_graph.cpp).  The persistent voxel -> cluster store, the dGraph
   (per-ground-node obstacle distance) and the lethal set live on the device.

   One dddmr_rollout_marking_update() = one StackedPerception::doClear_then_Mark() pass of the lidar
   plugin (src/stacked_perception.cpp:72-90): selfClear against the PREVIOUS update's observation
   and the current sensor pose, then selfMark of the current observation.  The observation is the
   context's current aggregate cloud in the global frame -- what dddmr_rollout_set_scan leaves on
   the device (pcl_msg_gbl_, :322-323) or dddmr_rollout_set_cloud uploaded.
   Parameters carry the plugin's YAML names (multilayer_spinning_lidar.cpp:73-139) and the node's
   inscribed_radius / inflation_radius / max_obstacle_distance. */
typedef struct {
  double xy_resolution, height_resolution;
  double marking_height, perception_window_size;
  double vertical_FOV_top, vertical_FOV_bottom;                 /* degrees */
  double scan_effective_positive_start, scan_effective_positive_end;
  double scan_effective_negative_start, scan_effective_negative_end;
  double euclidean_cluster_extraction_tolerance;
  int32_t euclidean_cluster_extraction_min_cluster_size;
  int32_t reserved;
  double segmentation_ignore_ratio;
  double inscribed_radius, inflation_radius, max_obstacle_distance;
  uint32_t max_markings;        /* slots of the persistent store; size it for about twice the markings alive at a time:
                                   cleared voxels keep their slot until the store's garbage collection drops them
                                   (it runs when half the slots hold a key) */
  uint32_t max_cluster_points;  /* capacity of the pool of stored cluster points (0.2 m downsampled) */
} dddmr_marking_config;

typedef struct {
  uint32_t n_observation;   /* points of the observation this update marked */
  uint32_t n_clusters;      /* Euclidean clusters found in it */
  uint32_t n_marked;        /* clusters stored by Marking::addPCPtr */
  uint32_t n_in_window;     /* stored markings selfClear looked at */
  uint32_t n_cleared;       /* ... of which removePCPtr'ed */
  uint32_t n_alive;         /* markings alive after the update */
  float clear_ms, mark_ms;  /* HIP-event times of the two halves */
} dddmr_marking_stats;

/* ground = shared_data_->pcl_ground_ (the nodes of the dGraph, kdtree_ground_), map =
   shared_data_->pcl_map_ (kdtree_map_, the static layer's cloud); both x y z records `stride`
   bytes apart, copied to the device once.  Also initialises the dGraph (resetdGraph, :831-839). */
int dddmr_rollout_marking_create(dddmr_rollout_ctx* ctx, const dddmr_marking_config* cfg,
                                 const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                                 const float* map_xyz, size_t n_map, size_t map_stride_bytes);
/* One doClear_then_Mark pass.  May be called between dddmr_rollout_tick_begin and _tick_end: the
   reference runs the perception thread's pass and the planner's tick side by side, and so does the
   device (the update takes a stream of its own next to the tick's kernels) -- provided no newer
   observation was published after tick_begin, else DDDMR_ERR_STATE (call it after tick_end). */
int dddmr_rollout_marking_update(dddmr_rollout_ctx* ctx, const double T_base_sensor[7],
                                 const double T_gbl_base[7], dddmr_marking_stats* stats);
/* resetdGraph: empty store, dGraph back to max_obstacle_distance. */
int dddmr_rollout_marking_reset(dddmr_rollout_ctx* ctx);
/* The generator points of every alive marking -- its cluster projected on the robot's ground plane and
   downsampled at 0.1 m, what computeMinDistanceFromObstacle2GroundNodes (cluster_marking.cpp:54-64)
   searches the ground nodes with -- as x y z floats, with the voxel key (x y z ints) of the marking each
   belongs to in voxel_out (may be NULL); call with xyz_out NULL for the count.  Debug / visualisation
   (the reference publishes its markings as a cloud). */
int dddmr_rollout_marking_get_points(dddmr_rollout_ctx* ctx, float* xyz_out, int32_t* voxel_out, size_t capacity,
                                     size_t* n);
/* Alive markings as voxel keys (x y z ints, xyz_out[n][3]); call with NULL for the count. */
int dddmr_rollout_marking_get_voxels(dddmr_rollout_ctx* ctx, int32_t* xyz_out, size_t capacity, size_t* n);
/* dGraph values of ground nodes 0..n_ground (DynamicGraph::initial fills n + 1 entries) and the
   lethal set (lethal_map_ keys) as one byte per ground node. */
int dddmr_rollout_marking_get_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity);
int dddmr_rollout_marking_get_lethal(dddmr_rollout_ctx* ctx, uint8_t* flags_out, size_t capacity);
/* Which route the updates took (observations of up to 32768 points run fused: five launches, no
   copies; larger ones take the general route with library sorts; DDDMR_MARKING_ROUTE=general|fused
   forces one) and how many kernels / memsets the last update launched.  Diagnostics, any pointer
   may be NULL. */
int dddmr_rollout_marking_route_counts(dddmr_rollout_ctx* ctx, uint32_t* updates_fused,
                                       uint32_t* updates_general, uint32_t* launches_last_update);

/* Perception stack on the device: both layers in one pass, the stacked minimum dGraph, the lethal masks and the list of
   ground nodes that changed (additions to ABI version 2; no existing struct or entry changes, and the layers' own
   entries answer exactly as before in a context that has a stack).  The counterpart of StackedPerception
   (src/dddmr_perception_3d/src/stacked_perception.cpp:72-126,142-155) around "a velodyne plus realsense".

   Layers are named by id: DDDMR_STACK_LIDAR (the dddmr_rollout_marking_* layer), DDDMR_STACK_DEPTH (the
   dddmr_rollout_depth_layer_* layer) and DDDMR_STACK_HOST0 + slot for up to DDDMR_STACK_MAX_HOST layers whose dGraph
   the host computes (the static layer, static_layer.cpp:233-285,430-435, whose edge detection runs PCL's RANSAC; the zone
   layers, no_entry_layer.cpp:225-304).  layer_order[0 .. n_order) is the plugin order: every layer of the stack exactly
   once.  The minimum is taken in that order, bit i of a lethal mask is the layer at position i (always 0 for a host
   layer, which has no lethal set), and dddmr_rollout_stack_get_lethal_nodes lists the device layers in that order.

   dddmr_rollout_stack_create: a device layer that is asked for must exist already (DDDMR_ERR_STATE) with cfg.n_ground
   ground nodes (DDDMR_ERR_BAD_ARG): the caller passes the SAME pcl_ground_ to marking_create and depth_layer_create, as
   the reference's plugins share shared_data_->pcl_ground_; the stack indexes both dGraphs by the same node number and
   cannot check more than the count.  A stack of host layers only is allowed.  DDDMR_ERR_BAD_ARG: more than
   DDDMR_STACK_MAX_HOST host layers, a layer_order that is not a permutation of the stack's layers, n_ground >= 2^30;
   DDDMR_ERR_CAPACITY: max_changes above 2^28; DDDMR_ERR_STATE: a dddmr_rollout_tick_begin is pending.  A refused call
   leaves an earlier stack in place; a successful one replaces it, with the stacked arrays recomputed from the layers as
   they are and an empty change list (host slots start unset).  A later marking_create or depth_layer_create drops the
   stack: every stack call then answers DDDMR_ERR_STATE until the next stack_create.

   dddmr_rollout_stack_set_host_layer uploads values[0 .. n_ground] once; they stay until the slot is replaced (NULL
   unsets it).  An unset slot does not take part.  The stacked arrays change with the next stack_update, whose change
   list shows it.

   dddmr_rollout_stack_update is one doClear_then_Mark pass (stacked_perception.cpp:82-88) over the device layers, each on
   its own sensor's observation:
     lidar layer: exactly the pass dddmr_rollout_marking_update runs (both routes, tie fixing, housekeeping), but on the
       LIDAR SOURCES' observation only: the segments of the published aggregate that came from sources fed with
       set_scan / set_scan_source, in source order (the aggregate is pinned like a tick pins it and carries the
       per-source counts recorded when it was published, so a concurrent feed cannot tear it).  A context with several
       lidar sources gives their concatenation to ONE store; the reference would hold one store per plugin (a limit).
       DDDMR_ERR_STATE when the published aggregate did not come from the sources (a set_cloud since the last feed).
     depth layer: exactly the pass dddmr_rollout_depth_layer_update runs (it reads the depth sources only).  Where the
       reference's plugin returns early -- no depth source, or a camera without a frustum yet
       (depth_camera_layer.cpp:266-269, :482-485) -- the layer is skipped for this pass: stats.depth_skipped = 1,
       depth_rc = DDDMR_OK, its state untouched, and the other layer runs.
     stacked arrays: k_stack_min recomputes them and the change list whatever the layers returned, so they always
       equal the layers' current arrays: v = 99999.9; for each layer in order: v = (x < v) ? x : v -- std::min(tmp, x)
       of stacked_perception.cpp:114-126, so a NaN in a host layer leaves v alone and nothing comes out above 99999.9.
   Returns the first failing layer's code (lidar first), DDDMR_OK otherwise; stats (required) is filled either way.
   T_base_sensor is the lidar's; both transforms may be NULL in a stack without device layers.  DDDMR_ERR_STATE while a
   dddmr_rollout_tick_begin is pending (the layers' own entries may run beside a tick; the stack does not yet).
   host_waits: the lidar pass counts as its one regular wait, the depth pass reports its own, the stack adds one.

   dddmr_rollout_stack_get_changes: the nodes whose stacked value (as a bit pattern) or lethal mask differs from before
   the last update, each exactly once, in no particular order, with the new value and mask.  Any output may be NULL;
   all NULL: count only.  More changes than max_changes or than capacity: DDDMR_ERR_CAPACITY with *n the true count and
   nothing written; dddmr_rollout_stack_get_min_dgraph / _get_lethal_mask (n_ground + 1 entries each, the last node
   unused by the layers) are then the way to resynchronise.  No device work: the list is in host memory when
   stack_update returns.

   dddmr_rollout_stack_get_lethal_nodes is aggregateLethal (:142-155): for each device layer in layer_order, that layer's
   lethal ground nodes (< n_ground) in ascending order, one list after the other; a node lethal in two layers appears
   twice, as in the reference's concatenated cloud.  node_out NULL: count only.

   dddmr_rollout_stack_reset is StackedPerception::resetdGraph (:92-102): both layers are reset, the stacked arrays
   recomputed, the change list emptied; host slots keep their values. */
#define DDDMR_STACK_LIDAR 0
#define DDDMR_STACK_DEPTH 1
#define DDDMR_STACK_HOST0 2
#define DDDMR_STACK_MAX_HOST 4
#define DDDMR_STACK_MAX_LAYERS 6
typedef struct {
  uint32_t n_ground;
  int32_t use_lidar_layer, use_depth_layer;
  int32_t n_host_layers;                              /* 0 .. DDDMR_STACK_MAX_HOST: slots 0 .. n_host_layers - 1 */
  int32_t n_order;                                    /* = the number of layers of the stack */
  int32_t layer_order[DDDMR_STACK_MAX_LAYERS];
  uint32_t max_changes;                               /* capacity of the change list */
} dddmr_stack_config;

typedef struct {
  dddmr_marking_stats lidar;
  dddmr_depth_layer_stats depth;
  int32_t lidar_rc, depth_rc;
  uint32_t depth_skipped;
  uint32_t n_changed;                                 /* the true count, also beyond max_changes */
  uint32_t launches;                                  /* device operations of the pass: the layers' own counts plus the stack's */
  uint32_t host_waits;
} dddmr_stack_stats;

int dddmr_rollout_stack_create(dddmr_rollout_ctx* ctx, const dddmr_stack_config* cfg);
int dddmr_rollout_stack_set_host_layer(dddmr_rollout_ctx* ctx, int32_t slot, const double* values /* [n_ground + 1] or NULL */);
int dddmr_rollout_stack_update(dddmr_rollout_ctx* ctx, const double T_base_sensor[7], const double T_gbl_base[7],
                               dddmr_stack_stats* stats);
int dddmr_rollout_stack_get_changes(dddmr_rollout_ctx* ctx, uint32_t* node_out, double* value_out, uint8_t* lethal_mask_out,
                                    size_t capacity, size_t* n);
int dddmr_rollout_stack_get_min_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity);
int dddmr_rollout_stack_get_lethal_mask(dddmr_rollout_ctx* ctx, uint8_t* mask_out, size_t capacity);
int dddmr_rollout_stack_get_lethal_nodes(dddmr_rollout_ctx* ctx, uint32_t* node_out, size_t capacity, size_t* n);
int dddmr_rollout_stack_reset(dddmr_rollout_ctx* ctx);

/* ---- Particle filter lidar likelihood: mcl_3dl's LidarMeasurementModelLikelihood::measure for a batch of particles ----
   (dddmr_mcl_3dl/src/lidar_measurement_model_likelihood.cpp:86-252, called once per particle by pf_->measure,
   src/mcl_3dl.cpp:466-503).  The localiser's one batch kernel; the preparation of the observation
   (cbLeGoFeatureCloud) is the block after this one, motion prediction, weight normalisation, bias and resampling on a
   particle set that stays in device memory are dddmr_rollout_mcl_filter_*, sub-map loading is dddmr_rollout_submap_*.

   dddmr_rollout_mcl_create takes the model's parameters (likelihood.match_dist_min / match_dist_flat /
   radius_of_ground_search / threshold_for_trusted_ground) and the capacities.  DDDMR_ERR_BAD_ARG: a distance that is
   not finite, match_dist_min or the ground radius not positive, match_dist_flat negative, a NEGATIVE threshold (the
   reference compares it as an unsigned number there), a capacity of 0.  DDDMR_ERR_CAPACITY: more than 2^24 map or
   ground points, 2^20 particles, 2000 observation points (flat + less sharp) or 1024 ground neighbours.  A second
   create replaces the state (and forgets the map).  The state is freed with the context.

   dddmr_rollout_mcl_set_map is SubMaps::swapKdTree: the sub-map cloud, the ground cloud and one normal per ground
   point (xyz records, strides in bytes).  The new grids are built beside the current ones and swapped in only on
   success: a refused call (DDDMR_ERR_CAPACITY above max_map_points / max_ground_points, DDDMR_ERR_BAD_ARG for a
   non-finite coordinate, one beyond 1e6 m, or a cloud wider than 4096 m on an axis: the search boxes' 1 mm widening
   covers float rounding up to there) changes nothing, and the next measure answers from the old map.  Either
   cloud may be empty.

   dddmr_rollout_mcl_measure: flat_xyz [n_flat][3], less_sharp_xyzi [n_less_sharp][4] (the intensity is the weight the
   reference divides by), states [n_states][7] = pos xyz, rot xyzw, raw and not normalised.  likelihood_out[i] =
   score_like * pos_weight and quality_out[i] = the match ratio of particle i; stats (may be NULL) carries the minimum
   and maximum quality as mcl_3dl.cpp:476-498 keeps them (they start at 1 and 0).  The arithmetic is the reference's,
   float where it is float and double where it is double; score_like and the normal averages are added in the
   reference's order, so score_like, the counts and the quality are bit-equal to it and pos_weight is within a float ulp
   (DESIGN.md 4e).  Deliberate differences: a call without any observation point is refused (DDDMR_ERR_BAD_ARG; the
   reference divides 0 by 0); a state with a non-finite component gets likelihood 0 and quality 0 and is counted in
   stats.n_bad_states; a non-finite observation point (before or after the transform) matches nothing and still counts
   in the denominator.  DDDMR_ERR_CAPACITY: more states or points than created for, or a particle with more than
   max_ground_neighbours ground points inside the radius (nothing is written then but stats).  DDDMR_ERR_STATE: no map
   yet, or a dddmr_rollout_tick_begin is pending (set_map too: the conservative rule of dddmr_rollout_stack_update).

   dddmr_rollout_mcl_get_terms: the parts of the last successful measure, per particle, for tests and debugging; any
   output may be NULL.  healthy_out: 1 where the ground was trusted.  DDDMR_ERR_CAPACITY when capacity is below the
   last call's particle count. */
typedef struct {
  double match_dist_min, match_dist_flat;
  double radius_of_ground_search;
  int32_t threshold_for_trusted_ground;
  uint32_t max_map_points, max_ground_points;
  uint32_t max_particles;
  uint32_t max_observation_points;                    /* flat + less sharp */
  uint32_t max_ground_neighbours;
  uint32_t reserved;
} dddmr_mcl_config;

typedef struct {
  float quality_min, quality_max;
  uint32_t n_bad_states;
  uint32_t n_over_capacity;                           /* particles beyond max_ground_neighbours */
  uint32_t max_ground_neighbours_seen;
  uint32_t launches, host_waits;
  uint32_t reserved;
} dddmr_mcl_stats;

int dddmr_rollout_mcl_create(dddmr_rollout_ctx* ctx, const dddmr_mcl_config* cfg);
int dddmr_rollout_mcl_set_map(dddmr_rollout_ctx* ctx, const float* map_xyz, size_t n_map, size_t map_stride_bytes,
                              const float* ground_xyz, const float* ground_normals, size_t n_ground, size_t ground_stride_bytes,
                              size_t normal_stride_bytes);
int dddmr_rollout_mcl_measure(dddmr_rollout_ctx* ctx, const float* flat_xyz, size_t n_flat, const float* less_sharp_xyzi,
                              size_t n_less_sharp, const float* states /* [n_states][7] */, size_t n_states, float* likelihood_out,
                              float* quality_out, dddmr_mcl_stats* stats);
int dddmr_rollout_mcl_get_terms(dddmr_rollout_ctx* ctx, float* score_like_out, float* pos_weight_out, uint32_t* n_match_out,
                                uint32_t* n_ground_out, uint8_t* healthy_out, size_t capacity);

/* ---- The localiser's observation: mcl_3dl's MCL3dlNode::cbLeGoFeatureCloud on the device (additions to ABI version 2;
   no existing struct or entry changes; a context that never configures the observation runs exactly the launches it
   ran before).  src/dddmr_mcl_3dl/src/mcl_3dl.cpp:263-464 turns a sweep's flat and less-sharp lists into the two clouds
   measure() takes; line numbers below are that file's.  T_b2s is trans_b2s_af3 (base_link <- sensor), row-major 3 x 4,
   computed by the caller.  Float where the reference is float, double where it is double, nothing fused:
     transform (:295-296)       pcl::transformPointCloud(Affine3d) on both lists: double multiply-add, float result.
     flat (:306-309)            VoxelGrid with leaf (1.0f, 1.0f, 0.1f): voxel = floor(p * inverse_leaf) - min_b with the
                                inverse per axis in float, output in voxel-index order (x fastest), centroid = float
                                running sum in input order / count.  Only x y z go on.
     normals (:320-329)         NormalEstimation, setKSearch(5), on the transformed less-sharp cloud itself: the 5 nearest
                                by FLANN's float L2_Simple, the point included, ties by (d2, index); all of them when
                                there are fewer than 5; fewer than 3 give a NaN normal; float mean and covariance about
                                the first neighbour; PCL's closed-form eigen33; flipped toward (0, 0, 0).  Restated from
                                memory of PCL 1.15: DESIGN.md 4e numbers the assumptions.
     dominance (:340-360)       two double sums of fabs(normal_y) and fabs(normal_x) in index order, each component
                                skipped on its own when NaN; x dominant when sx / sy >= 1.6, else y dominant when
                                sy / sx >= 1.6 (0 / 0 selects neither: an empty list takes the cluster branch).
     dominant branch (:362-403) every point in input order; intensity 1.0f when normal_x is NaN, else float(0.05 * sy /
                                sx) (x dominant; y dominant mirrored) when the float ratio normal_y / normal_x >= 0.5,
                                else 1.0f.
     cluster branch (:404-443)  EuclideanClusterExtraction(euc_cluster_distance, euc_cluster_min_size, N): strict float
                                d2 < float(tol * tol), clusters in order of their lowest index, indices ascending, a
                                cluster below the minimum is dropped WITH its points, the kept ones ordered by
                                libstdc++'s std::sort(rbegin, rend) on the size (replayed on the host: the prepare's one
                                wait); intensity float(double(size) / double(N)), halved when size < min_size + 1.
   The result is measure()'s two arrays: flat x y z and less sharp x y z intensity.  It is double-buffered and stays in
   device memory; a refused prepare leaves the previous one in place for the getter and the measure.

   dddmr_rollout_mcl_set_observation_config: the two parameters (mcl_3dl.yaml: euc_cluster_distance 0.8,
   euc_cluster_min_size 3) and the input capacities; NULL switches the observation off.  A new configuration forgets the
   prepared observation, and so does a second dddmr_rollout_mcl_create.  Deliberate differences from the reference:
   a NEGATIVE euc_cluster_min_size and a non-positive or non-finite euc_cluster_distance are refused
   (DDDMR_ERR_BAD_ARG), and dddmr_rollout_mcl_prepare refuses a non-finite input coordinate (DDDMR_ERR_BAD_ARG; the
   reference's answer there is whatever PCL does with is_dense).  DDDMR_ERR_CAPACITY: max_flat_points +
   max_less_sharp_points above mcl_create's max_observation_points (the outputs are never more than the inputs).
   dddmr_rollout_mcl_prepare: xyz records, strides in bytes.  dddmr_rollout_mcl_prepare_from_sweep: the accepted
   sweep's flat (which 2) and less-sharp (which 1) features of a sweep source, x y z only, read in device memory.
   DDDMR_ERR_STATE: no mcl_create, no configuration, a dddmr_rollout_tick_begin pending, or (from_sweep) not a sweep
   source or its features off.  DDDMR_ERR_CAPACITY: more input points than configured.  DDDMR_ERR_BAD_ARG: a
   non-finite T_b2s entry, a bad stride, unknown flags.  stats (may be NULL): the counts, the branch, the two sums;
   n_clusters counts the kept clusters, n_small_clusters those of them with size < min_size + 1, n_nan_normals the
   points whose normal_x is NaN; launches (1, or 2 in the cluster branch) and host_waits (1).

   dddmr_rollout_mcl_get_observation follows dddmr_rollout_get_lidar_sweep_features: NULL outputs only report the counts,
   DDDMR_ERR_CAPACITY when an output is wanted and its capacity is below the count; normals_out is [n_less_sharp_in][3]
   in INPUT order.  Before the first prepare: zero points.
   dddmr_rollout_mcl_measure_prepared is dddmr_rollout_mcl_measure on the prepared observation where it lies: the same
   three kernels, the same answers, dddmr_rollout_mcl_get_terms answers for it too.  Like mcl_measure it refuses an
   observation without any point (DDDMR_ERR_BAD_ARG). */
typedef struct {
  double euc_cluster_distance;                        /* mcl_3dl.yaml: 0.8 */
  int32_t euc_cluster_min_size;                       /* 3 */
  uint32_t max_flat_points, max_less_sharp_points;    /* inputs; sum <= mcl max_observation_points */
  uint32_t flags, reserved;                           /* 0 */
} dddmr_mcl_observation_config;

typedef struct {
  uint32_t n_flat_in, n_flat_out, n_less_sharp_in, n_less_sharp_out;
  uint32_t branch;                                    /* 0 clusters, 1 x dominant, 2 y dominant */
  uint32_t n_clusters, n_small_clusters, n_nan_normals;
  double sum_normal_x, sum_normal_y;
  uint32_t launches, host_waits;
} dddmr_mcl_observation_stats;

int dddmr_rollout_mcl_set_observation_config(dddmr_rollout_ctx* ctx, const dddmr_mcl_observation_config* cfg);
int dddmr_rollout_mcl_prepare(dddmr_rollout_ctx* ctx, const float* flat_xyz, size_t n_flat, size_t flat_stride_bytes,
                              const float* less_sharp_xyz, size_t n_less_sharp, size_t less_sharp_stride_bytes,
                              const double T_b2s[12], dddmr_mcl_observation_stats* stats);
int dddmr_rollout_mcl_prepare_from_sweep(dddmr_rollout_ctx* ctx, int32_t source_id, const double T_b2s[12],
                                         dddmr_mcl_observation_stats* stats);
int dddmr_rollout_mcl_get_observation(dddmr_rollout_ctx* ctx, float* flat_xyz_out, size_t flat_capacity, size_t* n_flat,
                                      float* less_sharp_xyzi_out, size_t less_sharp_capacity, size_t* n_less_sharp,
                                      float* normals_out /* [n_less_sharp_in][3], input order */, size_t normals_capacity);
int dddmr_rollout_mcl_measure_prepared(dddmr_rollout_ctx* ctx, const float* states /* [n_states][7] */, size_t n_states,
                                       float* likelihood_out, float* quality_out, dddmr_mcl_stats* stats);

/* ---- The localiser's particle set: mcl_3dl's filter step on the device, noise drawn by the caller (additions to ABI
   version 2; no existing struct or entry changes).  The particles (pose, odom_err_integ_lin_ / _ang_, noise_ll_ / la_ /
   al_ / aa_, probability_, probability_bias_) stay in device memory between the calls; what goes up per step is the
   caller's random numbers, what comes down is one dddmr_mcl_filter_estimate.  Line numbers are
   src/dddmr_mcl_3dl/include/mcl_3dl/pf.h's unless another file is named.  Float where the reference is float, double
   where it is double, no fused multiply-add; every sum whose order the result shows is taken in index order by one
   lane.  States are 13 floats in State6DOF::operator[] order (pos xyz, rot xyzw, integ_lin xyz, integ_ang xyz), noise4
   rows are noise_ll_, noise_la_, noise_al_, noise_aa_.

   dddmr_rollout_mcl_filter_create needs a dddmr_rollout_mcl_create first (DDDMR_ERR_STATE) with at least
   max_particles (DDDMR_ERR_CAPACITY); a second mcl_create drops the filter.  DDDMR_ERR_BAD_ARG: a time constant or
   variance that is not finite and positive (also once rounded to float, as the reference stores them), 0 particles.

   _filter_set_particles: probability NULL = float(1.0 / n) as init (:164-176) computes it, noise4 NULL = zeros.
   Deliberate difference: a negative or non-finite probability and a non-finite state or noise component are
   DDDMR_ERR_BAD_ARG (resample's map rests on a non-decreasing accum_probability_).  _filter_get_particles is a two-call
   getter: all outputs NULL reports *n; any output may be NULL; a capacity below the count is DDDMR_ERR_CAPACITY.

   _filter_predict: setOdoms (motion_prediction_model_differential_drive.h:46-54) on the host, predict (:56-67) one lane
   per particle; the device's transcendentals are sinf / cosf of yaw_diff / 2 (quat.h:216-225).  time_diff is rounded to
   float.  DDDMR_ERR_BAD_ARG: a non-finite odometry component or time_diff.

   _filter_set_noise: update_noise_func (src/mcl_3dl.cpp:221-229), the values already multiplied by odom_err_*.

   _filter_measure is MCL3dlNode::measure up to the covariance (src/mcl_3dl.cpp:466-601).  likelihood NULL: the three
   measure kernels run on the resident poses and the prepared observation (quality must be NULL too; the errors of
   dddmr_rollout_mcl_measure_prepared apply, stats is filled as there).  Otherwise likelihood [n] is taken as given
   (deliberate difference: a negative or non-finite one is DDDMR_ERR_BAD_ARG) and quality [n] or NULL feeds the
   minimum / maximum (1 and 0 without).  Then: pf::measure (:247-268; the products' float sum in index order; divided
   when sum > 0, else the old probabilities stay and `restored` is 1), the bias (src/mcl_3dl.cpp:518-530; 1.0f when
   state_prev [7] is NULL, the branch for more particles than num_particles_), expectationBiased with
   ParticleWeightedMeanQuat::add (state_6dof.h:303-315), max() (the first strict maximum), covariance(1.0, 1.0)
   (:293-348): expectation(1.0) with its break after the first running sum above 1.0f, p_num from the same sum, the
   elements of rows and columns 0 .. 5 as ((s[k] - e[k]) * (s[j] - e[j])) * p accumulated in float in index order and
   divided by the float p_sum.  random_sample_ratio < 1, resizeParticle and appendParticle are not built.
   mean_biased is raw as getMean returns it (the caller normalises its rotation as src/mcl_3dl.cpp:545 does).  The
   device evaluates acosf / expf for the bias: DESIGN.md 4e has the measured distance to the host's.

   _filter_reset_integ: integ_reset_func (src/mcl_3dl.cpp:570-575).

   _filter_resample is resampleUsingNoiseGenerator (:182-220).  u is the canonical draw in [0, 1) (DDDMR_ERR_BAD_ARG
   outside), rounded to float: initial_p = u * pstep in float, which is what libstdc++'s
   uniform_real_distribution<float>(0, pstep) computes from it.  accum is a float prefix in index order; particle i picks
   the first index with accum >= pstep * i + initial_p; past the end every later particle keeps the last valid pick; a
   particle whose pick equals the previous particle's (for particle 0: pick 0) is a duplicate, and the k-th duplicate in
   index order takes noise row k: state = pick's state + noise by State6DOF::operator+ (rot = noise.rot * rot, the
   integrals add, noise_* become 0 as the operator's default-constructed result has them), then normalize().  A noise
   row is pos xyz, rot xyzw, odom_err_integ_ang_ xyz of the state generateNoise builds (state_6dof.h:200-221; the linear
   integral's noise equals pos).  Every probability becomes float(1.0 / n).  Deliberate difference: among EQUAL accum
   values the lowest index is picked, where the reference's std::sort leaves an order of libstdc++'s making for more
   than 16 particles (n_ties counts the equal neighbours; 0 means the picks are the reference's).  DDDMR_ERR_CAPACITY
   with stats filled and nothing changed when rows < n_duplicates.

   _filter_add_noise: pf::noise (:226-232), the same addition for every particle without normalize().

   All entries run on the context's stream and answer DDDMR_ERR_STATE while a dddmr_rollout_tick_begin is pending, before
   filter_create, and (all but create and set_particles) before the first set_particles.  A refused call changes nothing. */
typedef struct {
  uint32_t max_particles;                             /* <= dddmr_mcl_config.max_particles */
  uint32_t reserved;
  double odom_err_integ_lin_tc, odom_err_integ_ang_tc; /* mcl_3dl.yaml: 5.0, 10.0 (doubles in Parameters, floats in the model) */
  double bias_var_dist, bias_var_ang;                 /* mcl_3dl.yaml: 2.0, 1.57 (doubles in Parameters, floats in NormalLikelihood) */
} dddmr_mcl_filter_config;

typedef struct {
  float mean_biased[7];        /* expectationBiased(): e_.pos_ / p_sum_, Quat(front_sum_, up_sum_) */
  float mean[7];               /* expectation(1.0), what covariance() subtracts */
  float max_state[13];
  uint32_t max_index;
  float cov[36];               /* rows and columns 0 .. 5 */
  float sums_biased[10];       /* p_sum_, e_.pos_, front_sum_, up_sum_ before getMean */
  float sums[10];
  float weight_sum;            /* pf::measure's sum */
  float bias_sum;              /* == sums_biased[0] */
  uint32_t p_num;
  uint32_t restored;
  float quality_min, quality_max;
  uint32_t launches, host_waits;
} dddmr_mcl_filter_estimate;

typedef struct {
  uint32_t n_duplicates, n_at_end, n_ties;
  uint32_t launches, host_waits;
  uint32_t reserved;
} dddmr_mcl_filter_resample_stats;

int dddmr_rollout_mcl_filter_create(dddmr_rollout_ctx* ctx, const dddmr_mcl_filter_config* cfg);
int dddmr_rollout_mcl_filter_set_particles(dddmr_rollout_ctx* ctx, const float* states /* [n][13] */, const float* probability /* [n] or NULL */,
                                           const float* noise4 /* [n][4] or NULL */, size_t n);
int dddmr_rollout_mcl_filter_get_particles(dddmr_rollout_ctx* ctx, float* states_out /* [n][13] */, float* probability_out, float* bias_out,
                                           float* noise4_out /* [n][4] */, size_t capacity, size_t* n);
int dddmr_rollout_mcl_filter_predict(dddmr_rollout_ctx* ctx, const float odom_prev[7], const float odom_cur[7], double time_diff);
int dddmr_rollout_mcl_filter_set_noise(dddmr_rollout_ctx* ctx, const float* noise4 /* [n][4] */, size_t n);
int dddmr_rollout_mcl_filter_measure(dddmr_rollout_ctx* ctx, const float* likelihood /* [n] or NULL */, const float* quality /* [n] or NULL */,
                                     size_t n, const float* state_prev /* [7] or NULL */, dddmr_mcl_filter_estimate* estimate,
                                     dddmr_mcl_stats* stats);
int dddmr_rollout_mcl_filter_reset_integ(dddmr_rollout_ctx* ctx);
int dddmr_rollout_mcl_filter_resample(dddmr_rollout_ctx* ctx, double u, const float* noise /* [rows][10] */, size_t rows,
                                      dddmr_mcl_filter_resample_stats* stats);
int dddmr_rollout_mcl_filter_add_noise(dddmr_rollout_ctx* ctx, const float* noise /* [n][10] */, size_t n);

/* ---- The localiser's sub-maps: mcl_3dl's SubMaps on the device (additions to ABI version 2; no existing struct or entry
   changes).  src/dddmr_mcl_3dl/src/sub_maps.cpp keeps the pose graph's keyframes, and every
   sub_map_warmup_trigger_distance (20 m) collects the keyframes within sub_map_search_radius (50 m) of the robot,
   concatenates their corner and ground clouds, builds two kd-trees and estimates one normal per ground point
   (pcl::NormalEstimation, setKSearch(20)), then swaps the result in.  Here the keyframes live in device memory once; a
   warm-up is a list of keyframe ids, and nothing but that list crosses the bus.  Line numbers are sub_maps.cpp's.

   dddmr_rollout_submap_create needs a dddmr_rollout_mcl_create first (DDDMR_ERR_STATE) and allocates the keyframe
   store, a warm-up generation beside mcl_set_map's two and the neighbour scratch.  normal_k is 3 .. 32 (the reference:
   20).  A later dddmr_rollout_mcl_create drops the store: every sub-map call then answers DDDMR_ERR_STATE until the
   next submap_create.  A second submap_create starts an empty store and forgets a warm-up; the current map stays.

   dddmr_rollout_submap_add_keyframe is one iteration of readPoseGraph's loop (:126-156) from pcl::transformPointCloud
   on: each output coordinate is the double expression t0 * x + t1 * y + t2 * z + t3 rounded to float once.
   T_map_base is 3 x 4 row-major, NULL = the clouds are in the map frame already; the quaternion from roll / pitch / yaw
   stays with the caller.  position is the keyframe's pose (what the reference puts into its pose kd-tree).  The store is
   append-only; ids are 0, 1, 2, ... in call order.  DDDMR_ERR_CAPACITY beyond max_keyframes or either point capacity;
   DDDMR_ERR_BAD_ARG for a non-finite transform, position or coordinate, or a bad stride.  A refused call stores nothing.

   dddmr_rollout_submap_select is the keyframe radius search (:225-235), host arithmetic: the position and the keyframe
   positions rounded to float, FLANN's L2_Simple in float (x y z order), kept where d2 <= float(radius * radius).  Ids
   come back ASCENDING (the reference asks FLANN for an unsorted result, whose order is the tree's traversal order;
   DESIGN.md 5).  ids_out NULL: count only; a capacity below the count is DDDMR_ERR_CAPACITY with *n the count.

   dddmr_rollout_submap_warm_up is the second half of warmUpThread (:283-298): the listed keyframes' corner clouds, then
   their ground clouds, gathered device to device in the order given; the two grids as mcl_set_map builds them; the
   normal_k nearest ground points of every ground point (the point included, ordered by (d2, index) with FLANN's float
   d2; all of them when there are fewer); NormalEstimation's normal over them as for the observation (mean and
   covariance about the first neighbour, PCL's closed-form eigen33, flipped toward (0, 0, 0), NaN below 3 neighbours).
   The result is the warm-up generation; the current one and every mcl_measure answer are untouched until the swap.
   DDDMR_ERR_BAD_ARG: an unknown or repeated id, or the extent mcl_set_map refuses (4096 m on an axis, 1e6 m from the
   origin); DDDMR_ERR_CAPACITY above mcl_create's max_map_points / max_ground_points; DDDMR_ERR_STATE while a
   dddmr_rollout_tick_begin is pending.  A refused call leaves an earlier warm-up in place.  stats (may be NULL):
   launches does not depend on the clouds' sizes (an empty cloud skips its own), host_waits is 1; max_rings_searched is
   the widest shell of grid cells a point's search reached, n_brute_force the points that finished by a pass over
   the whole cloud instead.

   dddmr_rollout_submap_swap is swapKdTree (:319-342): the warm-up generation becomes current, the warm-up slot empty.
   DDDMR_ERR_STATE without a ready warm-up.  The first sub-map of a run (:224-268) is a warm-up followed by a swap.
   dddmr_rollout_mcl_set_map keeps working and replaces the current generation only.

   dddmr_rollout_submap_get: what the reference publishes as sub_map / sub_ground, and what tests need.  which: 0 the
   current generation, 1 the warm-up (zero points when there is none).  Any output may be NULL; DDDMR_ERR_CAPACITY when
   one is wanted and its capacity is below the count.  neighbours_out is [n_ground][normal_k], -1 padded; it answers for
   a generation made by warm_up and gives -1 rows for one made by mcl_set_map. */
typedef struct {
  uint32_t max_keyframes;
  uint32_t max_store_map_points, max_store_ground_points;   /* all keyframes' corner / ground points together */
  uint32_t normal_k;                                  /* 3 .. 32; the reference: 20 */
  uint32_t reserved[2];
} dddmr_submap_config;

typedef struct {
  uint32_t n_keyframes, n_map, n_ground;
  uint32_t n_nan_normals;
  uint32_t max_rings_searched;
  uint32_t launches, host_waits;
  uint32_t n_brute_force;
} dddmr_submap_stats;

int dddmr_rollout_submap_create(dddmr_rollout_ctx* ctx, const dddmr_submap_config* cfg);
int dddmr_rollout_submap_add_keyframe(dddmr_rollout_ctx* ctx, const float* corner_xyz, size_t n_corner, size_t corner_stride_bytes,
                                      const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                                      const double T_map_base[12] /* 3x4 row-major, NULL = already in the map frame */,
                                      const double position[3], int32_t* id_out);
int dddmr_rollout_submap_select(dddmr_rollout_ctx* ctx, const double position[3], double radius, int32_t* ids_out, size_t capacity,
                                size_t* n);
int dddmr_rollout_submap_warm_up(dddmr_rollout_ctx* ctx, const int32_t* ids, size_t n_ids, dddmr_submap_stats* stats);
int dddmr_rollout_submap_swap(dddmr_rollout_ctx* ctx);
int dddmr_rollout_submap_get(dddmr_rollout_ctx* ctx, int32_t which /* 0 current, 1 warm-up */, float* map_xyz_out, size_t map_capacity,
                             size_t* n_map, float* ground_xyz_out, float* normals_out,
                             int32_t* neighbours_out /* [n_ground][normal_k], -1 padded */, size_t ground_capacity, size_t* n_ground);

/* ---- The static layer and the no-entry layer on the device: sGraph, dGraphs, stack slots (additions to ABI version 2;
   no existing struct or entry changes).  src/dddmr_perception_3d/plugins/static_layer.cpp regenerates its graphs in
   selfClear (:201-231) whenever the map and ground clouds are republished: one radius search per ground node for the
   edges of sGraph (generateStaticGraph, :233-285), the nearest map point of every node (:275-282) and the overhang test
   (radiusSearchConnection, :390-415) for its dGraph.  plugins/no_entry_layer.cpp inflates its enabled zones into a dGraph
   of its own (:265-283).  DESIGN.md 4d-3 restates the arithmetic; in short: radiusSearch(p, r) keeps
   l2_simple < float(double(r) * double(r)), strict, the query point included; an edge weight is sqrtf(d2), a dGraph value
   double(sqrtf(d2)); setValue is a minimum.

   dddmr_rollout_static_layer_create allocates two generations of the graph and the build's scratch.  DDDMR_ERR_BAD_ARG:
   adaptive_connection_number outside 1 .. 32 in adaptive mode, a radius that is negative, not finite or above 1000 m,
   max_ground_points 0; DDDMR_ERR_CAPACITY: more than 2^24 ground points, 2^26 map points or 2^30 edges.  A second create
   replaces the state (graphs and dGraphs are gone); a refused one leaves it.

   dddmr_rollout_static_layer_build is one selfClear regeneration (:201-231) from the two clouds (only x y z are read):
     neighbourhood of node i (:240-261): radiusSearch(node, radius_of_ground_connection), or in adaptive mode
       radiusSearch(node, double(0.5f) + 0.2 * k) for the first k in 1 .. 101 whose count reaches
       adaptive_connection_number, else k = 101;
     sGraph (:263-273, static_graph.cpp:46-48), when generate_static_graph: node i's edges are its neighbourhood with
       weights sqrtf(d2), the self edge of weight 0 included, as CSR rows in ascending neighbour index (the std::set's
       order); without generate_static_graph the graph has no edge (the reference does not call generateStaticGraph);
     dGraph: n_ground + 1 doubles, all max_obstacle_distance (resetdGraph, :422-427), then minima: when
       enable_edge_detection, 0.25 for a node whose neighbourhood holds at least 5 points and that has more than 10 map
       points inside radiusSearch(node, static_imposing_radius) with node.z + 0.1 <= z <= node.z + 1.0 and x, y within
       0.5 of the node's (pcl::PassThrough: float limits, both ends inclusive); when generate_static_graph,
       double(sqrtf(d2)) of the nearest map point when that is below inscribed_radius.
   The RANSAC plane, the ring probes and the node weights (:350-388, :417) stay with the caller.  The build goes into a
   second generation and replaces the served one only on success.  DDDMR_ERR_CAPACITY: more points than created for, or
   more edges than max_edges -- stats.n_edges is then the true count.  DDDMR_ERR_BAD_ARG: an empty ground, a coordinate
   that is not finite or beyond 1e6 m, a cloud wider than 4096 m on an axis.  DDDMR_ERR_STATE: no static_layer_create.
   A successful build drops the zones' dGraph (requestAllLayersToResetDGraph, :207): call set_zones again.  stats (may
   be NULL): host_waits is 2 (the edge count, then the result); n_long_rows counts the rows longer than
   DDDMR_STATIC_LAYER_ROW_LDS entries, which are ranked in global memory instead of LDS.

   dddmr_rollout_static_layer_get_graph: row_start_out takes n_ground + 1 entries, neighbour_out and weight_out n_edges
   each (edge_capacity entries are there).  Any output may be NULL; all NULL: the count only.  DDDMR_ERR_CAPACITY when
   an edge output is wanted and edge_capacity is below the count.  dddmr_rollout_static_layer_get_dgraph: n_ground + 1
   doubles (StaticLayer::get_dGraphValue, :429-434).

   dddmr_rollout_static_layer_set_zones rebuilds the no-entry dGraph (no_entry_layer.cpp:265-283) over the last build's
   ground from the concatenated points of the enabled zones: node i gets min(max_obstacle_distance, double(sqrtf(d2))) of
   its nearest zone point when d2 < float(inflation_distance^2), which equals the reference's loop over the zone points
   (l2_simple is symmetric, sqrtf monotone).  n_points = 0: every zone is off, every value max_obstacle_distance.
   Reading zones.yaml and the .pcd files, the markers and the layer's lethal cloud stay with the caller.
   DDDMR_ERR_STATE before the first build.  dddmr_rollout_static_layer_get_zone_dgraph: the same n_ground + 1 layout.

   dddmr_rollout_static_layer_bind copies one of the two dGraphs device to device into a host slot of the perception
   stack; the slot is then exactly as after dddmr_rollout_stack_set_host_layer with the same values: set, and shown by
   the next stack_update's change list.  DDDMR_ERR_STATE without a stack or without that dGraph; DDDMR_ERR_BAD_ARG for a
   slot out of range or a build whose n_ground differs from the stack's.

   All seven run on the context's stream and answer DDDMR_ERR_STATE while a dddmr_rollout_tick_begin is pending.  A
   refused or failed call leaves the previous build, dGraphs and slots as they were. */
#define DDDMR_STATIC_LAYER_ROW_LDS 512                /* entries of a row the fill pass ranks in LDS */
typedef struct {
  uint32_t max_ground_points, max_map_points, max_edges;
  int32_t use_adaptive_connection;                    /* static_layer.cpp:240 */
  uint32_t adaptive_connection_number;                /* 1 .. 32 in adaptive mode */
  int32_t enable_edge_detection;                      /* :215  the overhang part */
  int32_t generate_static_graph;                      /* :218  sGraph and the nearest-obstacle part */
  uint32_t reserved;
  double radius_of_ground_connection, static_imposing_radius;
  double inscribed_radius, max_obstacle_distance;     /* gbl_utils_->getInscribedRadius() / getMaxObstacleDistance() */
} dddmr_static_layer_config;

typedef struct {
  uint64_t n_edges;
  uint32_t n_ground, n_map;
  uint32_t max_degree, n_long_rows;
  uint32_t n_overhang, n_near_obstacle;               /* nodes set to 0.25 / to their nearest obstacle's distance */
  uint32_t n_zone_points, n_zone_nodes;               /* set_zones: points given, nodes inside an inflation ball */
  uint32_t launches, host_waits;
} dddmr_static_layer_stats;

int dddmr_rollout_static_layer_create(dddmr_rollout_ctx* ctx, const dddmr_static_layer_config* cfg);
int dddmr_rollout_static_layer_build(dddmr_rollout_ctx* ctx, const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                                     const float* map_xyz, size_t n_map, size_t map_stride_bytes, dddmr_static_layer_stats* stats);
int dddmr_rollout_static_layer_get_graph(dddmr_rollout_ctx* ctx, uint32_t* row_start_out /* [n_ground + 1] */, uint32_t* neighbour_out,
                                         float* weight_out, size_t edge_capacity, size_t* n_edges);
int dddmr_rollout_static_layer_get_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity);
int dddmr_rollout_static_layer_set_zones(dddmr_rollout_ctx* ctx, const float* zone_xyz, size_t n_points, size_t stride_bytes,
                                         double inflation_distance, dddmr_static_layer_stats* stats);
int dddmr_rollout_static_layer_get_zone_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity);
int dddmr_rollout_static_layer_bind(dddmr_rollout_ctx* ctx, int32_t which /* 0 static, 1 no-entry */, int32_t slot);

/* ---- The pre-graph global planner on the device graph (dddmr_rollout_global_plan_*; additions to version 2, no
   existing struct or entry changes).  src/dddmr_global_planner/src/a_star_on_pre_graph.cpp's A_Star_on_PreGraph::getPath
   (:191-289, use_pre_graph: true) reads two arrays that are already on the device: the static layer's sGraph
   (dddmr_rollout_static_layer_build) and get_min_dGraphValue, the stack's stacked minimum.  These entries search them
   where they are, so no graph and no dGraph crosses the bus for a plan.  DESIGN.md 4d-4 restates the arithmetic.

   dddmr_rollout_global_plan_create needs a static_layer_create (DDDMR_ERR_STATE otherwise) and sizes the node records
   of each of max_queries (1 .. DDDMR_GLOBAL_PLAN_MAX_QUERIES) query slots by that layer's max_ground_points.
   dgraph_source 0: the perception stack's stacked minimum (dddmr_rollout_stack_get_min_dgraph's array); 1: the static
   layer's own dGraph.  max_open_entries: the frontier entries a query may hold at once; max_expansions: the nodes a
   query may close.  DDDMR_ERR_BAD_ARG: a parameter that is not finite, a count of 0, a dgraph_source other than 0 / 1.

   dddmr_rollout_global_plan_set_node_weights uploads the ground cloud's `intensity` (getPath adds it at :246; the
   device keeps none otherwise): n = the last build's n_ground, or 0 for all zero, which is also the default.  A weight
   that is negative or not finite is DDDMR_ERR_BAD_ARG: a negative weight would let a node's self edge update the node
   while it is expanded, which the device version excludes (a deliberate difference).  A later static_layer_build with
   another n_ground drops the weights.

   dddmr_rollout_global_plan_nearest is getStartGoalID's search (global_planner.cpp:407, :451) for n points
   (xyz[n][3]): ids_out[i] = the nearest ground node of radiusSearch(p, 0.5), UINT32_MAX without one; equal distances
   resolve to the lowest index.  dddmr_rollout_global_plan_probe is determineDWAPlan's goal test
   (dynamic_window_aware_global_planner.cpp:248-270) for n points: the number of ground nodes in radiusSearch(p, 0.25)
   and whether any of them has a dGraph value below inscribed_radius.  Both use the ground grid of the last build
   (DDDMR_ERR_STATE when a build was refused since) and refuse a coordinate that is not finite.

   dddmr_rollout_global_plan_plan runs n_queries <= max_queries independent searches in one launch, one workgroup per
   query, with one host wait for the whole call.  Each query answers what getPath answers for it alone: results[i].status
   FOUND with path_len node ids from start to goal at path_out + path_offset (the paths follow one another), or NO_PATH
   (the frontier is exhausted, also where only entries of closed nodes remain: the reference reads begin() of an empty
   set there, a deliberate difference), BUDGET (max_expansions nodes closed) or OPEN_FULL (then the call returns
   DDDMR_ERR_CAPACITY), all three with an empty path.  n_expanded: nodes closed; n_pushed: entries the frontier set grew
   by (the start's included); n_discarded_closed: entries of closed nodes taken off the frontier; g_goal: the goal's g.
   start == goal gives the one-node path after one expansion.  DDDMR_ERR_STATE: no create, no build, a build without
   generate_static_graph, dgraph_source 0 without a stack, a pending tick_begin.  DDDMR_ERR_BAD_ARG: an id >= n_ground,
   a stack whose n_ground differs.  DDDMR_ERR_CAPACITY: more queries than max_queries, or paths beyond path_capacity
   (results are filled in either case).

   All five run on the context's stream and answer DDDMR_ERR_STATE while a dddmr_rollout_tick_begin is pending. */
#define DDDMR_GLOBAL_PLAN_MAX_QUERIES 16
#define DDDMR_GLOBAL_PLAN_FOUND 0
#define DDDMR_GLOBAL_PLAN_NO_PATH 1
#define DDDMR_GLOBAL_PLAN_BUDGET 2
#define DDDMR_GLOBAL_PLAN_OPEN_FULL 3
typedef struct {
  double turning_weight;                              /* a_star_on_pre_graph.cpp:246 */
  double a_star_expanding_radius;                     /* :222 */
  double inscribed_radius, inflation_descending_rate; /* :209-210 */
  int32_t dgraph_source;                              /* 0 the stack's minimum, 1 the static layer's dGraph */
  uint32_t max_queries, max_open_entries, max_expansions;
} dddmr_global_plan_config;

typedef struct {
  uint32_t status;                                    /* DDDMR_GLOBAL_PLAN_* */
  uint32_t path_offset, path_len;
  uint32_t n_expanded, n_pushed, n_discarded_closed;
  float g_goal;
  uint32_t host_waits;                                /* of the whole call */
} dddmr_global_plan_result;

int dddmr_rollout_global_plan_create(dddmr_rollout_ctx* ctx, const dddmr_global_plan_config* cfg);
int dddmr_rollout_global_plan_set_node_weights(dddmr_rollout_ctx* ctx, const float* weights, size_t n);
int dddmr_rollout_global_plan_nearest(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, uint32_t* ids_out);
int dddmr_rollout_global_plan_probe(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, uint32_t* n_ground_near_out, uint8_t* blocked_out);
int dddmr_rollout_global_plan_plan(dddmr_rollout_ctx* ctx, const uint32_t* start_id, const uint32_t* goal_id, size_t n_queries,
                                   uint32_t* path_out, size_t path_capacity, dddmr_global_plan_result* results);

/* ---- The global planner's default A* on the ground cloud (additions to version 2, no existing struct or entry
   changes).  global_planner.cpp:100 declares use_pre_graph false, so a robot running the reference as shipped plans with
   src/dddmr_global_planner/src/a_star_on_pc.cpp's A_Star_on_Graph::getPath (:200-329): the successors of a node are a
   radius search of the ground (the 8 nearest nodes where fewer than 8 are found), and an edge of 2 * inscribed_radius
   or more is marched by isLineOfSightClear (:168-198) against the aggregate lethal cloud.  These entries run that search
   on the planner state of dddmr_rollout_global_plan_create, with its config and budgets, on what is resident: the static
   layer's ground and grid, the stack's stacked minimum and lethal masks.  No sGraph is needed: a static layer built
   without generate_static_graph is enough.  DESIGN.md 4d-5 restates the arithmetic; the restatement the device is tested
   against is not pinned to compiled reference code yet.

   The aggregate lethal cloud (stacked_perception.cpp:142-155) is the plugins' lethal clouds appended.  With
   dgraph_source 0 the device layers' part is read where it is: a ground node counts once per device layer that holds it
   lethal (dddmr_rollout_stack_get_lethal_mask's bits).  dddmr_rollout_global_plan_set_lethal_points hands in the lethal
   points of the layers left on the host (the no-entry layer, a host-side plugin), n records of x y z stride_bytes apart:
   they replace the ones set before, n == 0 clears them, a duplicate is two points.  DDDMR_ERR_BAD_ARG: a coordinate that
   is not finite or beyond 1e6 m, a cloud wider than 4096 m; DDDMR_ERR_CAPACITY: more points than the static layer's
   max_ground_points.  With dgraph_source 1 these points are the whole cloud.  Without any lethal point every edge is
   clear, as in the reference, whose tree then has no cloud.

   dddmr_rollout_global_plan_set_graph_node_weights uploads sGraph_ptr_->getNodeWeight (static_graph.cpp:62, added at
   a_star_on_pc.cpp:287-288), a second per-node array beside set_node_weights' intensity, under the same rules: n = the
   last build's n_ground or 0 for all zero (the default), negative or non-finite weights refused, dropped by a build
   with another n_ground.  The intensity enters this search as avg_intensity (:248-252), the float sum over the
   successor list in list order divided by its size.  Both arrays of this section belong to the context: a
   global_plan_create keeps them unless the static layer's max_ground_points has changed since.

   dddmr_rollout_global_plan_plan_on_cloud is global_plan_plan's twin: n_queries <= max_queries searches in one launch,
   one workgroup per query, one host wait per call; results[i].plan is filled as global_plan_plan fills it.  The
   successor list is ascending in distance and, among equal distances, in index (nanoflann orders equals by its tree
   walk; the order shows only in which nodes make the 8 nearest and in avg_intensity's float sum).  Deliberate
   differences: a ground of fewer than 8 nodes is DDDMR_ERR_STATE (nearestKSearch leaves entries unfilled there);
   inscribed_radius <= 0 is DDDMR_ERR_BAD_ARG for this entry (the reference's march does not end), as is a negative
   a_star_expanding_radius or a radius above 1000 m; an edge whose march would take more than
   DDDMR_GLOBAL_PLAN_LOS_MAX_SAMPLES samples is blocked and counted in n_los_capped; a radius search that finds more than
   DDDMR_GLOBAL_PLAN_CLOUD_MAX_SUCCESSORS nodes ends its query with status ROW_FULL and the call with
   DDDMR_ERR_CAPACITY (results are filled); NO_PATH also where only entries of closed nodes remain, as global_plan_plan.
   The two searches share the planner's records and stamps and may be called in any order.  Other errors as
   global_plan_plan's, except that a build without generate_static_graph is accepted.

   All three answer DDDMR_ERR_STATE while a dddmr_rollout_tick_begin is pending. */
#define DDDMR_GLOBAL_PLAN_ROW_FULL 4
#define DDDMR_GLOBAL_PLAN_CLOUD_MAX_SUCCESSORS 1024
#define DDDMR_GLOBAL_PLAN_LOS_MAX_SAMPLES 4096
typedef struct {
  dddmr_global_plan_result plan;            /* as global_plan_plan fills it */
  uint32_t n_knn_fallbacks;                 /* expansions that took the 8 nearest */
  uint32_t n_lethal_skipped;                /* successors below inscribed_radius */
  uint32_t n_los_tested, n_los_blocked;     /* edges marched / refused by the march */
  uint32_t n_los_capped;                    /* of the blocked: by the sample cap */
  uint32_t max_successors;                  /* longest successor list met */
} dddmr_global_plan_cloud_result;

int dddmr_rollout_global_plan_set_graph_node_weights(dddmr_rollout_ctx* ctx, const float* weights, size_t n);
int dddmr_rollout_global_plan_set_lethal_points(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes);
int dddmr_rollout_global_plan_plan_on_cloud(dddmr_rollout_ctx* ctx, const uint32_t* start_id, const uint32_t* goal_id, size_t n_queries,
                                            uint32_t* path_out, size_t path_capacity, dddmr_global_plan_cloud_result* results);

/* Measurement aid ("a measured stream-copy ceiling on the same GPU"): streams
   `bytes` (>= 1 GiB recommended: beyond the 256 MB of MALL) `reps` times through a float4 copy
   kernel and a read-only kernel on the context's device; *copy_gbps counts read + write bytes.
   Not part of the reference's surface and not on the tick's path. */
int dddmr_rollout_stream_ceiling(dddmr_rollout_ctx* ctx, size_t bytes, int32_t reps,
                                 double* copy_gbps, double* read_gbps);

/* Self-test aid: sine and cosine of n heading angles from the rollout's own double-precision routine
   (the stand-in for the libm sin / cos the reference's theories call, dd_simple...cpp:416,457-464,
   omni_simple...cpp:498-505), so that a test can bound its error against a higher-precision value.
   Not part of the reference's surface and not on the tick's path. */
int dddmr_rollout_selftest_sincos(dddmr_rollout_ctx* ctx, const double* angles, size_t n,
                                  double* sin_out, double* cos_out);

/* Self-test aid: the library's wave and workgroup primitives (csrc/wave_ops.hip.h) over n <= 256 values and flags (a
   flag is set when its byte is not 0; n = 0 is allowed), one per lane of a single workgroup of 256 lanes; the lanes at
   or past n take part with value 0 and a clear flag.  With `lane` the thread's index modulo 64 and a wave 64 threads:
     out32[0][t]  inclusive prefix sum of the values over t's wave       out32[5][t]  minimum of the values of t's wave
     out32[1][t]  exclusive prefix sum over the workgroup                out32[6][t]  maximum
     out32[2][t]  how many lanes below t have their flag set             out32[7][t]  sum (wrapping)
     out32[3][t]  t's index from a wave-aggregated append, counter in    out32[8][t]  bits of the minimum of (float)value
                  global memory (of no meaning where the flag is clear)  out64[0][t]  minimum of (value << 32) | lane
     out32[4][t]  the same with the counter in LDS                       out64[1][t]  sum (wrapping) of the same
     out32[9][0 .. 3]  the workgroup's sum, its number of flags, the final global and LDS counters (both start at
                  append_base); the rest of row 9 is not written
   Rows are 256 entries.  Not part of the reference's surface and not on the tick's path. */
#define DDDMR_WAVE_OPS_OUT32 (10 * 256)
#define DDDMR_WAVE_OPS_OUT64 (2 * 256)
int dddmr_rollout_selftest_wave_ops(dddmr_rollout_ctx* ctx, const uint32_t* values, const uint8_t* flags, size_t n,
                                    uint32_t append_base, uint32_t* out32, unsigned long long* out64);

/* Self-test aid: what dddmr_rollout_selftest_wave_ops does not reach, in three launches.
     scan_out[0][t]  block_excl_scan<16> over one workgroup of 1024 lanes: the exclusive prefix sum of the n <= 1024 values
                     (lanes at or past n take part with 0; n = 0 is allowed); misc_out[0] is the total it reports
     scan_out[1][t]  wave_last of the inclusive prefix sum over t's wave: the wave's sum
     reduce_out[0 .. 3][l]  over ONE wave whose lane l holds lanes[l] (64 words, never null): the bits of wave_min and of
                     wave_max of the words read as float (feed no NaN), then wave_min and wave_max of the words read as int
     misc_out[1], [2]  last_block among n_groups workgroups of 256 lanes (1 .. DDDMR_WAVE_WIDE_MAX_GROUPS): lane 63 of each
                     wave stores the word n_groups * 0x9E3779B1 + i * i + 1 (wrapping) to slot i = 4 * workgroup + wave with a
                     device-scope atomic; the workgroup last_block names reads all 4 * n_groups slots with ld_agent.
                     [1] is how many workgroups were named, [2] the wrapping sum it read.  misc_out[3] stays 0.
   Rows of scan_out are 1024 entries, of reduce_out 64.  Not part of the reference's surface and not on the tick's path. */
#define DDDMR_WAVE_WIDE_SCAN (2 * 1024)
#define DDDMR_WAVE_WIDE_REDUCE (4 * 64)
#define DDDMR_WAVE_WIDE_MISC 4
#define DDDMR_WAVE_WIDE_MAX_GROUPS 4096
int dddmr_rollout_selftest_wave_wide(dddmr_rollout_ctx* ctx, const uint32_t* values, size_t n, const uint32_t* lanes,
                                     uint32_t n_groups, uint32_t* scan_out, uint32_t* reduce_out, uint32_t* misc_out);

/* Self-test aid: the uniform grid of csrc/point_grid.hip.h, built and walked as the modules do it.  The library's own
   grid_shape(lo, hi, cell[0] = cell_xy, cell[1] = cell_z, cap_cells), grid_alloc and grid_build run over the n packed
   xyz points (n = 0 is allowed; points outside the box are allowed and land in edge cells), then two kernels walk the
   grid for each of the m packed xyz queries with the box half width radius[0] = r_box and the squared radius
   radius[1] = r2.  Copied back, all as 32-bit words (floats as their bits):
     grid_out[8]             nx, ny, nz, then ox, oy, oz, inv_xy, inv_z
     cell_start_out          [nx * ny * nz + 1]; the caller provides cap_cells + 1 words
     sorted_out[n][4]        the cell-sorted records: x, y, z, original index
     thread_out[m][8]        from one thread per query: grid_radius_count with stop_at, grid_radius_count with 0x7fffffff,
                             grid_nearest, grid_nearest_id's id and d2, and from a grid_for_each whose functor never stops
                             the number of points visited, the wrapping sum and the xor of their original indices
     wave_out[m][5]          from one wave per query over grid_for_each_wave: the same visited count, index sum and index
                             xor, the number of points with d2 < r2, the minimum d2 (+inf without a point)
   Refused with DDDMR_ERR_BAD_ARG: counts over the limits below, a null pointer with a nonzero count, cap_cells of 0,
   stop_at below 1, a cell size outside 0.01 .. 1e6 m, r_box or r2 negative or not finite, lo > hi, and any coordinate
   that is not finite within 1e6 m.  Not part of the reference's surface and not on the tick's path. */
#define DDDMR_POINT_GRID_MAX_POINTS (1 << 16)
#define DDDMR_POINT_GRID_MAX_QUERIES (1 << 16)
#define DDDMR_POINT_GRID_MAX_CELLS (1 << 22)
int dddmr_rollout_selftest_point_grid(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, const float lo[3], const float hi[3],
                                      const float cell[2], uint32_t cap_cells, const float* queries, size_t m,
                                      const float radius[2], int32_t stop_at, uint32_t grid_out[8], uint32_t* cell_start_out,
                                      uint32_t* sorted_out, uint32_t* thread_out, uint32_t* wave_out);

const char* dddmr_rollout_last_error(dddmr_rollout_ctx* ctx);
const char* dddmr_rollout_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DDDMR_ROLLOUT_H_ */
