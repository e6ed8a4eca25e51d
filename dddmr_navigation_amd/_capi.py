"""ctypes view of include/dddmr_rollout.h (the C-ABI of the rollout engine).

The struct layouts here mirror the header field by field, and `SIGNATURES` is the one table of every function's
return and argument types; `load_library()` binds it and `EXPORTED_SYMBOLS` is derived from it.  What keeps the two
sides from drifting apart silently, all in `tests/test_capi_cpu.py`: sizeof() of every struct in `SIZEOF_STRUCTS`
against the compiled library (`dddmr_rollout_sizeof`; absolute sizes are pinned in the features' own test files);
every prototype of the header against `SIGNATURES` (name, parameter count, the kind of each parameter and of the return
type -- field order and pointee types are not checked); the library's exports against the header.  What the classes
on top hand to the library is pinned call by call in `tests/test_binding_trace_cpu.py`.

There is deliberately no CPU fallback: if the HIP library is missing or no HIP
device is usable, loading / `dddmr_rollout_create` fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

MAX_CRITICS = 8
NAME_LEN = 64
ABI_VERSION = 2

# dddmr_status
OK = 0
ERR_BAD_ARG = -1
ERR_NO_DEVICE = -2
ERR_HIP = -3
ERR_UNKNOWN_THEORY = -4
ERR_CAPACITY = -5
ERR_STATE = -6
OPINION_PASS = 0                 # perception_3d::PerceptionOpinion
OPINION_PATH_BLOCKED_WAIT = 1

# dddmr_planner_state (dddmr_sys_core/include/dddmr_sys_core/dddmr_enum_states.h:46-54)
TF_FAIL = 0
PRUNE_PLAN_FAIL = 1
ALL_TRAJECTORIES_FAIL = 2
PERCEPTION_MALFUNCTION = 3
TRAJECTORY_FOUND = 4
PATH_BLOCKED_WAIT = 5
PATH_BLOCKED_REPLANNING = 6

# dddmr_theory_kind
THEORY_DD_SIMPLE = 0
THEORY_OMNI_SIMPLE = 1
THEORY_DD_ROTATE_INPLACE = 2

# dddmr_critic_kind
CRITIC_COLLISION = 0
CRITIC_COLLISION_MIN_MAX = 1
CRITIC_STICK_PATH = 2
CRITIC_PURE_PURSUIT = 3
CRITIC_TOWARD_GLOBAL_PLAN = 4
CRITIC_SHORTEST_ANGLE = 5
CRITIC_TWIRLING = 6

COST_COLLISION = -1.0
COST_PURE_PURSUIT_GUARD = -4.0
COST_NN_FAIL = -12.0
COST_NOT_GENERATED = -100.0

KEY_NONE = (1 << 63) - 1
COMM_ID_BYTES = 128


class CriticConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("reserved", C.c_int32),
        ("weight", C.c_double),
        ("translation_weight", C.c_double),
        ("orientation_weight", C.c_double),
    ]


class TheoryConfig(C.Structure):
    _fields_ = [
        ("name", C.c_char * NAME_LEN),
        ("kind", C.c_int32),
        ("use_motor_constraint", C.c_int32),
        ("min_vel_x", C.c_double), ("max_vel_x", C.c_double),
        ("min_vel_y", C.c_double), ("max_vel_y", C.c_double),
        ("min_vel_trans", C.c_double), ("max_vel_trans", C.c_double),
        ("min_vel_theta", C.c_double), ("max_vel_theta", C.c_double),
        ("acc_lim_x", C.c_double), ("acc_lim_y", C.c_double), ("acc_lim_theta", C.c_double),
        ("deceleration_ratio", C.c_double),
        ("max_motor_shaft_rpm", C.c_double), ("wheel_diameter", C.c_double),
        ("gear_ratio", C.c_double), ("robot_radius", C.c_double),
        ("controller_frequency", C.c_double),
        ("sim_time", C.c_double),
        ("linear_x_sample", C.c_double), ("linear_y_sample", C.c_double),
        ("angular_z_sample", C.c_double),
        ("sim_granularity", C.c_double), ("angular_sim_granularity", C.c_double),
        ("rotation_speed", C.c_double),
        ("cuboid", (C.c_float * 3) * 8),
        ("bench_fixed_steps", C.c_int32),
        ("bench_no_zero_insert", C.c_int32),
        ("n_critics", C.c_int32),
        ("reserved", C.c_int32),
        ("critics", CriticConfig * MAX_CRITICS),
    ]


class RolloutConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("device", C.c_int32),
        ("rank", C.c_int32),
        ("world_size", C.c_int32),
        ("max_points", C.c_uint32),
        ("max_trajectories", C.c_uint32),
        ("max_steps", C.c_uint32),
        ("max_plan_poses", C.c_uint32),
        ("n_theories", C.c_int32),
        ("reserved", C.c_int32),
        ("theories", C.POINTER(TheoryConfig)),
    ]


class TickInput(C.Structure):
    _fields_ = [
        ("robot_pose", C.c_double * 7),
        ("robot_twist", C.c_double * 3),
        ("allowed_max_linear_speed", C.c_double),
        ("heading_deviation", C.c_double),
    ]


class RolloutResult(C.Structure):
    _fields_ = [
        ("planner_state", C.c_int32),
        ("best_index", C.c_int32),
        ("best_cost", C.c_double),
        ("vx", C.c_double), ("vy", C.c_double), ("wz", C.c_double),
        ("n_samples", C.c_uint32),
        ("n_local", C.c_uint32),
        ("local_begin", C.c_uint32),
        ("n_points_binned", C.c_uint32),
        ("key", C.c_int64),
        ("device_ms", C.c_float),
        ("score_ms", C.c_float),
    ]


class MarkingConfig(C.Structure):
    """dddmr_marking_config: the lidar plugin's global-mode parameters
    (dddmr_perception_3d/plugins/multilayer_spinning_lidar.cpp:73-139) + the node's radii."""
    _fields_ = [
        ("xy_resolution", C.c_double), ("height_resolution", C.c_double),
        ("marking_height", C.c_double), ("perception_window_size", C.c_double),
        ("vertical_FOV_top", C.c_double), ("vertical_FOV_bottom", C.c_double),
        ("scan_effective_positive_start", C.c_double), ("scan_effective_positive_end", C.c_double),
        ("scan_effective_negative_start", C.c_double), ("scan_effective_negative_end", C.c_double),
        ("euclidean_cluster_extraction_tolerance", C.c_double),
        ("euclidean_cluster_extraction_min_cluster_size", C.c_int32),
        ("reserved", C.c_int32),
        ("segmentation_ignore_ratio", C.c_double),
        ("inscribed_radius", C.c_double), ("inflation_radius", C.c_double), ("max_obstacle_distance", C.c_double),
        ("max_markings", C.c_uint32), ("max_cluster_points", C.c_uint32),
    ]


class MarkingStats(C.Structure):
    _fields_ = [
        ("n_observation", C.c_uint32), ("n_clusters", C.c_uint32), ("n_marked", C.c_uint32),
        ("n_in_window", C.c_uint32), ("n_cleared", C.c_uint32), ("n_alive", C.c_uint32),
        ("clear_ms", C.c_float), ("mark_ms", C.c_float),
    ]


class DepthSourceConfig(C.Structure):
    _fields_ = [
        ("min_obstacle_height", C.c_double), ("max_obstacle_height", C.c_double),
        ("observation_persistence_ns", C.c_int64),
        ("max_frame_points", C.c_uint32), ("max_frames", C.c_uint32),
    ]


DEPTH_IMAGE_DROP_ZERO = 1


class DepthImageConfig(C.Structure):
    """dddmr_depth_image_config: the image geometry, CameraInfo K and DepthImg2PointCloud's node parameters."""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("max_distance", C.c_double), ("leaf_size", C.c_double),
        ("sample_step", C.c_uint32), ("flags", C.c_uint32),
    ]


class LidarSweepConfig(C.Structure):
    """dddmr_lidar_sweep_config: ImageProjection's laser.* / imageProjection.* parameters and the mount pitch."""
    _fields_ = [
        ("num_vertical_scans", C.c_uint32), ("num_horizontal_scans", C.c_uint32),
        ("vertical_angle_bottom", C.c_double), ("vertical_angle_top", C.c_double),
        ("ground_scan_index", C.c_uint32),
        ("segment_theta", C.c_double),
        ("segment_valid_point_num", C.c_uint32), ("segment_valid_line_num", C.c_uint32),
        ("minimum_detection_range", C.c_double), ("maximum_detection_range", C.c_double),
        ("sensor_mount_angle", C.c_double),
        ("max_sweep_points", C.c_uint32), ("flags", C.c_uint32),
    ]


class LidarFeaturesConfig(C.Structure):
    """dddmr_lidar_features_config: featureAssociation.edge_threshold / surf_threshold and publishCloud's
    trans_c2s.inverse() as a row-major 3 x 4."""
    _fields_ = [
        ("edge_threshold", C.c_double), ("surf_threshold", C.c_double),
        ("T_out", C.c_double * 12),
        ("flags", C.c_uint32),
    ]


class DepthFrustumConfig(C.Structure):
    """dddmr_depth_frustum_config: the depth buffer's FOV_W / FOV_V (radians) and obstacle_min_range / obstacle_max_range."""
    _fields_ = [
        ("FOV_W", C.c_double), ("FOV_V", C.c_double),
        ("obstacle_min_range", C.c_double), ("obstacle_max_range", C.c_double),
    ]


class DepthMarkConfig(C.Structure):
    """dddmr_depth_mark_config: the depth camera layer's clustering parameters (depth_camera_layer.cpp:52-75)."""
    _fields_ = [
        ("xy_resolution", C.c_double), ("height_resolution", C.c_double),
        ("euclidean_cluster_extraction_tolerance", C.c_double),
        ("euclidean_cluster_extraction_min_cluster_size", C.c_int32),
        ("reserved", C.c_int32),
        ("segmentation_ignore_ratio", C.c_double),
        ("max_observation_points", C.c_uint32), ("reserved2", C.c_uint32),
    ]


class DepthMarkStats(C.Structure):
    _fields_ = [
        ("n_observation", C.c_uint32), ("n_clusters", C.c_uint32), ("n_ground_rejected", C.c_uint32),
        ("n_static_rejected", C.c_uint32), ("n_outside_frustums", C.c_uint32), ("n_accepted", C.c_uint32),
        ("n_points", C.c_uint32), ("launches", C.c_uint32),
    ]


class DepthLayerConfig(C.Structure):
    """dddmr_depth_layer_config: the global-mode depth camera layer (depth_camera_layer.cpp:52-75 and the Marking's radii)."""
    _fields_ = [
        ("xy_resolution", C.c_double), ("height_resolution", C.c_double),
        ("marking_height", C.c_double), ("perception_window_size", C.c_double),
        ("euclidean_cluster_extraction_tolerance", C.c_double),
        ("euclidean_cluster_extraction_min_cluster_size", C.c_int32),
        ("reserved", C.c_int32),
        ("segmentation_ignore_ratio", C.c_double),
        ("inscribed_radius", C.c_double), ("inflation_radius", C.c_double), ("max_obstacle_distance", C.c_double),
        ("max_observation_points", C.c_uint32), ("max_markings", C.c_uint32), ("max_cluster_points", C.c_uint32),
        ("reserved2", C.c_uint32),
    ]


class DepthLayerStats(C.Structure):
    _fields_ = [
        ("n_observation", C.c_uint32), ("n_in_window", C.c_uint32), ("n_cleared", C.c_uint32), ("n_clusters", C.c_uint32),
        ("n_accepted", C.c_uint32), ("n_contested", C.c_uint32), ("n_alive", C.c_uint32), ("gc_runs", C.c_uint32),
        ("launches", C.c_uint32), ("host_waits", C.c_uint32),
    ]


# dddmr_rollout_stack_*: layer ids of dddmr_stack_config.layer_order
STACK_LIDAR, STACK_DEPTH, STACK_HOST0, STACK_MAX_HOST, STACK_MAX_LAYERS = 0, 1, 2, 4, 6
STACK_START = 99999.9          # get_min_dGraphValue's start value (stacked_perception.cpp:116)


class StackConfig(C.Structure):
    _fields_ = [
        ("n_ground", C.c_uint32), ("use_lidar_layer", C.c_int32), ("use_depth_layer", C.c_int32), ("n_host_layers", C.c_int32),
        ("n_order", C.c_int32), ("layer_order", C.c_int32 * STACK_MAX_LAYERS), ("max_changes", C.c_uint32),
    ]


class StackStats(C.Structure):
    _fields_ = [
        ("lidar", MarkingStats), ("depth", DepthLayerStats), ("lidar_rc", C.c_int32), ("depth_rc", C.c_int32),
        ("depth_skipped", C.c_uint32), ("n_changed", C.c_uint32), ("launches", C.c_uint32), ("host_waits", C.c_uint32),
    ]


class MclConfig(C.Structure):
    """dddmr_mcl_config: mcl_3dl's likelihood.* parameters (lidar_measurement_model_likelihood.cpp:49-67) and capacities."""
    _fields_ = [
        ("match_dist_min", C.c_double), ("match_dist_flat", C.c_double), ("radius_of_ground_search", C.c_double),
        ("threshold_for_trusted_ground", C.c_int32),
        ("max_map_points", C.c_uint32), ("max_ground_points", C.c_uint32), ("max_particles", C.c_uint32),
        ("max_observation_points", C.c_uint32), ("max_ground_neighbours", C.c_uint32), ("reserved", C.c_uint32),
    ]


class MclStats(C.Structure):
    _fields_ = [
        ("quality_min", C.c_float), ("quality_max", C.c_float), ("n_bad_states", C.c_uint32), ("n_over_capacity", C.c_uint32),
        ("max_ground_neighbours_seen", C.c_uint32), ("launches", C.c_uint32), ("host_waits", C.c_uint32), ("reserved", C.c_uint32),
    ]


class MclObservationConfig(C.Structure):
    """dddmr_mcl_observation_config: cbLeGoFeatureCloud's two parameters (mcl_3dl.yaml) and the input capacities."""
    _fields_ = [
        ("euc_cluster_distance", C.c_double), ("euc_cluster_min_size", C.c_int32),
        ("max_flat_points", C.c_uint32), ("max_less_sharp_points", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
    ]


class MclObservationStats(C.Structure):
    _fields_ = [
        ("n_flat_in", C.c_uint32), ("n_flat_out", C.c_uint32), ("n_less_sharp_in", C.c_uint32), ("n_less_sharp_out", C.c_uint32),
        ("branch", C.c_uint32), ("n_clusters", C.c_uint32), ("n_small_clusters", C.c_uint32), ("n_nan_normals", C.c_uint32),
        ("sum_normal_x", C.c_double), ("sum_normal_y", C.c_double), ("launches", C.c_uint32), ("host_waits", C.c_uint32),
    ]


class MclFilterConfig(C.Structure):
    """dddmr_mcl_filter_config: the motion model's time constants and the bias variances (doubles in mcl_3dl's Parameters)."""
    _fields_ = [
        ("max_particles", C.c_uint32), ("reserved", C.c_uint32),
        ("odom_err_integ_lin_tc", C.c_double), ("odom_err_integ_ang_tc", C.c_double),
        ("bias_var_dist", C.c_double), ("bias_var_ang", C.c_double),
    ]


class MclFilterEstimate(C.Structure):
    """dddmr_mcl_filter_estimate: what MCL3dlNode::measure reads of the particle set after pf_->measure."""
    _fields_ = [
        ("mean_biased", C.c_float * 7), ("mean", C.c_float * 7), ("max_state", C.c_float * 13), ("max_index", C.c_uint32),
        ("cov", C.c_float * 36), ("sums_biased", C.c_float * 10), ("sums", C.c_float * 10),
        ("weight_sum", C.c_float), ("bias_sum", C.c_float), ("p_num", C.c_uint32), ("restored", C.c_uint32),
        ("quality_min", C.c_float), ("quality_max", C.c_float), ("launches", C.c_uint32), ("host_waits", C.c_uint32),
    ]


class MclFilterResampleStats(C.Structure):
    _fields_ = [
        ("n_duplicates", C.c_uint32), ("n_at_end", C.c_uint32), ("n_ties", C.c_uint32),
        ("launches", C.c_uint32), ("host_waits", C.c_uint32), ("reserved", C.c_uint32),
    ]


class SubmapConfig(C.Structure):
    """dddmr_submap_config: the keyframe store's capacities and NormalEstimation's setKSearch."""
    _fields_ = [
        ("max_keyframes", C.c_uint32), ("max_store_map_points", C.c_uint32), ("max_store_ground_points", C.c_uint32),
        ("normal_k", C.c_uint32), ("reserved", C.c_uint32 * 2),
    ]


class SubmapStats(C.Structure):
    _fields_ = [
        ("n_keyframes", C.c_uint32), ("n_map", C.c_uint32), ("n_ground", C.c_uint32), ("n_nan_normals", C.c_uint32),
        ("max_rings_searched", C.c_uint32), ("launches", C.c_uint32), ("host_waits", C.c_uint32), ("n_brute_force", C.c_uint32),
    ]


class StaticLayerConfig(C.Structure):
    """dddmr_static_layer_config: static_layer.cpp's parameters, the two global radii and the capacities."""
    _fields_ = [
        ("max_ground_points", C.c_uint32), ("max_map_points", C.c_uint32), ("max_edges", C.c_uint32),
        ("use_adaptive_connection", C.c_int32), ("adaptive_connection_number", C.c_uint32),
        ("enable_edge_detection", C.c_int32), ("generate_static_graph", C.c_int32), ("reserved", C.c_uint32),
        ("radius_of_ground_connection", C.c_double), ("static_imposing_radius", C.c_double),
        ("inscribed_radius", C.c_double), ("max_obstacle_distance", C.c_double),
    ]


class StaticLayerStats(C.Structure):
    _fields_ = [
        ("n_edges", C.c_uint64), ("n_ground", C.c_uint32), ("n_map", C.c_uint32), ("max_degree", C.c_uint32), ("n_long_rows", C.c_uint32),
        ("n_overhang", C.c_uint32), ("n_near_obstacle", C.c_uint32), ("n_zone_points", C.c_uint32), ("n_zone_nodes", C.c_uint32),
        ("launches", C.c_uint32), ("host_waits", C.c_uint32),
    ]


class GlobalPlanConfig(C.Structure):
    """dddmr_global_plan_config: A_Star_on_PreGraph's parameters, where the dGraph comes from, and the capacities."""
    _fields_ = [
        ("turning_weight", C.c_double), ("a_star_expanding_radius", C.c_double), ("inscribed_radius", C.c_double),
        ("inflation_descending_rate", C.c_double), ("dgraph_source", C.c_int32), ("max_queries", C.c_uint32),
        ("max_open_entries", C.c_uint32), ("max_expansions", C.c_uint32),
    ]


class GlobalPlanResult(C.Structure):
    _fields_ = [
        ("status", C.c_uint32), ("path_offset", C.c_uint32), ("path_len", C.c_uint32), ("n_expanded", C.c_uint32), ("n_pushed", C.c_uint32),
        ("n_discarded_closed", C.c_uint32), ("g_goal", C.c_float), ("host_waits", C.c_uint32),
    ]


class GlobalPlanCloudResult(C.Structure):
    """dddmr_global_plan_cloud_result (56 bytes; pinned by global_plan_cloud.hip.h and tests/test_global_plan_cloud_cpu.py)"""
    _fields_ = [
        ("plan", GlobalPlanResult), ("n_knn_fallbacks", C.c_uint32), ("n_lethal_skipped", C.c_uint32), ("n_los_tested", C.c_uint32),
        ("n_los_blocked", C.c_uint32), ("n_los_capped", C.c_uint32), ("max_successors", C.c_uint32),
    ]


GLOBAL_PLAN_MAX_QUERIES = 16
GLOBAL_PLAN_FOUND, GLOBAL_PLAN_NO_PATH, GLOBAL_PLAN_BUDGET, GLOBAL_PLAN_OPEN_FULL = 0, 1, 2, 3
GLOBAL_PLAN_NONE = 0xFFFFFFFF             # global_plan_nearest: no ground node inside the radius
GLOBAL_PLAN_ROW_FULL = 4                  # global_plan_plan_on_cloud: a radius search found more than ..._CLOUD_MAX_SUCCESSORS
GLOBAL_PLAN_CLOUD_MAX_SUCCESSORS, GLOBAL_PLAN_LOS_MAX_SAMPLES = 1024, 4096

MCL_BRANCH_CLUSTERS, MCL_BRANCH_X_DOMINANT, MCL_BRANCH_Y_DOMINANT = 0, 1, 2


# dddmr_rollout_depth_clear_verdicts: bit 0 of a verdict = kept, bits 1-2 = the branch that decided
DEPTH_CLEAR_KEPT = 1
DEPTH_CLEAR_OUTSIDE, DEPTH_CLEAR_ATTACHED, DEPTH_CLEAR_INSIDE = 1, 2, 3


class RolloutDebug(C.Structure):
    _fields_ = [
        ("costs", C.POINTER(C.c_double)),
        ("steps", C.POINTER(C.c_int32)),
        ("samples", C.POINTER(C.c_float)),
    ]


# the structs dddmr_rollout_sizeof knows, in its order (rollout_engine.hip: case 0 .. 22; the sub-map structs
# are pinned by static_asserts in mcl_submap.hip.h and by tests/test_submap_cpu.py instead, the static layer's by
# static_layer.hip.h and tests/test_static_layer_cpu.py, the global planner's by global_plan.hip.h and
# tests/test_global_plan_cpu.py)
SIZEOF_STRUCTS = (
    CriticConfig, TheoryConfig, RolloutConfig, TickInput, RolloutResult, RolloutDebug, MarkingConfig, MarkingStats,
    DepthSourceConfig, DepthImageConfig, DepthFrustumConfig, DepthMarkConfig, DepthMarkStats, DepthLayerConfig,
    DepthLayerStats, StackConfig, StackStats, LidarSweepConfig, MclConfig, MclStats, LidarFeaturesConfig,
    MclObservationConfig, MclObservationStats,
)

_P = C.POINTER
_int, _i32, _u32, _i64, _sz, _dbl, _str = C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_size_t, C.c_double, C.c_char_p
_ctx = _vp = C.c_void_p
_pd, _pu, _pn, _pi64 = _P(_dbl), _P(_u32), _P(_sz), _P(_i64)
_cloud = [_vp, _sz, _sz]                      # records, count, stride in bytes
_get = (_int, [_ctx, _vp, _sz, _pn])          # the two-call getter: buffer, capacity, count
_get_of = (_int, [_ctx, _i32, _vp, _sz, _pn])     # ... of a source
_fixed = (_int, [_ctx, _vp, _sz])             # n values into a buffer (also set_prune_plan)
_plain = (_int, [_ctx])

# name without the dddmr_rollout_ prefix -> (restype, argtypes), in the header's order
_TABLE = {
    "create": (_int, [_P(RolloutConfig), _P(_ctx)]),
    "destroy": (None, [_ctx]),
    "set_cloud": (_int, [_ctx] + _cloud),
    "set_scan": (_int, [_ctx] + _cloud + [_pd, _pd, _dbl, _dbl, _pu]),
    "set_stitcher": (_int, [_ctx, _i32]),
    "get_cloud": _get,
    "set_prune_plan": _fixed,
    "samples": (_int, [_ctx, _str, _P(TickInput), _vp, _sz, _pn]),
    "tick": (_int, [_ctx, _str, _P(TickInput), _P(RolloutResult)]),
    "tick_begin": (_int, [_ctx, _str, _P(TickInput)]),
    "tick_end": (_int, [_ctx, _P(RolloutResult)]),
    "resolve": (_int, [_ctx, _i64, _P(RolloutResult)]),
    "winner_words": (None, [_P(RolloutResult), _pi64]),
    "resolve_words": (_int, [_ctx, _pi64, _i32, _P(RolloutResult)]),
    "get_debug": (_int, [_ctx, _P(RolloutDebug)]),
    "heading_rows": _plain,
    "fused_walk": _plain,
    "score_paths": _plain,
    "deal": _plain,
    "get_deal": (_int, [_ctx, _vp, _vp, _sz, _pn, _P(_i32)]),
    "get_best_poses": _get,
    "get_best_cuboids": _get,
    "get_pose_arrays": _get_of,
    "path_blocked": (_int, [_ctx, _vp, _sz, _dbl, _pd, _P(_i32), _vp]),
    "pack_key": (_i64, [_dbl, _u32]),
    "key_index": (_i32, [_i64]),
    "comm_unique_id": (_int, [_vp]),
    "comm_init": (_int, [_ctx, _vp, _i32, _i32]),
    "comm_destroy": _plain,
    "comm_ranks": (_int, [_ctx, _P(_i32)]),
    "device_count": (_int, [_P(_i32)]),
    "comm_loopback": _plain,
    "comm_loopback_set_peer": (_int, [_ctx, _i32, _pi64]),
    "marking_create": (_int, [_ctx, _P(MarkingConfig)] + _cloud + _cloud),
    "marking_update": (_int, [_ctx, _pd, _pd, _P(MarkingStats)]),
    "marking_reset": _plain,
    "marking_get_voxels": _get,
    "marking_get_points": (_int, [_ctx, _vp, _vp, _sz, _pn]),
    "marking_get_dgraph": _fixed,
    "marking_get_lethal": _fixed,
    "marking_route_counts": (_int, [_ctx, _pu, _pu, _pu]),
    "set_scan_source": (_int, [_ctx, _i32] + _cloud + [_pd, _pd, _dbl, _dbl, _pu, _pu]),
    "set_stitcher_source": (_int, [_ctx, _i32, _i32]),
    "set_depth_source": (_int, [_ctx, _i32, _P(DepthSourceConfig)]),
    "set_depth_frame": (_int, [_ctx, _i32] + _cloud + [_pd, _pd, _i64, _pu, _pu, _pu]),
    "set_depth_image_source": (_int, [_ctx, _i32, _P(DepthSourceConfig), _P(DepthImageConfig)]),
    "set_depth_image": (_int, [_ctx, _i32, _vp, _sz, _pd, _pd, _i64, _pu, _pu, _pu, _pu]),
    "get_depth_image_cloud": _get_of,
    "set_lidar_sweep_source": (_int, [_ctx, _i32, _P(LidarSweepConfig)]),
    "set_lidar_sweep": (_int, [_ctx, _i32] + _cloud + [_pd, _pd, _dbl, _dbl, _pu, _pu, _pu]),
    "get_lidar_sweep_cloud": _get_of,
    "get_lidar_sweep_image": (_int, [_ctx, _i32, _vp, _vp, _vp, _sz]),
    "set_lidar_sweep_features": (_int, [_ctx, _i32, _P(LidarFeaturesConfig)]),
    "get_lidar_sweep_segmented": (_int, [_ctx, _i32] + [_vp] * 6 + [_sz, _pn]),
    "get_lidar_sweep_features": (_int, [_ctx, _i32, _int, _vp, _vp, _sz, _pn]),
    "set_lidar_sweep_association": (_int, [_ctx, _i32, _i32, _dbl]),
    "get_lidar_sweep_orientation": (_int, [_ctx, _i32, _vp, _P(_i32)]),
    "get_lidar_sweep_times": _get_of,
    "get_lidar_sweep_association": (_int, [_ctx, _i32, _int, _int, _vp, _vp, _sz, _pn]),
    "get_lidar_sweep_outliers": _get_of,
    "set_depth_frustum": (_int, [_ctx, _i32, _P(DepthFrustumConfig), _pd]),
    "get_depth_frustum": (_int, [_ctx, _i32, _vp, _vp, _vp, _vp]),
    "depth_frustum_test": (_int, [_ctx] + _cloud + [_vp, _vp]),
    "depth_clear_verdicts": (_int, [_ctx, _dbl, _dbl, _vp, _vp, _vp, _sz, _vp, _vp]),
    "depth_clear_launches": (_int, [_ctx, _pu]),
    "depth_mark_create": (_int, [_ctx, _P(DepthMarkConfig)] + _cloud + _cloud),
    "depth_mark_clusters": (_int, [_ctx, _pd, _sz, _sz] + [_vp] * 6 + [_P(DepthMarkStats)]),
    "depth_layer_create": (_int, [_ctx, _P(DepthLayerConfig)] + _cloud + _cloud),
    "depth_layer_update": (_int, [_ctx, _pd, _P(DepthLayerStats)]),
    "depth_layer_reset": _plain,
    "depth_layer_get_voxels": _get,
    "depth_layer_get_clusters": (_int, [_ctx, _vp, _vp, _vp, _sz, _sz, _pn, _pn]),
    "depth_layer_get_dgraph": _fixed,
    "depth_layer_get_lethal": _fixed,
    "stack_create": (_int, [_ctx, _P(StackConfig)]),
    "stack_set_host_layer": (_int, [_ctx, _i32, _vp]),
    "stack_update": (_int, [_ctx, _pd, _pd, _P(StackStats)]),
    "stack_get_changes": (_int, [_ctx, _vp, _vp, _vp, _sz, _pn]),
    "stack_get_min_dgraph": _fixed,
    "stack_get_lethal_mask": _fixed,
    "stack_get_lethal_nodes": _get,
    "stack_reset": _plain,
    "mcl_create": (_int, [_ctx, _P(MclConfig)]),
    "mcl_set_map": (_int, [_ctx] + _cloud + [_vp, _vp, _sz, _sz, _sz]),
    "mcl_measure": (_int, [_ctx, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _P(MclStats)]),
    "mcl_get_terms": (_int, [_ctx] + [_vp] * 5 + [_sz]),
    "mcl_set_observation_config": (_int, [_ctx, _P(MclObservationConfig)]),
    "mcl_prepare": (_int, [_ctx] + _cloud + _cloud + [_pd, _P(MclObservationStats)]),
    "mcl_prepare_from_sweep": (_int, [_ctx, _i32, _pd, _P(MclObservationStats)]),
    "mcl_get_observation": (_int, [_ctx, _vp, _sz, _pn, _vp, _sz, _pn, _vp, _sz]),
    "mcl_measure_prepared": (_int, [_ctx, _vp, _sz, _vp, _vp, _P(MclStats)]),
    "mcl_filter_create": (_int, [_ctx, _P(MclFilterConfig)]),
    "mcl_filter_set_particles": (_int, [_ctx, _vp, _vp, _vp, _sz]),
    "mcl_filter_get_particles": (_int, [_ctx, _vp, _vp, _vp, _vp, _sz, _pn]),
    "mcl_filter_predict": (_int, [_ctx, _vp, _vp, _dbl]),
    "mcl_filter_set_noise": (_int, [_ctx, _vp, _sz]),
    "mcl_filter_measure": (_int, [_ctx, _vp, _vp, _sz, _vp, _P(MclFilterEstimate), _P(MclStats)]),
    "mcl_filter_reset_integ": _plain,
    "mcl_filter_resample": (_int, [_ctx, _dbl, _vp, _sz, _P(MclFilterResampleStats)]),
    "mcl_filter_add_noise": (_int, [_ctx, _vp, _sz]),
    "submap_create": (_int, [_ctx, _P(SubmapConfig)]),
    "submap_add_keyframe": (_int, [_ctx] + _cloud + _cloud + [_pd, _pd, _vp]),
    "submap_select": (_int, [_ctx, _pd, _dbl, _vp, _sz, _pn]),
    "submap_warm_up": (_int, [_ctx, _vp, _sz, _P(SubmapStats)]),
    "submap_swap": _plain,
    "submap_get": (_int, [_ctx, _i32, _vp, _sz, _pn, _vp, _vp, _vp, _sz, _pn]),
    "static_layer_create": (_int, [_ctx, _P(StaticLayerConfig)]),
    "static_layer_build": (_int, [_ctx] + _cloud + _cloud + [_P(StaticLayerStats)]),
    "static_layer_get_graph": (_int, [_ctx, _vp, _vp, _vp, _sz, _pn]),
    "static_layer_get_dgraph": _fixed,
    "static_layer_set_zones": (_int, [_ctx] + _cloud + [_dbl, _P(StaticLayerStats)]),
    "static_layer_get_zone_dgraph": _fixed,
    "static_layer_bind": (_int, [_ctx, _i32, _i32]),
    "global_plan_create": (_int, [_ctx, _P(GlobalPlanConfig)]),
    "global_plan_set_node_weights": _fixed,
    "global_plan_nearest": (_int, [_ctx, _vp, _sz, _vp]),
    "global_plan_probe": (_int, [_ctx, _vp, _sz, _vp, _vp]),
    "global_plan_plan": (_int, [_ctx, _vp, _vp, _sz, _vp, _sz, _P(GlobalPlanResult)]),
    "global_plan_set_graph_node_weights": _fixed,
    "global_plan_set_lethal_points": (_int, [_ctx] + _cloud),
    "global_plan_plan_on_cloud": (_int, [_ctx, _vp, _vp, _sz, _vp, _sz, _P(GlobalPlanCloudResult)]),
    "stream_ceiling": (_int, [_ctx, _sz, _i32, _pd, _pd]),
    "selftest_sincos": (_int, [_ctx, _vp, _sz, _vp, _vp]),
    "selftest_wave_ops": (_int, [_ctx, _vp, _vp, _sz, _u32, _vp, _vp]),
    "selftest_wave_wide": (_int, [_ctx, _vp, _sz, _vp, _u32, _vp, _vp, _vp]),
    "selftest_point_grid": (_int, [_ctx, _vp, _sz, _vp, _vp, _vp, _u32, _vp, _sz, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "last_error": (_str, [_ctx]),
    "version": (_str, []),
    "sizeof": (_sz, [_int]),                  # the layout self-check of the CPU tests
}
SIGNATURES = {"dddmr_rollout_" + name: sig for name, sig in _TABLE.items()}
NOT_IN_HEADER = ("dddmr_rollout_sizeof",)
# every symbol include/dddmr_rollout.h declares
EXPORTED_SYMBOLS = tuple(name for name in SIGNATURES if name not in NOT_IN_HEADER)

_LIB_NAME = "libdddmr_rollout.so"
_lib = None


def library_path() -> str:
    # DDDMR_LIB_NAME selects the diagnostic build (phase stamps) for tools/phase_stamps.py
    name = os.environ.get("DDDMR_LIB_NAME", _LIB_NAME)
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", name)


def load_library() -> C.CDLL:
    """Load the HIP engine and bind SIGNATURES.  Raises (never falls back) if it is not built.  The shipped library
    must export every entry; one that DDDMR_LIB_NAME selects (a diagnostic build, a measurement tool's build of an older
    commit) may lack some, and calling one of those raises AttributeError."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the rollout engine."
        )
    lib = C.CDLL(path)
    shipped = "DDDMR_LIB_NAME" not in os.environ
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if shipped:
                raise RuntimeError(f"{path} does not export {name}: rebuild it from this tree") from None
            continue
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib

