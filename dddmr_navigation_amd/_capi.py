"""ctypes view of include/dddmr_rollout.h (the C-ABI of the rollout engine).

The struct layouts here mirror the header field by field; `tests/test_capi_cpu.py`
checks sizeof() of every struct against the compiled library
(`dddmr_rollout_sizeof`) so the two cannot drift apart silently.

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


# every symbol include/dddmr_rollout.h declares
EXPORTED_SYMBOLS = (
    "dddmr_rollout_create",
    "dddmr_rollout_destroy",
    "dddmr_rollout_set_cloud",
    "dddmr_rollout_set_scan",
    "dddmr_rollout_set_stitcher",
    "dddmr_rollout_get_cloud",
    "dddmr_rollout_set_prune_plan",
    "dddmr_rollout_samples",
    "dddmr_rollout_tick",
    "dddmr_rollout_tick_begin",
    "dddmr_rollout_tick_end",
    "dddmr_rollout_resolve",
    "dddmr_rollout_winner_words",
    "dddmr_rollout_resolve_words",
    "dddmr_rollout_get_debug",
    "dddmr_rollout_heading_rows",
    "dddmr_rollout_fused_walk",
    "dddmr_rollout_get_best_poses",
    "dddmr_rollout_get_best_cuboids",
    "dddmr_rollout_get_pose_arrays",
    "dddmr_rollout_path_blocked",
    "dddmr_rollout_pack_key",
    "dddmr_rollout_key_index",
    "dddmr_rollout_comm_unique_id",
    "dddmr_rollout_comm_init",
    "dddmr_rollout_comm_destroy",
    "dddmr_rollout_comm_ranks",
    "dddmr_rollout_device_count",
    "dddmr_rollout_comm_loopback",
    "dddmr_rollout_comm_loopback_set_peer",
    "dddmr_rollout_marking_create",
    "dddmr_rollout_marking_update",
    "dddmr_rollout_marking_reset",
    "dddmr_rollout_marking_get_voxels",
    "dddmr_rollout_marking_get_points",
    "dddmr_rollout_marking_get_dgraph",
    "dddmr_rollout_marking_get_lethal",
    "dddmr_rollout_marking_route_counts",
    "dddmr_rollout_set_scan_source",
    "dddmr_rollout_set_stitcher_source",
    "dddmr_rollout_set_depth_source",
    "dddmr_rollout_set_depth_frame",
    "dddmr_rollout_set_depth_image_source",
    "dddmr_rollout_set_depth_image",
    "dddmr_rollout_get_depth_image_cloud",
    "dddmr_rollout_set_lidar_sweep_source",
    "dddmr_rollout_set_lidar_sweep",
    "dddmr_rollout_get_lidar_sweep_cloud",
    "dddmr_rollout_get_lidar_sweep_image",
    "dddmr_rollout_set_lidar_sweep_features",
    "dddmr_rollout_get_lidar_sweep_segmented",
    "dddmr_rollout_get_lidar_sweep_features",
    "dddmr_rollout_set_depth_frustum",
    "dddmr_rollout_get_depth_frustum",
    "dddmr_rollout_depth_frustum_test",
    "dddmr_rollout_depth_clear_verdicts",
    "dddmr_rollout_depth_clear_launches",
    "dddmr_rollout_depth_mark_create",
    "dddmr_rollout_depth_mark_clusters",
    "dddmr_rollout_depth_layer_create",
    "dddmr_rollout_depth_layer_update",
    "dddmr_rollout_depth_layer_reset",
    "dddmr_rollout_depth_layer_get_voxels",
    "dddmr_rollout_depth_layer_get_clusters",
    "dddmr_rollout_depth_layer_get_dgraph",
    "dddmr_rollout_depth_layer_get_lethal",
    "dddmr_rollout_stack_create",
    "dddmr_rollout_stack_set_host_layer",
    "dddmr_rollout_stack_update",
    "dddmr_rollout_stack_get_changes",
    "dddmr_rollout_stack_get_min_dgraph",
    "dddmr_rollout_stack_get_lethal_mask",
    "dddmr_rollout_stack_get_lethal_nodes",
    "dddmr_rollout_stack_reset",
    "dddmr_rollout_mcl_create",
    "dddmr_rollout_mcl_set_map",
    "dddmr_rollout_mcl_measure",
    "dddmr_rollout_mcl_get_terms",
    "dddmr_rollout_mcl_set_observation_config",
    "dddmr_rollout_mcl_prepare",
    "dddmr_rollout_mcl_prepare_from_sweep",
    "dddmr_rollout_mcl_get_observation",
    "dddmr_rollout_mcl_measure_prepared",
    "dddmr_rollout_stream_ceiling",
    "dddmr_rollout_selftest_sincos",
    "dddmr_rollout_last_error",
    "dddmr_rollout_version",
)

_LIB_NAME = "libdddmr_rollout.so"
_lib = None


def library_path() -> str:
    # DDDMR_LIB_NAME selects the diagnostic build (phase stamps) for tools/phase_stamps.py
    name = os.environ.get("DDDMR_LIB_NAME", _LIB_NAME)
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", name)


def load_library() -> C.CDLL:
    """Load the HIP engine.  Raises (never falls back) if it is not built."""
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
    ctx_p = C.c_void_p
    lib.dddmr_rollout_create.argtypes = [C.POINTER(RolloutConfig), C.POINTER(ctx_p)]
    lib.dddmr_rollout_create.restype = C.c_int
    lib.dddmr_rollout_destroy.argtypes = [ctx_p]
    lib.dddmr_rollout_destroy.restype = None
    lib.dddmr_rollout_set_cloud.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_size_t]
    lib.dddmr_rollout_set_cloud.restype = C.c_int
    lib.dddmr_rollout_set_scan.argtypes = [
        ctx_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double),
        C.c_double, C.c_double, C.POINTER(C.c_uint32)]
    lib.dddmr_rollout_set_scan.restype = C.c_int
    lib.dddmr_rollout_set_stitcher.argtypes = [ctx_p, C.c_int32]
    lib.dddmr_rollout_set_stitcher.restype = C.c_int
    lib.dddmr_rollout_get_cloud.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_get_cloud.restype = C.c_int
    lib.dddmr_rollout_set_prune_plan.argtypes = [ctx_p, C.c_void_p, C.c_size_t]
    lib.dddmr_rollout_set_prune_plan.restype = C.c_int
    lib.dddmr_rollout_samples.argtypes = [ctx_p, C.c_char_p, C.POINTER(TickInput), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_samples.restype = C.c_int
    lib.dddmr_rollout_tick.argtypes = [ctx_p, C.c_char_p, C.POINTER(TickInput), C.POINTER(RolloutResult)]
    lib.dddmr_rollout_tick.restype = C.c_int
    lib.dddmr_rollout_tick_begin.argtypes = [ctx_p, C.c_char_p, C.POINTER(TickInput)]
    lib.dddmr_rollout_tick_begin.restype = C.c_int
    lib.dddmr_rollout_tick_end.argtypes = [ctx_p, C.POINTER(RolloutResult)]
    lib.dddmr_rollout_tick_end.restype = C.c_int
    lib.dddmr_rollout_resolve.argtypes = [ctx_p, C.c_int64, C.POINTER(RolloutResult)]
    lib.dddmr_rollout_resolve.restype = C.c_int
    lib.dddmr_rollout_winner_words.argtypes = [C.POINTER(RolloutResult), C.POINTER(C.c_int64)]
    lib.dddmr_rollout_winner_words.restype = None
    lib.dddmr_rollout_resolve_words.argtypes = [ctx_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(RolloutResult)]
    lib.dddmr_rollout_resolve_words.restype = C.c_int
    lib.dddmr_rollout_get_debug.argtypes = [ctx_p, C.POINTER(RolloutDebug)]
    lib.dddmr_rollout_get_debug.restype = C.c_int
    # (a library built from an older commit, loaded through DDDMR_LIB_NAME by the measurement jobs, has no such entry)
    if hasattr(lib, "dddmr_rollout_heading_rows"):
        lib.dddmr_rollout_heading_rows.argtypes = [ctx_p]
        lib.dddmr_rollout_heading_rows.restype = C.c_int
    if hasattr(lib, "dddmr_rollout_fused_walk"):
        lib.dddmr_rollout_fused_walk.argtypes = [ctx_p]
        lib.dddmr_rollout_fused_walk.restype = C.c_int
    lib.dddmr_rollout_get_best_poses.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_get_best_poses.restype = C.c_int
    lib.dddmr_rollout_get_best_cuboids.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_get_best_cuboids.restype = C.c_int
    lib.dddmr_rollout_get_pose_arrays.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_get_pose_arrays.restype = C.c_int
    lib.dddmr_rollout_path_blocked.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_double, C.POINTER(C.c_double),
                                               C.POINTER(C.c_int32), C.c_void_p]
    lib.dddmr_rollout_path_blocked.restype = C.c_int
    lib.dddmr_rollout_pack_key.argtypes = [C.c_double, C.c_uint32]
    lib.dddmr_rollout_pack_key.restype = C.c_int64
    lib.dddmr_rollout_key_index.argtypes = [C.c_int64]
    lib.dddmr_rollout_key_index.restype = C.c_int32
    lib.dddmr_rollout_comm_unique_id.argtypes = [C.c_void_p]
    lib.dddmr_rollout_comm_unique_id.restype = C.c_int
    lib.dddmr_rollout_comm_init.argtypes = [ctx_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.dddmr_rollout_comm_init.restype = C.c_int
    lib.dddmr_rollout_comm_destroy.argtypes = [ctx_p]
    lib.dddmr_rollout_comm_destroy.restype = C.c_int
    lib.dddmr_rollout_device_count.argtypes = [C.POINTER(C.c_int32)]
    lib.dddmr_rollout_device_count.restype = C.c_int
    lib.dddmr_rollout_comm_ranks.argtypes = [ctx_p, C.POINTER(C.c_int32)]
    lib.dddmr_rollout_comm_ranks.restype = C.c_int
    lib.dddmr_rollout_comm_loopback.argtypes = [ctx_p]
    lib.dddmr_rollout_comm_loopback.restype = C.c_int
    lib.dddmr_rollout_comm_loopback_set_peer.argtypes = [ctx_p, C.c_int32, C.POINTER(C.c_int64)]
    lib.dddmr_rollout_comm_loopback_set_peer.restype = C.c_int
    lib.dddmr_rollout_marking_create.argtypes = [ctx_p, C.POINTER(MarkingConfig), C.c_void_p, C.c_size_t, C.c_size_t,
                                                 C.c_void_p, C.c_size_t, C.c_size_t]
    lib.dddmr_rollout_marking_create.restype = C.c_int
    lib.dddmr_rollout_marking_update.argtypes = [ctx_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(MarkingStats)]
    lib.dddmr_rollout_marking_update.restype = C.c_int
    lib.dddmr_rollout_marking_reset.argtypes = [ctx_p]
    lib.dddmr_rollout_marking_reset.restype = C.c_int
    lib.dddmr_rollout_marking_get_voxels.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_marking_get_voxels.restype = C.c_int
    lib.dddmr_rollout_marking_get_points.argtypes = [ctx_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_marking_get_points.restype = C.c_int
    lib.dddmr_rollout_marking_get_dgraph.argtypes = [ctx_p, C.c_void_p, C.c_size_t]
    lib.dddmr_rollout_marking_get_dgraph.restype = C.c_int
    lib.dddmr_rollout_marking_get_lethal.argtypes = [ctx_p, C.c_void_p, C.c_size_t]
    lib.dddmr_rollout_marking_get_lethal.restype = C.c_int
    lib.dddmr_rollout_marking_route_counts.argtypes = [ctx_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.dddmr_rollout_marking_route_counts.restype = C.c_int
    lib.dddmr_rollout_set_scan_source.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.dddmr_rollout_set_scan_source.restype = C.c_int
    lib.dddmr_rollout_set_stitcher_source.argtypes = [ctx_p, C.c_int32, C.c_int32]
    lib.dddmr_rollout_set_stitcher_source.restype = C.c_int
    lib.dddmr_rollout_set_depth_source.argtypes = [ctx_p, C.c_int32, C.POINTER(DepthSourceConfig)]
    lib.dddmr_rollout_set_depth_source.restype = C.c_int
    lib.dddmr_rollout_set_depth_frame.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_uint32)]
    lib.dddmr_rollout_set_depth_frame.restype = C.c_int
    lib.dddmr_rollout_set_depth_image_source.argtypes = [ctx_p, C.c_int32, C.POINTER(DepthSourceConfig), C.POINTER(DepthImageConfig)]
    lib.dddmr_rollout_set_depth_image_source.restype = C.c_int
    lib.dddmr_rollout_set_depth_image.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                  C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_uint32)]
    lib.dddmr_rollout_set_depth_image.restype = C.c_int
    lib.dddmr_rollout_get_depth_image_cloud.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_get_depth_image_cloud.restype = C.c_int
    # (a library built from an older commit, loaded through DDDMR_LIB_NAME by tools/lidar_sweep_bench.py, has no sweep entries)
    if hasattr(lib, "dddmr_rollout_set_lidar_sweep_source"):
        lib.dddmr_rollout_set_lidar_sweep_source.argtypes = [ctx_p, C.c_int32, C.POINTER(LidarSweepConfig)]
        lib.dddmr_rollout_set_lidar_sweep_source.restype = C.c_int
        lib.dddmr_rollout_set_lidar_sweep.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_uint32),
                                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.dddmr_rollout_set_lidar_sweep.restype = C.c_int
        lib.dddmr_rollout_get_lidar_sweep_cloud.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.dddmr_rollout_get_lidar_sweep_cloud.restype = C.c_int
        lib.dddmr_rollout_get_lidar_sweep_image.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.dddmr_rollout_get_lidar_sweep_image.restype = C.c_int
    if hasattr(lib, "dddmr_rollout_set_lidar_sweep_features"):         # (absent from a library built from an older commit)
        lib.dddmr_rollout_set_lidar_sweep_features.argtypes = [ctx_p, C.c_int32, C.POINTER(LidarFeaturesConfig)]
        lib.dddmr_rollout_set_lidar_sweep_features.restype = C.c_int
        lib.dddmr_rollout_get_lidar_sweep_segmented.argtypes = [ctx_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_size_t, C.POINTER(C.c_size_t)]
        lib.dddmr_rollout_get_lidar_sweep_segmented.restype = C.c_int
        lib.dddmr_rollout_get_lidar_sweep_features.argtypes = [ctx_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                               C.POINTER(C.c_size_t)]
        lib.dddmr_rollout_get_lidar_sweep_features.restype = C.c_int
    lib.dddmr_rollout_set_depth_frustum.argtypes = [ctx_p, C.c_int32, C.POINTER(DepthFrustumConfig), C.POINTER(C.c_double)]
    lib.dddmr_rollout_set_depth_frustum.restype = C.c_int
    lib.dddmr_rollout_get_depth_frustum.argtypes = [ctx_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dddmr_rollout_get_depth_frustum.restype = C.c_int
    lib.dddmr_rollout_depth_frustum_test.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.dddmr_rollout_depth_frustum_test.restype = C.c_int
    lib.dddmr_rollout_depth_clear_verdicts.argtypes = [ctx_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                       C.c_void_p, C.c_void_p]
    lib.dddmr_rollout_depth_clear_verdicts.restype = C.c_int
    lib.dddmr_rollout_depth_clear_launches.argtypes = [ctx_p, C.POINTER(C.c_uint32)]
    lib.dddmr_rollout_depth_clear_launches.restype = C.c_int
    lib.dddmr_rollout_depth_mark_create.argtypes = [ctx_p, C.POINTER(DepthMarkConfig), C.c_void_p, C.c_size_t, C.c_size_t,
                                                    C.c_void_p, C.c_size_t, C.c_size_t]
    lib.dddmr_rollout_depth_mark_create.restype = C.c_int
    lib.dddmr_rollout_depth_mark_clusters.argtypes = [ctx_p, C.POINTER(C.c_double), C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DepthMarkStats)]
    lib.dddmr_rollout_depth_mark_clusters.restype = C.c_int
    lib.dddmr_rollout_depth_layer_create.argtypes = [ctx_p, C.POINTER(DepthLayerConfig), C.c_void_p, C.c_size_t, C.c_size_t,
                                                     C.c_void_p, C.c_size_t, C.c_size_t]
    lib.dddmr_rollout_depth_layer_create.restype = C.c_int
    lib.dddmr_rollout_depth_layer_update.argtypes = [ctx_p, C.POINTER(C.c_double), C.POINTER(DepthLayerStats)]
    lib.dddmr_rollout_depth_layer_update.restype = C.c_int
    lib.dddmr_rollout_depth_layer_reset.argtypes = [ctx_p]
    lib.dddmr_rollout_depth_layer_reset.restype = C.c_int
    lib.dddmr_rollout_depth_layer_get_voxels.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_depth_layer_get_voxels.restype = C.c_int
    lib.dddmr_rollout_depth_layer_get_clusters.argtypes = [ctx_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                           C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.dddmr_rollout_depth_layer_get_clusters.restype = C.c_int
    lib.dddmr_rollout_depth_layer_get_dgraph.argtypes = [ctx_p, C.c_void_p, C.c_size_t]
    lib.dddmr_rollout_depth_layer_get_dgraph.restype = C.c_int
    lib.dddmr_rollout_depth_layer_get_lethal.argtypes = [ctx_p, C.c_void_p, C.c_size_t]
    lib.dddmr_rollout_depth_layer_get_lethal.restype = C.c_int
    # (a library built from an older commit, which the measurement tools load through DDDMR_LIB_NAME, has no stack entries;
    # build() and tests/test_capi_cpu.py check that the shipped library exports every symbol, and calling a missing one raises)
    if hasattr(lib, "dddmr_rollout_stack_create"):
        lib.dddmr_rollout_stack_create.argtypes = [ctx_p, C.POINTER(StackConfig)]
        lib.dddmr_rollout_stack_create.restype = C.c_int
        lib.dddmr_rollout_stack_set_host_layer.argtypes = [ctx_p, C.c_int32, C.c_void_p]
        lib.dddmr_rollout_stack_set_host_layer.restype = C.c_int
        lib.dddmr_rollout_stack_update.argtypes = [ctx_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(StackStats)]
        lib.dddmr_rollout_stack_update.restype = C.c_int
        lib.dddmr_rollout_stack_get_changes.argtypes = [ctx_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.dddmr_rollout_stack_get_changes.restype = C.c_int
        lib.dddmr_rollout_stack_get_min_dgraph.argtypes = [ctx_p, C.c_void_p, C.c_size_t]
        lib.dddmr_rollout_stack_get_min_dgraph.restype = C.c_int
        lib.dddmr_rollout_stack_get_lethal_mask.argtypes = [ctx_p, C.c_void_p, C.c_size_t]
        lib.dddmr_rollout_stack_get_lethal_mask.restype = C.c_int
        lib.dddmr_rollout_stack_get_lethal_nodes.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.dddmr_rollout_stack_get_lethal_nodes.restype = C.c_int
        lib.dddmr_rollout_stack_reset.argtypes = [ctx_p]
        lib.dddmr_rollout_stack_reset.restype = C.c_int
    # (a library built from an older commit, loaded through DDDMR_LIB_NAME by the measurement tools, has no mcl entries)
    if hasattr(lib, "dddmr_rollout_mcl_create"):
        lib.dddmr_rollout_mcl_create.argtypes = [ctx_p, C.POINTER(MclConfig)]
        lib.dddmr_rollout_mcl_create.restype = C.c_int
        lib.dddmr_rollout_mcl_set_map.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_size_t, C.c_size_t]
        lib.dddmr_rollout_mcl_set_map.restype = C.c_int
        lib.dddmr_rollout_mcl_measure.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_void_p, C.POINTER(MclStats)]
        lib.dddmr_rollout_mcl_measure.restype = C.c_int
        lib.dddmr_rollout_mcl_get_terms.argtypes = [ctx_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.dddmr_rollout_mcl_get_terms.restype = C.c_int
    if hasattr(lib, "dddmr_rollout_mcl_prepare"):
        lib.dddmr_rollout_mcl_set_observation_config.argtypes = [ctx_p, C.POINTER(MclObservationConfig)]
        lib.dddmr_rollout_mcl_set_observation_config.restype = C.c_int
        lib.dddmr_rollout_mcl_prepare.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                                  C.POINTER(C.c_double), C.POINTER(MclObservationStats)]
        lib.dddmr_rollout_mcl_prepare.restype = C.c_int
        lib.dddmr_rollout_mcl_prepare_from_sweep.argtypes = [ctx_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(MclObservationStats)]
        lib.dddmr_rollout_mcl_prepare_from_sweep.restype = C.c_int
        lib.dddmr_rollout_mcl_get_observation.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t,
                                                          C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t]
        lib.dddmr_rollout_mcl_get_observation.restype = C.c_int
        lib.dddmr_rollout_mcl_measure_prepared.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(MclStats)]
        lib.dddmr_rollout_mcl_measure_prepared.restype = C.c_int
    lib.dddmr_rollout_stream_ceiling.argtypes = [ctx_p, C.c_size_t, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.dddmr_rollout_stream_ceiling.restype = C.c_int
    lib.dddmr_rollout_selftest_sincos.argtypes = [ctx_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.dddmr_rollout_selftest_sincos.restype = C.c_int
    lib.dddmr_rollout_last_error.argtypes = [ctx_p]
    lib.dddmr_rollout_last_error.restype = C.c_char_p
    lib.dddmr_rollout_version.argtypes = []
    lib.dddmr_rollout_version.restype = C.c_char_p
    # not part of the public header: layout self-check used by the CPU tests
    lib.dddmr_rollout_sizeof.argtypes = [C.c_int]
    lib.dddmr_rollout_sizeof.restype = C.c_size_t
    _lib = lib
    return lib
