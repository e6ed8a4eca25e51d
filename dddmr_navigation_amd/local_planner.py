"""Host-side mirror of the reference's local-planner surface on top of the C-ABI.

Names and argument meaning follow
/root/reference/src/dddmr_local_planner/local_planner/include/local_planner/local_planner.h:72-85
(`computeVelocityCommand(traj_gen_name, best_traj) -> PlannerState`, `setPlan`)
and base_trajectory/include/base_trajectory/trajectory.h:47-126 (`Trajectory`
with `xv_, yv_, thetav_, cost_`).  All compute happens in the HIP library; this
file only marshals buffers.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass
from typing import Iterable, Optional

import numpy as np

from . import _capi as K
from . import _marshal as M
from . import configs


class PlannerState(enum.IntEnum):
    """dddmr_sys_core/include/dddmr_sys_core/dddmr_enum_states.h:46-54"""
    TF_FAIL = 0
    PRUNE_PLAN_FAIL = 1
    ALL_TRAJECTORIES_FAIL = 2
    PERCEPTION_MALFUNCTION = 3
    TRAJECTORY_FOUND = 4
    PATH_BLOCKED_WAIT = 5
    PATH_BLOCKED_REPLANNING = 6


@dataclass
class Trajectory:
    """The fields consumers read from best_traj (p2p_move_base.cpp:338,415,492).
    Default-constructed values are trajectory.cpp:34-37."""
    xv_: float = 0.0
    yv_: float = 0.0
    thetav_: float = 0.0
    cost_: float = -1.0
    index: int = -1


class RolloutError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"dddmr_rollout error {code}: {msg}")
        self.code = code


def device_count() -> int:
    """HIP devices this process sees (0 without a GPU); through the library, so no torch import is needed."""
    n = C.c_int32(0)
    rc = K.load_library().dddmr_rollout_device_count(C.byref(n))
    return int(n.value) if rc == K.OK else 0


# Diagnostics of the load-feedback deal.  Functions of a planner, not methods: the methods of LocalPlanner are the set
# whose calls tests/golden/binding_trace.json records.
def deal(lp: "LocalPlanner") -> int:
    """How the last launched tick dealt the trajectories to k_score's workgroups: 0 snake, 1 sorted, 2 light tail,
    -1 before any tick (dddmr_rollout_deal)."""
    return int(lp._rc("deal"))


def score_paths(lp: "LocalPlanner") -> int:
    """Which optional paths the last launched tick's k_score took, as bits: bit 0 = the fused plan walk and the
    StickPath sums left out the rejected trajectories; -1 before any tick (dddmr_rollout_score_paths)."""
    return int(lp._rc("score_paths"))


def deal_arrays(lp: "LocalPlanner"):
    """-> (assign[n_local] u32, load[n_local] u32, assigned) of the last tick (dddmr_rollout_get_deal): assign[slot] is
    the local trajectory in that slot (slot = member * workgroups + workgroup), load[i] what trajectory i filed for the
    next tick's deal, assigned whether the tick dealt by load feedback at all (else assign is the identity)."""
    n, used = C.c_size_t(0), C.c_int32(0)
    lp._call("get_deal", None, None, 0, C.byref(n), C.byref(used))
    assign = np.zeros(max(n.value, 1), dtype=np.uint32)
    load = np.zeros(max(n.value, 1), dtype=np.uint32)
    lp._call("get_deal", M.ptr(assign), M.ptr(load), assign.size, C.byref(n), C.byref(used))
    return assign[:n.value], load[:n.value], bool(used.value)


class LocalPlanner:
    """One rollout context = the trajectory generators + critics of one robot."""

    def __init__(self, theories: Iterable[K.TheoryConfig], device: int = 0, max_points: int = 600_000,
                 max_trajectories: int = 65_536, max_steps: int = 256, max_plan_poses: int = 256,
                 rank: int = 0, world_size: int = 1):
        self._lib = K.load_library()
        self._theories = configs.theory_array(theories)
        cfg = K.RolloutConfig()
        cfg.abi_version = K.ABI_VERSION
        cfg.device = device
        cfg.rank = rank
        cfg.world_size = world_size
        cfg.max_points = max_points
        cfg.max_trajectories = max_trajectories
        cfg.max_steps = max_steps
        cfg.max_plan_poses = max_plan_poses
        cfg.n_theories = len(self._theories)
        cfg.theories = C.cast(self._theories, C.POINTER(K.TheoryConfig))
        self._ctx = C.c_void_p()
        rc = self._lib.dddmr_rollout_create(C.byref(cfg), C.byref(self._ctx))
        if rc != K.OK:
            self._ctx = C.c_void_p()
            raise RolloutError(rc, "dddmr_rollout_create failed (no CPU fallback exists; "
                                   "a HIP device and the gfx950 build are required)")
        self.last_result: Optional[K.RolloutResult] = None

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.dddmr_rollout_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc != K.OK:
            msg = self._lib.dddmr_rollout_last_error(self._ctx)
            raise RolloutError(rc, msg.decode() if msg else "")

    # -- how everything off the timed paths reaches the library (this class and the layer classes on top of it);
    # -- tick, tick_begin / tick_end, set_cloud, set_scan, setPlan and the word exchange name their function themselves
    def _rc(self, name: str, *args) -> int:
        """dddmr_rollout_<name>(ctx, *args) -> its status, for the callers that store stats before they raise."""
        return getattr(self._lib, "dddmr_rollout_" + name)(self._ctx, *args)

    def _call(self, name: str, *args):
        self._check(getattr(self._lib, "dddmr_rollout_" + name)(self._ctx, *args))

    def _get(self, name: str, lead, *outs):
        """A two-call getter dddmr_rollout_<name>(ctx, *lead, buffers..., capacity, count*): see _marshal.two_call."""
        fn = getattr(self._lib, "dddmr_rollout_" + name)
        return M.two_call(lambda *a: fn(self._ctx, *lead, *a), self._check, *outs)

    def _fixed(self, name: str, n: int, dtype, as_bool: bool = False):
        fn = getattr(self._lib, "dddmr_rollout_" + name)
        return M.fixed(lambda *a: fn(self._ctx, *a), self._check, n, dtype, as_bool)

    # -- inputs ------------------------------------------------------------
    def set_cloud(self, cloud: np.ndarray):
        """Aggregate observation, [P, >=3] float32 rows (x y z [intensity ...])."""
        _, p, n, stride = M.cloud(cloud, "cloud")
        self._check(self._lib.dddmr_rollout_set_cloud(self._ctx, p, n, stride))

    def set_scan(self, scan_xyz: np.ndarray, T_base_sensor, T_gbl_base, perception_window_size: float,
                 marking_height: float) -> int:
        """Fused local-mode perception feed (cbSensor); returns the number of
        downsampled points now forming the aggregate observation."""
        _, p, n, stride = M.cloud(scan_xyz, "scan")
        n_out = C.c_uint32(0)
        self._check(self._lib.dddmr_rollout_set_scan(self._ctx, p, n, stride, M.pose(T_base_sensor), M.pose(T_gbl_base),
                                                     perception_window_size, marking_height, C.byref(n_out)))
        return int(n_out.value)

    def set_scan_source(self, source_id: int, scan_xyz: np.ndarray, T_base_sensor, T_gbl_base, perception_window_size: float,
                        marking_height: float):
        """One of several sensors (StackedPerception::aggregateObservations, stacked_perception.cpp:128-140): returns
        (points of this sensor's observation, points of the aggregate = all sensors' latest observations in source order)."""
        _, p, n, stride = M.cloud(scan_xyz, "scan")
        n_src, n_all = C.c_uint32(0), C.c_uint32(0)
        self._call("set_scan_source", int(source_id), p, n, stride, M.pose(T_base_sensor), M.pose(T_gbl_base),
                   perception_window_size, marking_height, C.byref(n_src), C.byref(n_all))
        return int(n_src.value), int(n_all.value)

    def set_stitcher_source(self, source_id: int, stitcher_num: int):
        self._call("set_stitcher_source", int(source_id), int(stitcher_num))

    def set_depth_source(self, source_id: int, min_obstacle_height: float, max_obstacle_height: float,
                         observation_persistence_ns: int = 0, max_frame_points: int = 848 * 480, max_frames: int = 1):
        """Make `source_id` a depth camera source (DepthCameraObservationBuffer's parameters); empties a configured one."""
        cfg = K.DepthSourceConfig(float(min_obstacle_height), float(max_obstacle_height), int(observation_persistence_ns),
                                  int(max_frame_points), int(max_frames))
        self._call("set_depth_source", int(source_id), C.byref(cfg))

    def set_depth_frame(self, source_id: int, frame_xyz: np.ndarray, T_base_sensor, T_gbl_base, stamp_ns: int):
        """One depth frame through bufferCloud's local-mode steps (depth_camera_observation_buffer.cpp:78-187): returns
        (points of this frame's observation, points of the source's alive frames, points of the aggregate)."""
        _, p, n, stride = M.cloud(frame_xyz, "frame")
        n_frame, n_src, n_all = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._call("set_depth_frame", int(source_id), p, n, stride, M.pose(T_base_sensor), M.pose(T_gbl_base), int(stamp_ns),
                   C.byref(n_frame), C.byref(n_src), C.byref(n_all))
        return int(n_frame.value), int(n_src.value), int(n_all.value)

    def set_depth_image_source(self, source_id: int, min_obstacle_height: float, max_obstacle_height: float, width: int, height: int,
                               fx: float, fy: float, cx: float, cy: float, max_distance: float = 4.0, leaf_size: float = 0.05,
                               sample_step: int = 2, observation_persistence_ns: int = 0, max_frame_points: Optional[int] = None,
                               max_frames: int = 1, drop_zero: bool = False):
        """Make `source_id` a depth camera source fed 16UC1 images: DepthImg2PointCloud's parameters (defaults: the
        node's own) in front of DepthCameraObservationBuffer's.  max_frame_points bounds the sampled pixels."""
        if max_frame_points is None:
            step = max(int(sample_step), 1)
            max_frame_points = -(-int(height) // step) * -(-int(width) // step)
        cfg = K.DepthSourceConfig(float(min_obstacle_height), float(max_obstacle_height), int(observation_persistence_ns),
                                  int(max_frame_points), int(max_frames))
        icfg = K.DepthImageConfig(int(width), int(height), float(fx), float(fy), float(cx), float(cy), float(max_distance),
                                  float(leaf_size), int(sample_step), K.DEPTH_IMAGE_DROP_ZERO if drop_zero else 0)
        self._call("set_depth_image_source", int(source_id), C.byref(cfg), C.byref(icfg))

    def set_depth_image(self, source_id: int, depth_mm: np.ndarray, T_base_optical, T_gbl_base, stamp_ns: int):
        """One [height, width] uint16 millimetre image (rows may be padded: any array whose pixels of a row are adjacent is
        passed as it is) through cbDepthImg and bufferCloud: returns (stage-one points = what the node would publish,
        points of this frame's observation, points of the source's alive frames, points of the aggregate)."""
        img = np.asarray(depth_mm)
        if img.dtype != np.uint16 or img.ndim != 2:
            raise ValueError("depth image must be [height, width] uint16")
        if img.shape[1] > 1 and img.strides[1] != 2 or img.strides[0] < 2 * img.shape[1]:
            img = np.ascontiguousarray(img)
        n_cam, n_frame, n_src, n_all = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._call("set_depth_image", int(source_id), M.ptr(img), img.strides[0], M.pose(T_base_optical), M.pose(T_gbl_base),
                   int(stamp_ns), C.byref(n_cam), C.byref(n_frame), C.byref(n_src), C.byref(n_all))
        return int(n_cam.value), int(n_frame.value), int(n_src.value), int(n_all.value)

    def get_depth_image_cloud(self, source_id: int) -> np.ndarray:
        """The stage-one cloud of the source's latest image, [K,3] float32 in the optical frame (the node's
        point_cloud_from_depth topic)."""
        return self._get("get_depth_image_cloud", (int(source_id),), ((3,), np.float32))[0]

    def set_lidar_sweep_source(self, source_id: int, num_vertical_scans: int, num_horizontal_scans: int,
                               vertical_angle_bottom: float, vertical_angle_top: float, ground_scan_index: int,
                               segment_theta: float = 60.0, segment_valid_point_num: int = 5, segment_valid_line_num: int = 3,
                               minimum_detection_range: float = 0.3, maximum_detection_range: float = 100.0,
                               sensor_mount_angle: float = 0.0, max_sweep_points: Optional[int] = None, flags: int = 0):
        """Make `source_id` a lidar source fed raw sweeps: ImageProjection's laser.* / imageProjection.* parameters (angles
        in degrees as the YAML gives them) and the mount pitch in radians; empties a configured one."""
        if max_sweep_points is None:
            max_sweep_points = 2 * int(num_vertical_scans) * int(num_horizontal_scans)
        cfg = K.LidarSweepConfig(int(num_vertical_scans), int(num_horizontal_scans), float(vertical_angle_bottom),
                                 float(vertical_angle_top), int(ground_scan_index), float(segment_theta),
                                 int(segment_valid_point_num), int(segment_valid_line_num), float(minimum_detection_range),
                                 float(maximum_detection_range), float(sensor_mount_angle), int(max_sweep_points), int(flags))
        self._call("set_lidar_sweep_source", int(source_id), C.byref(cfg))

    def set_lidar_sweep(self, source_id: int, sweep_xyz: np.ndarray, T_base_sensor, T_gbl_base, perception_window_size: float,
                        marking_height: float):
        """One raw sweep through ImageProjection::cloudHandler's front half and cbSensor: returns (stage-one points = what
        the node would publish on segmented_cloud_pure, points of this source's observation, points of the aggregate)."""
        _, p, n, stride = M.cloud(sweep_xyz, "sweep")
        n_seg, n_src, n_all = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._call("set_lidar_sweep", int(source_id), p, n, stride, M.pose(T_base_sensor), M.pose(T_gbl_base),
                   perception_window_size, marking_height, C.byref(n_seg), C.byref(n_src), C.byref(n_all))
        return int(n_seg.value), int(n_src.value), int(n_all.value)

    def get_lidar_sweep_cloud(self, source_id: int) -> np.ndarray:
        """Stage one's cloud of the source's latest sweep, [K,4] float32: x y z in the pitch-removed frame and the segment
        label, in raster order (the topic segmented_cloud_pure)."""
        return self._get("get_lidar_sweep_cloud", (int(source_id),), ((4,), np.float32))[0]

    def get_lidar_sweep_image(self, source_id: int, num_vertical_scans: int, num_horizontal_scans: int):
        """(range [V,H] float32 with FLT_MAX where empty, label [V,H] int32, ground [V,H] int8) of the latest sweep."""
        V, H = int(num_vertical_scans), int(num_horizontal_scans)
        rng, lab, gnd = np.zeros((V, H), np.float32), np.zeros((V, H), np.int32), np.zeros((V, H), np.int8)
        self._call("get_lidar_sweep_image", int(source_id), M.ptr(rng), M.ptr(lab), M.ptr(gnd), V * H)
        return rng, lab, gnd

    def set_lidar_sweep_features(self, source_id: int, edge_threshold: float = 0.1, surf_threshold: float = 0.1, T_out=None,
                                 enable: bool = True, flags: int = 0):
        """Switch the feature half of mcl_feature_node on for a sweep source (enable=False: off): every accepted sweep then
        also yields the segmented cloud and LeGO-LOAM's sharp / less sharp / flat points.  T_out: publishCloud's
        trans_c2s.inverse() as a [3,4] (or [4,4]) float64 matrix applied to the camera-frame point; identity if None."""
        if not enable:
            self._call("set_lidar_sweep_features", int(source_id), None)
            return
        T = np.hstack([np.eye(3), np.zeros((3, 1))]) if T_out is None else np.asarray(T_out, dtype=np.float64)
        if T.shape not in ((3, 4), (4, 4)):
            raise ValueError("T_out must be [3,4] or [4,4]")
        cfg = K.LidarFeaturesConfig(float(edge_threshold), float(surf_threshold), (C.c_double * 12)(*T[:3].reshape(-1).tolist()), int(flags))
        self._call("set_lidar_sweep_features", int(source_id), C.byref(cfg))

    def get_lidar_sweep_segmented(self, source_id: int, num_vertical_scans: int):
        """ImageProjection's segmented_cloud and seg_msg of the latest sweep: dict of xyz [n,3] float32, range [n] float32,
        col [n] int32, ground [n] uint8, start / end [V] int32 (start_ring_index / end_ring_index)."""
        V = int(num_vertical_scans)
        out = self._get("get_lidar_sweep_segmented", (int(source_id),), ((3,), np.float32), ((), np.float32), ((), np.int32),
                        ((), np.uint8), np.zeros(V, np.int32), np.zeros(V, np.int32))
        return dict(zip(("xyz", "range", "col", "ground", "start", "end"), out))

    def get_lidar_sweep_features(self, source_id: int, which: int):
        """One feature list of the latest sweep (which: 0 sharp, 1 less sharp, 2 flat): ([K,4] float32 x y z ring after T_out,
        [K] uint32 indices into the segmented cloud), in the reference's push order."""
        return tuple(self._get("get_lidar_sweep_features", (int(source_id), int(which)), ((4,), np.float32), ((), np.uint32)))

    def set_depth_frustum(self, source_id: int, fov_w: float, fov_v: float, obstacle_min_range: float, obstacle_max_range: float,
                          T_gbl_sensor):
        """The frustum half of bufferCloud (depth_camera_observation_buffer.cpp:134-174) for this frame of the source:
        FOV in radians, T_gbl_sensor = m2s (x y z qx qy qz qw).  Replaces the source's frustum."""
        cfg = K.DepthFrustumConfig(float(fov_w), float(fov_v), float(obstacle_min_range), float(obstacle_max_range))
        self._call("set_depth_frustum", int(source_id), C.byref(cfg), M.pose(T_gbl_sensor))

    def get_depth_frustum(self, source_id: int):
        """-> (vertices [8,3] TLNear TRNear BLNear BRNear TLFar TRFar BLFar BRFar, normals [6,3] near right bottom left
        far top, planes [6,4], origin [3]), float32, global frame."""
        vtx, nrm = np.zeros((8, 3), np.float32), np.zeros((6, 3), np.float32)
        pl, org = np.zeros((6, 4), np.float32), np.zeros(3, np.float32)
        self._call("get_depth_frustum", int(source_id), M.ptr(vtx), M.ptr(nrm), M.ptr(pl), M.ptr(org))
        return vtx, nrm, pl, org

    def depth_frustum_test(self, points_xyz: np.ndarray):
        """FrustumUtils::isinFrustumsObservations / isAttachFRUSTUMs (frustum_utils.cpp:124-290) for [N, >=3] float32
        points over all depth sources' frustums -> (in_frustums [N] bool, attach [N] bool)."""
        _, p, n, stride = M.cloud(points_xyz, "points")
        inside, attach = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        self._call("depth_frustum_test", p, n, stride, M.ptr(inside), M.ptr(attach))
        return inside[:n].astype(bool), attach[:n].astype(bool)

    def depth_clear_verdicts(self, xy_resolution: float, height_resolution: float, voxels: np.ndarray, offsets: np.ndarray,
                             cluster_xyz: np.ndarray):
        """The decision tree of DepthCameraLayer::selfClear (depth_camera_layer.cpp:324-422) for the markings
        voxels [M,3] int32 with stored clusters cluster_xyz[offsets[i]:offsets[i+1]] ([T,3] float32), against the depth
        sources' current observation -> (verdict [M] uint8: bit 0 kept, bits 1-2 branch; engaged [M] uint32)."""
        vox = np.ascontiguousarray(voxels, dtype=np.int32).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        pts = np.ascontiguousarray(cluster_xyz, dtype=np.float32).reshape(-1, 3)
        m = vox.shape[0]
        if off.shape[0] != m + 1 or (m and int(off[-1]) != pts.shape[0]):
            raise ValueError("offsets must be [M + 1] and end at the number of cluster points")
        verdict, engaged = np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.uint32)
        self._call("depth_clear_verdicts", float(xy_resolution), float(height_resolution), M.ptr(vox), M.ptr(off), M.ptr(pts), m,
                   M.ptr(verdict), M.ptr(engaged))
        return verdict[:m], engaged[:m]

    def depth_clear_launches(self) -> int:
        """Device operations (kernels, memsets, copies) the last depth_clear_verdicts call enqueued."""
        n = C.c_uint32(0)
        self._call("depth_clear_launches", C.byref(n))
        return int(n.value)

    def _create_on_maps(self, name: str, cfg, ground_xyz, map_xyz):
        """The layers' create calls: the configuration, then pcl_ground_ and pcl_map_ as clouds -> the ground array."""
        g, gp, gn, gs = M.cloud(ground_xyz, "ground")
        _, mp, mn, ms = M.cloud(map_xyz, "map")
        self._call(name, C.byref(cfg), gp, gn, gs, mp, mn, ms)
        return g

    def depth_mark_create(self, xy_resolution: float, height_resolution: float, ground_xyz: np.ndarray, map_xyz: np.ndarray,
                          tolerance: float = 0.1, min_cluster_size: int = 1, segmentation_ignore_ratio: float = 0.2,
                          max_observation_points: int = 1 << 16):
        """The depth camera layer's selfMark state: pcl_ground_ / pcl_map_ ([N, >=3] float32, the map may be empty) go to
        the device once.  Independent of the lidar marking layer; calling it again replaces the state."""
        cfg = K.DepthMarkConfig(float(xy_resolution), float(height_resolution), float(tolerance), int(min_cluster_size), 0,
                                float(segmentation_ignore_ratio), int(max_observation_points), 0)
        self._create_on_maps("depth_mark_create", cfg, ground_xyz, map_xyz)

    def depth_mark_clusters(self, T_gbl_base):
        """One DepthCameraLayer::selfMark (depth_camera_layer.cpp:487-601) on the depth sources' current observation ->
        (centroids [C,3] float32, voxels [C,3] int32, sizes [C] uint32, offsets [C+1] uint32, points [P,3] float32,
        plane [4] float32, stats): what addPCPtr is to be called with, in the reference's order.  The buffers are sized
        by a count-only call first."""
        tgb = M.pose(T_gbl_base)
        st = K.DepthMarkStats()
        self._call("depth_mark_clusters", tgb, 0, 0, None, None, None, None, None, None, C.byref(st))
        c, p = int(st.n_accepted), int(st.n_points)
        cen, vox = np.zeros((max(c, 1), 3), np.float32), np.zeros((max(c, 1), 3), np.int32)
        size, off = np.zeros(max(c, 1), np.uint32), np.zeros(c + 1, np.uint32)
        pts, plane = np.zeros((max(p, 1), 3), np.float32), np.zeros(4, np.float32)
        self._call("depth_mark_clusters", tgb, c, p, M.ptr(cen), M.ptr(vox), M.ptr(size), M.ptr(off), M.ptr(pts), M.ptr(plane),
                   C.byref(st))
        return cen[:c], vox[:c], size[:c], off, pts[:p], plane, st

    def depth_layer_create(self, cfg: "K.DepthLayerConfig", ground_xyz: np.ndarray, map_xyz: np.ndarray):
        """The depth camera layer's device state (store, dGraph, lethal set): pcl_ground_ / pcl_map_ ([N, >=3] float32, the
        map may be empty) go to the device once.  See dddmr_navigation_amd.depth_layer.DepthLayer."""
        self._create_on_maps("depth_layer_create", cfg, ground_xyz, map_xyz)

    def depth_layer_update(self, T_gbl_base) -> "K.DepthLayerStats":
        """One selfClear + selfMark pass of the depth camera layer on the depth sources' current observation."""
        st = K.DepthLayerStats()
        self._call("depth_layer_update", M.pose(T_gbl_base), C.byref(st))
        return st

    def depth_layer_reset(self):
        self._call("depth_layer_reset")

    def depth_layer_voxels(self) -> np.ndarray:
        return self._get("depth_layer_get_voxels", (), ((3,), np.int32))[0]

    def depth_layer_clusters(self):
        """The alive markings with their stored pc_ -> (voxels [M,3] int32, offsets [M+1] uint32, points [P,3] float32)."""
        m, p = C.c_size_t(0), C.c_size_t(0)
        self._call("depth_layer_get_clusters", None, None, None, 0, 0, C.byref(m), C.byref(p))
        vox, off = np.zeros((max(m.value, 1), 3), np.int32), np.zeros(m.value + 1, np.uint32)
        pts = np.zeros((max(p.value, 1), 3), np.float32)
        self._call("depth_layer_get_clusters", M.ptr(vox), M.ptr(off), M.ptr(pts), m.value, p.value, C.byref(m), C.byref(p))
        return vox[: m.value], off, pts[: p.value]

    def depth_layer_dgraph(self, n_ground: int) -> np.ndarray:
        return self._fixed("depth_layer_get_dgraph", int(n_ground) + 1, np.float64)

    def depth_layer_lethal(self, n_ground: int) -> np.ndarray:
        return self._fixed("depth_layer_get_lethal", int(n_ground) + 1, np.uint8, as_bool=True)

    def set_stitcher(self, stitcher_num: int):
        """cbSensor's `stitcher_num` (multilayer_spinning_lidar.cpp:185-200): feed the last N raw scans together."""
        self._call("set_stitcher", int(stitcher_num))

    def get_cloud(self) -> np.ndarray:
        return self._get("get_cloud", (), ((4,), np.float32))[0]

    def setPlan(self, prune_plan: np.ndarray):
        """Prune plan poses [M,7] (x y z qx qy qz qw), the output of
        Local_Planner::prunePlan (local_planner.cpp:374-445)."""
        plan = np.ascontiguousarray(prune_plan, dtype=np.float64).reshape(-1, 7)
        self._check(self._lib.dddmr_rollout_set_prune_plan(self._ctx, plan.ctypes.data_as(C.c_void_p), plan.shape[0]))

    set_prune_plan = setPlan

    def path_blocked(self, pcl_prune_plan: np.ndarray, check_radius: float):
        """PathBlockedStrategy::selfMark (path_blocked_strategy.cpp:56-100) on the current
        aggregate observation.  pcl_prune_plan: [M,4] x y z intensity as prunePlan fills it
        (host_logic.prune_plan_cloud).  -> (blocked ratio in percent, opinion, flags[M])"""
        plan = np.ascontiguousarray(pcl_prune_plan, dtype=np.float32).reshape(-1, 4)
        flags = np.zeros(max(len(plan), 1), dtype=np.uint8)
        ratio, op = C.c_double(0.0), C.c_int32(0)
        self._call("path_blocked", M.ptr(plan), len(plan), float(check_radius), C.byref(ratio), C.byref(op), M.ptr(flags))
        return ratio.value, op.value, flags[: len(plan)].astype(bool)

    def samples(self, traj_gen_name: str, tick_in: K.TickInput) -> np.ndarray:
        """The theory's initialise(): the sample list a tick would roll out, [N,3] vx vy wz (host-only)."""
        return self._get("samples", (traj_gen_name.encode(), C.byref(tick_in)), ((3,), np.float32))[0]

    # -- the tick ----------------------------------------------------------
    def tick(self, traj_gen_name: str, tick_in: K.TickInput) -> K.RolloutResult:
        res = K.RolloutResult()
        self._check(self._lib.dddmr_rollout_tick(self._ctx, traj_gen_name.encode(), C.byref(tick_in), C.byref(res)))
        self.last_result = res
        return res

    def tick_begin(self, traj_gen_name: str, tick_in: K.TickInput) -> None:
        """Enqueue a tick and return at once (pair with tick_end)."""
        self._check(self._lib.dddmr_rollout_tick_begin(self._ctx, traj_gen_name.encode(), C.byref(tick_in)))

    def tick_end(self) -> K.RolloutResult:
        res = K.RolloutResult()
        self._check(self._lib.dddmr_rollout_tick_end(self._ctx, C.byref(res)))
        self.last_result = res
        return res

    def computeVelocityCommand(self, traj_gen_name: str, best_traj: Trajectory, tick_in: K.TickInput) -> PlannerState:
        """Local_Planner::computeVelocityCommand (local_planner.cpp:482-621), the
        section :535-587; fills best_traj like the reference does."""
        res = self.tick(traj_gen_name, tick_in)
        best_traj.xv_, best_traj.yv_, best_traj.thetav_ = res.vx, res.vy, res.wz
        best_traj.cost_ = res.best_cost
        best_traj.index = res.best_index
        return PlannerState(res.planner_state)

    def resolve(self, reduced_key: int) -> K.RolloutResult:
        res = K.RolloutResult()
        if self.last_result is not None:
            C.memmove(C.byref(res), C.byref(self.last_result), C.sizeof(res))
        self._call("resolve", C.c_int64(reduced_key), C.byref(res))
        return res

    def winner_words(self, res: Optional[K.RolloutResult] = None):
        """This rank's two int64 words of the exact multi-rank argmin (cost bits, -index)."""
        res = res if res is not None else self.last_result
        w = (C.c_int64 * 2)()
        self._lib.dddmr_rollout_winner_words(C.byref(res), w)
        return int(w[0]), int(w[1])

    def resolve_words(self, words) -> K.RolloutResult:
        """Resolve the global winner from the min-all-reduced slot vector [2 * n_ranks] int64."""
        words = [int(v) for v in words]
        arr = (C.c_int64 * len(words))(*words)
        res = K.RolloutResult()
        if self.last_result is not None:
            C.memmove(C.byref(res), C.byref(self.last_result), C.sizeof(res))
        self._check(self._lib.dddmr_rollout_resolve_words(self._ctx, arr, len(words) // 2, C.byref(res)))
        return res

    # -- in-library RCCL exchange (multi-rank contexts) ------------------------
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * K.COMM_ID_BYTES)()
        rc = self._lib.dddmr_rollout_comm_unique_id(buf)
        if rc != K.OK:
            raise RolloutError(rc, "dddmr_rollout_comm_unique_id failed (librccl not loadable?)")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, n_ranks: int):
        if len(unique_id) != K.COMM_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        self._call("comm_init", (C.c_uint8 * K.COMM_ID_BYTES)(*unique_id), rank, n_ranks)

    def comm_destroy(self):
        self._call("comm_destroy")

    def comm_ranks(self) -> int:
        """Ranks the context's communicator reports (ncclCommCount); 0 without one."""
        n = C.c_int32(0)
        self._call("comm_ranks", C.byref(n))
        return int(n.value)

    def comm_loopback(self):
        """Single-device rehearsal of the exchange: see dddmr_rollout_comm_loopback."""
        self._call("comm_loopback")

    def comm_loopback_set_peer(self, peer_rank: int, words):
        self._call("comm_loopback_set_peer", int(peer_rank), (C.c_int64 * 2)(int(words[0]), int(words[1])))

    def stream_ceiling(self, nbytes: int = 1 << 30, reps: int = 10):
        """Measured stream ceilings of this GPU -> (copy GB/s counting read + write, read-only GB/s)."""
        cp, rd = C.c_double(0.0), C.c_double(0.0)
        self._call("stream_ceiling", nbytes, reps, C.byref(cp), C.byref(rd))
        return cp.value, rd.value

    def selftest_sincos(self, angles):
        """sin / cos of heading angles from the rollout's own double routine -> (sin[n], cos[n]) f64"""
        a = np.ascontiguousarray(angles, dtype=np.float64)
        sn, cs = np.empty_like(a), np.empty_like(a)
        self._call("selftest_sincos", M.ptr(a), a.size, M.ptr(sn), M.ptr(cs))
        return sn, cs

    def selftest_wave_ops(self, values, flags, append_base: int = 0):
        """The wave primitives of csrc/wave_ops.hip.h over n <= 256 values (u32) and flags, one per lane of one workgroup
        -> (out32[10, 256] u32, out64[2, 256] u64), rows as include/dddmr_rollout.h lists them"""
        v = np.ascontiguousarray(values, dtype=np.uint32)
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        out32, out64 = np.zeros((10, 256), dtype=np.uint32), np.zeros((2, 256), dtype=np.uint64)
        self._call("selftest_wave_ops", M.ptr(v), M.ptr(f), v.size, int(append_base), M.ptr(out32), M.ptr(out64))
        return out32, out64

    def selftest_wave_wide(self, values, lanes, n_groups: int):
        """What selftest_wave_ops does not reach: block_excl_scan<16> and wave_last over n <= 1024 values (u32), the float
        and int reductions over the 64 words of `lanes`, last_block among n_groups workgroups
        -> (scan[2, 1024], reduce[4, 64], misc[4]) u32, rows as include/dddmr_rollout.h lists them"""
        v = np.ascontiguousarray(values, dtype=np.uint32)
        l = np.ascontiguousarray(lanes, dtype=np.uint32)
        if l.size != 64:
            raise ValueError("lanes: one word per lane of a wave, 64")
        scan, red, misc = np.zeros((2, 1024), np.uint32), np.zeros((4, 64), np.uint32), np.zeros(4, np.uint32)
        self._call("selftest_wave_wide", M.ptr(v), v.size, M.ptr(l), int(n_groups), M.ptr(scan), M.ptr(red), M.ptr(misc))
        return scan, red, misc

    def selftest_point_grid(self, points, lo, hi, cell_xy, cell_z, cap_cells: int, queries, r_box, r2, stop_at: int = 0x7fffffff):
        """The point grid of csrc/point_grid.hip.h built over `points` [n, 3] in the box lo .. hi and walked for `queries`
        [m, 3] -> dict of the grid (nx, ny, nz, and as float32 ox, oy, oz, inv_xy, inv_z), cell_start [cells + 1] u32,
        sorted [n, 4] u32 (bits of x y z, original index), thread [m, 8] u32 and wave [m, 5] u32, columns as
        include/dddmr_rollout.h lists them.  r_box and r2 go to the library as the float32 they round to."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)
        box_lo, box_hi = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(hi, dtype=np.float32)
        if box_lo.size != 3 or box_hi.size != 3:
            raise ValueError("lo and hi: three coordinates each")
        cell = np.array([cell_xy, cell_z], dtype=np.float32)
        radius = np.array([r_box, r2], dtype=np.float32)
        grid = np.zeros(8, np.uint32)
        cell_start = np.zeros(max(int(cap_cells), 0) + 1, np.uint32)
        srt, thr, wav = np.zeros((len(p), 4), np.uint32), np.zeros((len(q), 8), np.uint32), np.zeros((len(q), 5), np.uint32)
        opt = lambda a: M.ptr(a) if a.size else None
        self._call("selftest_point_grid", opt(p), len(p), M.ptr(box_lo), M.ptr(box_hi), M.ptr(cell), int(cap_cells), opt(q), len(q),
                   M.ptr(radius), int(stop_at), M.ptr(grid), M.ptr(cell_start), opt(srt), opt(thr), opt(wav))
        nx, ny, nz = (int(x) for x in grid[:3])
        geom = grid[3:].view(np.float32)
        return dict(nx=nx, ny=ny, nz=nz, ox=geom[0], oy=geom[1], oz=geom[2], inv_xy=geom[3], inv_z=geom[4],
                    cell_start=cell_start[: nx * ny * nz + 1], sorted=srt, thread=thr, wave=wav)

    # -- per-trajectory outputs of the last tick -----------------------------
    def debug(self):
        """-> (costs[n_local] f64, steps[n_local] i32, samples[n_local,3] f32)"""
        n = int(self.last_result.n_local) if self.last_result is not None else 0
        costs = np.zeros(max(n, 1), dtype=np.float64)
        steps = np.zeros(max(n, 1), dtype=np.int32)
        smp = np.zeros((max(n, 1), 3), dtype=np.float32)
        dbg = K.RolloutDebug()
        dbg.costs = costs.ctypes.data_as(C.POINTER(C.c_double))
        dbg.steps = steps.ctypes.data_as(C.POINTER(C.c_int32))
        dbg.samples = smp.ctypes.data_as(C.POINTER(C.c_float))
        self._call("get_debug", C.byref(dbg))
        return costs[:n], steps[:n], smp[:n]

    def pose_arrays(self, accepted_only: bool = False) -> np.ndarray:
        """The `trajectory` / `accepted_trajectory` debug pose arrays of the last tick, [n,7]."""
        return self._get("get_pose_arrays", (1 if accepted_only else 0,), ((7,), np.float64))[0]

    def heading_rows(self) -> int:
        """1 if the last launched tick shared one row of headings per angular sample, 0 if every trajectory ran its
        own chain, -1 before any tick (dddmr_rollout_heading_rows)."""
        return int(self._rc("heading_rows"))

    def fused_walk(self) -> int:
        """1 if the last launched tick walked the prune plan as the tail of the collision walk, 0 if the path critics' search
        ran as a phase of its own, -1 before any tick (dddmr_rollout_fused_walk)."""
        return int(self._rc("fused_walk"))

    def best_poses(self) -> np.ndarray:
        return self._get("get_best_poses", (), ((7,), np.float64))[0]

    def best_cuboids(self) -> np.ndarray:
        """Cuboid vertices carried along the best trajectory, [n_poses, 8, 3] float32."""
        return self._get("get_best_cuboids", (), ((8, 3), np.float32))[0]
