"""Host-side mirror of the global-mode depth camera layer on top of the C-ABI (dddmr_rollout_depth_layer_*):
DepthCameraLayer::selfClear / selfMark with its Marking store, dGraph and lethal set
(dddmr_perception_3d/plugins/depth_camera/depth_camera_layer.cpp:252-601, plugins/cluster_marking.cpp:49-138).
All compute and all state live in the HIP library; the depth sources are fed through the LocalPlanner."""
from __future__ import annotations

import numpy as np

from . import _capi as K
from . import _marshal as M


def shipped_config(**kw) -> K.DepthLayerConfig:
    """The depth camera block of the shipped perception_3d_global configuration, the plugin's defaults elsewhere."""
    return M.struct_from(K.DepthLayerConfig, dict(
        xy_resolution=0.05, height_resolution=0.05, marking_height=2.0, perception_window_size=5.0,
        euclidean_cluster_extraction_tolerance=0.1, euclidean_cluster_extraction_min_cluster_size=1,
        segmentation_ignore_ratio=0.2, inscribed_radius=0.5, inflation_radius=1.5, max_obstacle_distance=9999.0,
        max_observation_points=1 << 16, max_markings=1 << 15, max_cluster_points=1 << 20), kw)


class DepthLayer:
    """The depth camera layer of one LocalPlanner context.  `ground` = pcl_ground_ (dGraph nodes), `static_map` = pcl_map_,
    both [N, >=3] float32."""

    def __init__(self, lp, cfg: K.DepthLayerConfig, ground: np.ndarray, static_map: np.ndarray):
        self._lp = lp
        self.cfg = cfg
        self.ground = np.ascontiguousarray(ground, dtype=np.float32)
        self.n_ground = len(self.ground)
        lp.depth_layer_create(cfg, self.ground, static_map)
        self.last = None
        self.totals = dict(updates=0, clusters=0, accepted=0, cleared=0, contested=0, gc_runs=0, host_waits=0)

    def update(self, T_gbl_base) -> K.DepthLayerStats:
        """One doClear_then_Mark pass on the depth sources' current observation."""
        st = self._lp.depth_layer_update(T_gbl_base)
        self.last = st
        t = self.totals
        t["updates"] += 1; t["clusters"] += st.n_clusters; t["accepted"] += st.n_accepted; t["cleared"] += st.n_cleared
        t["contested"] += st.n_contested; t["gc_runs"] += st.gc_runs; t["host_waits"] += st.host_waits
        return st

    def reset(self):
        self._lp.depth_layer_reset()

    def voxels(self) -> np.ndarray:
        return self._lp.depth_layer_voxels()

    def clusters(self):
        """-> (voxels [M,3] int32, offsets [M+1] uint32, points [P,3] float32): the alive markings' stored pc_"""
        return self._lp.depth_layer_clusters()

    def dgraph(self) -> np.ndarray:
        return self._lp.depth_layer_dgraph(self.n_ground)

    def lethal(self) -> np.ndarray:
        return self._lp.depth_layer_lethal(self.n_ground)

    def lethal_points(self) -> np.ndarray:
        """updateLethalPointCloud: the ground points whose lethal flag is set"""
        return self.ground[self.lethal()[: self.n_ground], :3]

    def summary(self) -> dict:
        t = self.totals
        n = max(t["updates"], 1)
        return {"updates": t["updates"], "clusters_per_update": round(t["clusters"] / n, 1),
                "accepted_per_update": round(t["accepted"] / n, 1), "cleared_per_update": round(t["cleared"] / n, 1),
                "contested": t["contested"], "gc_runs": t["gc_runs"], "host_waits_per_update": round(t["host_waits"] / n, 2),
                "alive_markings": int(self.last.n_alive) if self.last is not None else 0}

    def close(self):
        pass      # the context owns the device state
