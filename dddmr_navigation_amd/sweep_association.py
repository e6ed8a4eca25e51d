"""Host-side mirror of the lidar sweep association on top of the C-ABI (dddmr_rollout_*_lidar_sweep_association and
its getters): the rest of the front half of LeGO-LOAM's feature node on a sweep source whose features are on -- the
sweep's start / end orientation (ImageProjection::findStartEndAngle), the point times of adjustDistortion, the less-flat
cloud with its VoxelGrid, the outlier cloud, and the four clouds as the host FeatureAssociation and mapOptimization take
them.  All compute and all state live in the HIP library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _marshal as M

SHARP, LESS_SHARP, FLAT, LESS_FLAT = 0, 1, 2, 3
FRAME_ASSOCIATION, FRAME_T_OUT = 0, 1


class SweepAssociation:
    """The association of sweep source `source_id` of LocalPlanner `lp` (its features must be on): switched on here,
    it holds from the next sweep; close() switches it off, as do switching the features off and re-configuring the source."""

    def __init__(self, lp, source_id: int, scan_period: float = 0.1):
        self._lp = lp
        self.source_id = int(source_id)
        self.scan_period = float(scan_period)
        lp._call("set_lidar_sweep_association", self.source_id, 1, self.scan_period)
        self._open = True

    def orientation(self):
        """(start_orientation, end_orientation, orientation_diff as float32, the index at which halfPassed flips or the
        number of segmented points when it never does) of the latest accepted sweep."""
        out = np.zeros(3, np.float32)
        half = C.c_int32(0)
        self._lp._call("get_lidar_sweep_orientation", self.source_id, M.ptr(out), C.byref(half))
        return out[0], out[1], out[2], int(half.value)

    def times(self) -> np.ndarray:
        """[n] float32: ring + scan_period * relTime of every segmented point, in segment-index order."""
        return self._lp._get("get_lidar_sweep_times", (self.source_id,), ((), np.float32))[0]

    def cloud(self, which: int, frame: int = FRAME_ASSOCIATION):
        """One of the four clouds (which: 0 sharp, 1 less sharp, 2 flat, 3 less flat) in the association frame (frame 0:
        (y, z, x) of the segmented point) or through the features' T_out (frame 1): ([K,4] float32 x y z intensity,
        [K] uint32 segment indices; for less flat the lowest index that went into the voxel)."""
        return tuple(self._lp._get("get_lidar_sweep_association", (self.source_id, int(which), int(frame)), ((4,), np.float32), ((), np.uint32)))

    def outliers(self) -> np.ndarray:
        """[K,4] float32: the outlier cloud, pitch-removed x y z and row + col / 10000, in raster order."""
        return self._lp._get("get_lidar_sweep_outliers", (self.source_id,), ((4,), np.float32))[0]

    def close(self):
        if self._open:
            self._open = False
            self._lp._call("set_lidar_sweep_association", self.source_id, 0, 0.0)
