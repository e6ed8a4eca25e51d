"""Host-side mirror of the localiser's sub-maps on top of the C-ABI (dddmr_rollout_submap_*): mcl_3dl's SubMaps
(dddmr_mcl_3dl/src/sub_maps.cpp) -- the keyframes of the pose graph kept in device memory, the radius search over their
poses, the warm-up (concatenation, the two grids, NormalEstimation with setKSearch(20) over the ground) and the swap.
All compute and all state live in the HIP library; a warm-up hands it a list of keyframe ids and nothing else."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import _marshal as M


def shipped_config(**kw) -> K.SubmapConfig:
    """NormalEstimation's setKSearch(20) of sub_maps.cpp:246-252, with room for a few hundred keyframes."""
    return M.struct_from(K.SubmapConfig, dict(max_keyframes=1024, max_store_map_points=1 << 22, max_store_ground_points=1 << 21, normal_k=20), kw)


class SubMaps:
    """The keyframe store and the warm-up generation of one ParticleMeasure (which must exist first: the warm-up is
    bounded by its max_map_points / max_ground_points, and a new ParticleMeasure on the context drops the store)."""

    def __init__(self, lp, particle_measure, cfg: K.SubmapConfig):
        self._lp = lp
        self.pm = particle_measure
        self.cfg = cfg
        lp._call("submap_create", C.byref(cfg))
        self.last = None

    def add_keyframe(self, corner_xyz, ground_xyz, position, T_map_base=None) -> int:
        """One keyframe of the pose graph: its corner [A,3+] and ground [B,3+] clouds (only x y z are read), its pose's
        position, and the 3x4 row-major transform into the map frame (None: the clouds are there already) -> its id."""
        _, cp, cn, cs = M.cloud(corner_xyz, "corner")
        _, gp, gn, gs = M.cloud(ground_xyz, "ground")
        tp = M.transform(T_map_base)[1] if T_map_base is not None else None
        pos = (C.c_double * 3)(*[float(v) for v in position])
        kid = C.c_int32(-1)
        self._lp._call("submap_add_keyframe", cp, cn, cs, gp, gn, gs, tp, pos, C.byref(kid))
        return kid.value

    def select(self, position, radius) -> np.ndarray:
        """The keyframes within `radius` of `position` -> their ids, ascending (int32)."""
        pos = (C.c_double * 3)(*[float(v) for v in position])
        return self._lp._get("submap_select", (pos, float(radius)), ((), np.int32))[0]

    def warm_up(self, ids) -> K.SubmapStats:
        """The listed keyframes become the warm-up generation (their order is the concatenation's) -> the call's
        SubmapStats, also kept in self.last before an error raises."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        st = K.SubmapStats()
        rc = self._lp._rc("submap_warm_up", M.ptr(a) if a.size else None, a.size, C.byref(st))
        self.last = st
        self._lp._check(rc)
        return st

    def swap(self):
        """SubMaps::swapKdTree: the warm-up generation answers the measures from now on."""
        self._lp._call("submap_swap")

    def get(self, which: int = 0) -> dict:
        """which 0: the current generation, 1: the warm-up -> map [M,3], ground [G,3], normals [G,3] float32 and
        neighbours [G,normal_k] int32 (-1 padded; all -1 for a generation that set_map made)."""
        nm, ng = C.c_size_t(0), C.c_size_t(0)
        self._lp._call("submap_get", int(which), None, 0, C.byref(nm), None, None, None, 0, C.byref(ng))
        k = int(self.cfg.normal_k)
        m = np.zeros((max(nm.value, 1), 3), np.float32)
        g, n = np.zeros((max(ng.value, 1), 3), np.float32), np.zeros((max(ng.value, 1), 3), np.float32)
        nb = np.full((max(ng.value, 1), k), -1, np.int32)
        self._lp._call("submap_get", int(which), M.ptr(m), len(m), C.byref(nm), M.ptr(g), M.ptr(n), M.ptr(nb), len(g), C.byref(ng))
        return dict(map=m[: nm.value], ground=g[: ng.value], normals=n[: ng.value], neighbours=nb[: ng.value])

    def close(self):
        pass      # the context owns the device state
