"""Host-side mirror of the localiser's device half on top of the C-ABI (dddmr_rollout_mcl_*):
mcl_3dl's LidarMeasurementModelLikelihood::measure for a batch of particles
(dddmr_mcl_3dl/src/lidar_measurement_model_likelihood.cpp:86-252, src/mcl_3dl.cpp:466-503) and the preparation of its
observation, MCL3dlNode::cbLeGoFeatureCloud (src/mcl_3dl.cpp:263-464).
All compute and all state live in the HIP library; the filter itself (prediction, bias, resampling) stays on the host."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K


def shipped_config(**kw) -> K.MclConfig:
    """The likelihood block of the shipped mcl_3dl.yaml, with capacities for its 60 particles many times over."""
    c = K.MclConfig()
    d = dict(match_dist_min=0.3, match_dist_flat=0.05, radius_of_ground_search=1.0, threshold_for_trusted_ground=6,
             max_map_points=1 << 20, max_ground_points=1 << 20, max_particles=1 << 14, max_observation_points=2000,
             max_ground_neighbours=1024)
    d.update(kw)
    for k, v in d.items():
        if not hasattr(c, k) or k.startswith("reserved"):
            raise KeyError(k)
        setattr(c, k, v)
    return c


def shipped_observation_config(**kw) -> K.MclObservationConfig:
    """cbLeGoFeatureCloud's parameters as p2p_move_base_localization.yaml ships them, with room for a 16-ring sweep's lists."""
    c = K.MclObservationConfig()
    d = dict(euc_cluster_distance=0.8, euc_cluster_min_size=3, max_flat_points=400, max_less_sharp_points=1600)
    d.update(kw)
    for k, v in d.items():
        if not hasattr(c, k) or k == "reserved":
            raise KeyError(k)
        setattr(c, k, v)
    return c


def _transform(T_b2s):
    t = np.ascontiguousarray(T_b2s, dtype=np.float64)
    if t.shape == (4, 4):
        t = np.ascontiguousarray(t[:3])
    if t.shape != (3, 4):
        raise ValueError("T_b2s: 3x4 (or 4x4) row-major")
    return t


def _cloud(a, cols):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size == 0:
        a = a.reshape(0, cols)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"expected [N, {cols}] float32")
    return a


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a.shape[0] else None


class ParticleMeasure:
    """The measurement model of one LocalPlanner context."""

    def __init__(self, lp, cfg: K.MclConfig):
        self._lp = lp
        self.cfg = cfg
        lp._check(lp._lib.dddmr_rollout_mcl_create(lp._ctx, C.byref(cfg)))
        self.last = None

    def set_map(self, map_xyz, ground_xyz, ground_normals):
        """SubMaps::swapKdTree: the sub-map cloud [M,3], the ground cloud [G,3] and one normal per ground point [G,3].
        A refused call leaves the current map in place."""
        m, g, n = _cloud(map_xyz, 3), _cloud(ground_xyz, 3), _cloud(ground_normals, 3)
        if len(g) != len(n):
            raise ValueError("one normal per ground point")
        lp = self._lp
        lp._check(lp._lib.dddmr_rollout_mcl_set_map(lp._ctx, _p(m), len(m), 12, _p(g), _p(n), len(g), 12, 12))

    def measure(self, flat_xyz, less_sharp_xyzi, states):
        """flat [A,3], less sharp [B,4] (x y z intensity), states [N,7] (pos xyz, rot xyzw, raw) ->
        (likelihood [N], quality [N]) float32; self.last holds the call's MclStats."""
        f, l, s = _cloud(flat_xyz, 3), _cloud(less_sharp_xyzi, 4), _cloud(states, 7)
        like, qual = np.zeros(max(len(s), 1), np.float32), np.zeros(max(len(s), 1), np.float32)
        st = K.MclStats()
        lp = self._lp
        rc = lp._lib.dddmr_rollout_mcl_measure(lp._ctx, _p(f), len(f), _p(l), len(l), _p(s), len(s), like.ctypes.data_as(C.c_void_p),
                                               qual.ctypes.data_as(C.c_void_p), C.byref(st))
        self.last = st
        lp._check(rc)
        return like[: len(s)], qual[: len(s)]

    def terms(self, n: int) -> dict:
        """The parts of the last measure for its n particles: score, pos_weight, n_match, n_ground, healthy."""
        n = int(n)
        out = dict(score=np.zeros(max(n, 1), np.float32), pos_weight=np.zeros(max(n, 1), np.float32),
                   n_match=np.zeros(max(n, 1), np.uint32), n_ground=np.zeros(max(n, 1), np.uint32), healthy=np.zeros(max(n, 1), np.uint8))
        lp = self._lp
        lp._check(lp._lib.dddmr_rollout_mcl_get_terms(lp._ctx, *(out[k].ctypes.data_as(C.c_void_p) for k in
                                                                 ("score", "pos_weight", "n_match", "n_ground", "healthy")), n))
        out = {k: v[:n] for k, v in out.items()}
        out["healthy"] = out["healthy"].astype(bool)
        return out

    # ---- the observation: cbLeGoFeatureCloud on the device -------------------------------------------------------------
    def configure_observation(self, cfg):
        """cfg: a K.MclObservationConfig (shipped_observation_config()), or None to switch the observation off."""
        lp = self._lp
        lp._check(lp._lib.dddmr_rollout_mcl_set_observation_config(lp._ctx, C.byref(cfg) if cfg is not None else None))
        self.obs_cfg = cfg
        self._n_normals = 0          # (a new configuration forgets the prepared observation)
        self.last_observation = None

    def prepare(self, flat_xyz, less_sharp_xyz, T_b2s):
        """The sweep's flat [A,3+] and less-sharp [B,3+] lists (only x y z are read) and trans_b2s_af3 (3x4 row-major) ->
        the call's MclObservationStats, also kept in self.last_observation.  The prepared clouds stay on the device."""
        f, l = np.ascontiguousarray(flat_xyz, dtype=np.float32), np.ascontiguousarray(less_sharp_xyz, dtype=np.float32)
        f = f.reshape(0, 3) if f.size == 0 else f
        l = l.reshape(0, 3) if l.size == 0 else l
        if f.ndim != 2 or l.ndim != 2 or f.shape[1] < 3 or l.shape[1] < 3:
            raise ValueError("expected [N, >=3] float32")
        t = _transform(T_b2s)
        st = K.MclObservationStats()
        lp = self._lp
        rc = lp._lib.dddmr_rollout_mcl_prepare(lp._ctx, _p(f), len(f), f.strides[0], _p(l), len(l), l.strides[0],
                                               t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        self.last_observation = st
        lp._check(rc)
        self._n_normals = st.n_less_sharp_in
        return st

    def prepare_from_sweep(self, source_id, T_b2s):
        """The same on the current features of a sweep source (set_lidar_sweep with features on), read where they lie."""
        t = _transform(T_b2s)
        st = K.MclObservationStats()
        lp = self._lp
        rc = lp._lib.dddmr_rollout_mcl_prepare_from_sweep(lp._ctx, int(source_id), t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        self.last_observation = st
        lp._check(rc)
        self._n_normals = st.n_less_sharp_in
        return st

    def observation(self):
        """-> (flat [A,3], less sharp [B,4] x y z intensity, normals [B_in,3] in input order) of the prepared observation."""
        lp = self._lp
        nf, nl = C.c_size_t(0), C.c_size_t(0)
        lp._check(lp._lib.dddmr_rollout_mcl_get_observation(lp._ctx, None, 0, C.byref(nf), None, 0, C.byref(nl), None, 0))
        cap = max(int(self.obs_cfg.max_less_sharp_points), 1)
        f, l = np.zeros((max(nf.value, 1), 3), np.float32), np.zeros((max(nl.value, 1), 4), np.float32)
        n = np.zeros((cap, 3), np.float32)
        lp._check(lp._lib.dddmr_rollout_mcl_get_observation(lp._ctx, f.ctypes.data_as(C.c_void_p), len(f), C.byref(nf),
                                                            l.ctypes.data_as(C.c_void_p), len(l), C.byref(nl),
                                                            n.ctypes.data_as(C.c_void_p), cap))
        return f[: nf.value], l[: nl.value], n[: self._n_normals]

    def measure_prepared(self, states):
        """measure() on the prepared observation where it lies -> (likelihood [N], quality [N]); self.last as for measure."""
        s = _cloud(states, 7)
        like, qual = np.zeros(max(len(s), 1), np.float32), np.zeros(max(len(s), 1), np.float32)
        st = K.MclStats()
        lp = self._lp
        rc = lp._lib.dddmr_rollout_mcl_measure_prepared(lp._ctx, _p(s), len(s), like.ctypes.data_as(C.c_void_p),
                                                        qual.ctypes.data_as(C.c_void_p), C.byref(st))
        self.last = st
        lp._check(rc)
        return like[: len(s)], qual[: len(s)]

    def close(self):
        pass      # the context owns the device state
