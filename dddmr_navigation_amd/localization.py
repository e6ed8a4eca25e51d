"""Host-side mirror of the localiser's device half on top of the C-ABI (dddmr_rollout_mcl_*):
mcl_3dl's LidarMeasurementModelLikelihood::measure for a batch of particles
(dddmr_mcl_3dl/src/lidar_measurement_model_likelihood.cpp:86-252, src/mcl_3dl.cpp:466-503) and the preparation of its
observation, MCL3dlNode::cbLeGoFeatureCloud (src/mcl_3dl.cpp:263-464).
All compute and all state live in the HIP library; the filter itself (prediction, bias, resampling) stays on the host."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import _marshal as M


def shipped_config(**kw) -> K.MclConfig:
    """The likelihood block of the shipped mcl_3dl.yaml, with capacities for its 60 particles many times over."""
    return M.struct_from(K.MclConfig, dict(
        match_dist_min=0.3, match_dist_flat=0.05, radius_of_ground_search=1.0, threshold_for_trusted_ground=6,
        max_map_points=1 << 20, max_ground_points=1 << 20, max_particles=1 << 14, max_observation_points=2000,
        max_ground_neighbours=1024), kw)


def shipped_observation_config(**kw) -> K.MclObservationConfig:
    """cbLeGoFeatureCloud's parameters as p2p_move_base_localization.yaml ships them, with room for a 16-ring sweep's lists."""
    return M.struct_from(K.MclObservationConfig, dict(
        euc_cluster_distance=0.8, euc_cluster_min_size=3, max_flat_points=400, max_less_sharp_points=1600), kw)


class ParticleMeasure:
    """The measurement model of one LocalPlanner context."""

    def __init__(self, lp, cfg: K.MclConfig):
        self._lp = lp
        self.cfg = cfg
        lp._call("mcl_create", C.byref(cfg))
        self.last = None

    def set_map(self, map_xyz, ground_xyz, ground_normals):
        """SubMaps::swapKdTree: the sub-map cloud [M,3], the ground cloud [G,3] and one normal per ground point [G,3].
        A refused call leaves the current map in place."""
        _, mp, mn, ms = M.cloud(map_xyz, "map", cols=3)
        _, gp, gn, gs = M.cloud(ground_xyz, "ground", cols=3)
        _, qp, qn, qs = M.cloud(ground_normals, "ground normals", cols=3)
        if gn != qn:
            raise ValueError("one normal per ground point")
        self._lp._call("mcl_set_map", mp, mn, ms, gp, qp, gn, gs, qs)

    def _measure(self, name: str, n_states: int, *inputs):
        """The two measure calls' tail: outputs per particle, the stats kept in self.last before an error raises."""
        like, qual = np.zeros(max(n_states, 1), np.float32), np.zeros(max(n_states, 1), np.float32)
        st = K.MclStats()
        rc = self._lp._rc(name, *inputs, M.ptr(like), M.ptr(qual), C.byref(st))
        self.last = st
        self._lp._check(rc)
        return like[:n_states], qual[:n_states]

    def measure(self, flat_xyz, less_sharp_xyzi, states):
        """flat [A,3], less sharp [B,4] (x y z intensity), states [N,7] (pos xyz, rot xyzw, raw) ->
        (likelihood [N], quality [N]) float32; self.last holds the call's MclStats."""
        fp, fn = M.cloud(flat_xyz, "flat", cols=3)[1:3]
        lp_, ln = M.cloud(less_sharp_xyzi, "less sharp", cols=4)[1:3]
        sp, sn = M.cloud(states, "states", cols=7)[1:3]
        return self._measure("mcl_measure", sn, fp, fn, lp_, ln, sp, sn)

    def terms(self, n: int) -> dict:
        """The parts of the last measure for its n particles: score, pos_weight, n_match, n_ground, healthy."""
        n = int(n)
        out = dict(score=np.zeros(max(n, 1), np.float32), pos_weight=np.zeros(max(n, 1), np.float32),
                   n_match=np.zeros(max(n, 1), np.uint32), n_ground=np.zeros(max(n, 1), np.uint32), healthy=np.zeros(max(n, 1), np.uint8))
        self._lp._call("mcl_get_terms", *(M.ptr(out[k]) for k in ("score", "pos_weight", "n_match", "n_ground", "healthy")), n)
        out = {k: v[:n] for k, v in out.items()}
        out["healthy"] = out["healthy"].astype(bool)
        return out

    # ---- the observation: cbLeGoFeatureCloud on the device -------------------------------------------------------------
    def configure_observation(self, cfg):
        """cfg: a K.MclObservationConfig (shipped_observation_config()), or None to switch the observation off."""
        self._lp._call("mcl_set_observation_config", C.byref(cfg) if cfg is not None else None)
        self.obs_cfg = cfg
        self._n_normals = 0          # (a new configuration forgets the prepared observation)
        self.last_observation = None

    def _prepare(self, name: str, *inputs):
        """The two prepare calls' tail: the stats kept in self.last_observation before an error raises."""
        st = K.MclObservationStats()
        rc = self._lp._rc(name, *inputs, C.byref(st))
        self.last_observation = st
        self._lp._check(rc)
        self._n_normals = st.n_less_sharp_in
        return st

    def prepare(self, flat_xyz, less_sharp_xyz, T_b2s):
        """The sweep's flat [A,3+] and less-sharp [B,3+] lists (only x y z are read) and trans_b2s_af3 (3x4 row-major) ->
        the call's MclObservationStats, also kept in self.last_observation.  The prepared clouds stay on the device."""
        _, fp, fn, fs = M.cloud(flat_xyz, "flat")
        _, lp_, ln, ls = M.cloud(less_sharp_xyz, "less sharp")
        _, tp = M.transform(T_b2s)
        return self._prepare("mcl_prepare", fp, fn, fs, lp_, ln, ls, tp)

    def prepare_from_sweep(self, source_id, T_b2s):
        """The same on the current features of a sweep source (set_lidar_sweep with features on), read where they lie."""
        _, tp = M.transform(T_b2s)
        return self._prepare("mcl_prepare_from_sweep", int(source_id), tp)

    def observation(self):
        """-> (flat [A,3], less sharp [B,4] x y z intensity, normals [B_in,3] in input order) of the prepared observation."""
        nf, nl = C.c_size_t(0), C.c_size_t(0)
        self._lp._call("mcl_get_observation", None, 0, C.byref(nf), None, 0, C.byref(nl), None, 0)
        cap = max(int(self.obs_cfg.max_less_sharp_points), 1)
        f, l = np.zeros((max(nf.value, 1), 3), np.float32), np.zeros((max(nl.value, 1), 4), np.float32)
        n = np.zeros((cap, 3), np.float32)
        self._lp._call("mcl_get_observation", M.ptr(f), len(f), C.byref(nf), M.ptr(l), len(l), C.byref(nl), M.ptr(n), cap)
        return f[: nf.value], l[: nl.value], n[: self._n_normals]

    def measure_prepared(self, states):
        """measure() on the prepared observation where it lies -> (likelihood [N], quality [N]); self.last as for measure."""
        sp, sn = M.cloud(states, "states", cols=7)[1:3]
        return self._measure("mcl_measure_prepared", sn, sp, sn)

    def close(self):
        pass      # the context owns the device state
