"""Host-side mirror of the localiser's device half on top of the C-ABI (dddmr_rollout_mcl_*):
mcl_3dl's LidarMeasurementModelLikelihood::measure for a batch of particles
(dddmr_mcl_3dl/src/lidar_measurement_model_likelihood.cpp:86-252, src/mcl_3dl.cpp:466-503) and the preparation of its
observation, MCL3dlNode::cbLeGoFeatureCloud (src/mcl_3dl.cpp:263-464).
All compute and all state live in the HIP library.  ParticleFilter keeps the particle set itself in device memory
(dddmr_rollout_mcl_filter_*): prediction, weighting, bias, estimate and resampling run there, on random numbers the
caller draws."""
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


def shipped_filter_config(**kw) -> K.MclFilterConfig:
    """The filter block of the shipped mcl_3dl.yaml, with room for the particle counts this project measures at."""
    return M.struct_from(K.MclFilterConfig, dict(
        max_particles=1 << 14, odom_err_integ_lin_tc=5.0, odom_err_integ_ang_tc=10.0, bias_var_dist=2.0, bias_var_ang=1.57), kw)


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


def _f32(a, shape, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {a.shape}")
    return a


class ParticleFilter:
    """mcl_3dl's particle set in device memory, beside a ParticleMeasure of the same context (its mcl_create comes first).
    States are [N,13] float32 in State6DOF::operator[] order (pos xyz, rot xyzw, odom_err_integ_lin_ xyz,
    odom_err_integ_ang_ xyz); noise4 rows are noise_ll_, noise_la_, noise_al_, noise_aa_; resample / add_noise rows are
    [*,10]: pos xyz, rot xyzw, odom_err_integ_ang_ xyz of the noise state.  Every random number is the caller's."""

    def __init__(self, lp, cfg: K.MclFilterConfig):
        self._lp = lp
        self.cfg = cfg
        lp._call("mcl_filter_create", C.byref(cfg))
        self.n = 0
        self.last = None             # the last measure's MclStats (the lidar model's, when it ran)
        self.last_resample = None

    def set_particles(self, states, probability=None, noise4=None):
        """probability None: float(1.0 / N) as pf::init computes it; noise4 None: zeros."""
        states = np.ascontiguousarray(states, dtype=np.float32)
        if states.ndim != 2 or states.shape[1] != 13:
            raise ValueError("states: [N,13]")
        n = states.shape[0]
        p = None if probability is None else _f32(probability, (n,), "probability")
        z = None if noise4 is None else _f32(noise4, (n, 4), "noise4")
        self._lp._call("mcl_filter_set_particles", M.ptr(states), None if p is None else M.ptr(p), None if z is None else M.ptr(z), n)
        self.n = n

    def particles(self) -> dict:
        """-> dict(states [N,13], probability [N], bias [N], noise4 [N,4]) as they lie on the device."""
        n = C.c_size_t(0)
        self._lp._call("mcl_filter_get_particles", None, None, None, None, 0, C.byref(n))
        N = n.value
        out = dict(states=np.zeros((N, 13), np.float32), probability=np.zeros(N, np.float32), bias=np.zeros(N, np.float32),
                   noise4=np.zeros((N, 4), np.float32))
        self._lp._call("mcl_filter_get_particles", M.ptr(out["states"]), M.ptr(out["probability"]), M.ptr(out["bias"]), M.ptr(out["noise4"]),
                       N, C.byref(n))
        return out

    def predict(self, odom_prev, odom_cur, time_diff):
        """setOdoms + predict: the two odometry poses as pos xyz, rot xyzw."""
        a, b = _f32(odom_prev, (7,), "odom_prev"), _f32(odom_cur, (7,), "odom_cur")
        self._lp._call("mcl_filter_predict", M.ptr(a), M.ptr(b), float(time_diff))

    def set_noise(self, noise4):
        z = _f32(noise4, (self.n, 4), "noise4")
        self._lp._call("mcl_filter_set_noise", M.ptr(z), self.n)

    def measure(self, likelihood=None, quality=None, state_prev=None) -> K.MclFilterEstimate:
        """MCL3dlNode::measure up to the covariance.  likelihood None: the lidar model runs on the resident poses and the
        prepared observation.  state_prev None: the bias is 1.  -> the call's MclFilterEstimate; self.last its MclStats."""
        lk = None if likelihood is None else _f32(likelihood, (self.n,), "likelihood")
        q = None if quality is None else _f32(quality, (self.n,), "quality")
        sp = None if state_prev is None else _f32(state_prev, (7,), "state_prev")
        est, st = K.MclFilterEstimate(), K.MclStats()
        rc = self._lp._rc("mcl_filter_measure", None if lk is None else M.ptr(lk), None if q is None else M.ptr(q), self.n,
                          None if sp is None else M.ptr(sp), C.byref(est), C.byref(st))
        self.last = st
        self._lp._check(rc)
        return est

    def reset_integ(self):
        self._lp._call("mcl_filter_reset_integ")

    def resample(self, u, noise_rows) -> K.MclFilterResampleStats:
        """u: the canonical draw in [0, 1); noise_rows [R,10], one per duplicate in index order (R below the number of
        duplicates is refused with the stats in self.last_resample and nothing changed)."""
        rows = np.ascontiguousarray(noise_rows, dtype=np.float32).reshape(-1, 10)
        st = K.MclFilterResampleStats()
        rc = self._lp._rc("mcl_filter_resample", float(u), M.ptr(rows) if len(rows) else None, len(rows), C.byref(st))
        self.last_resample = st
        self._lp._check(rc)
        return st

    def add_noise(self, noise_rows):
        rows = _f32(noise_rows, (self.n, 10), "noise_rows")
        self._lp._call("mcl_filter_add_noise", M.ptr(rows), self.n)
