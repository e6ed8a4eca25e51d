"""ctypes binding of oracle/liboracle.so (TEST INFRASTRUCTURE ONLY)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

from dddmr_navigation_amd import _capi as K

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class OracleResult(C.Structure):
    _fields_ = [
        ("planner_state", C.c_int32),
        ("best_index", C.c_int32),
        ("best_cost", C.c_double),
        ("vx", C.c_double), ("vy", C.c_double), ("wz", C.c_double),
        ("n_samples", C.c_uint32),
        ("n_local", C.c_uint32),
        ("n_generated", C.c_uint32),
        ("reserved", C.c_uint32),
        ("k_sum", C.c_uint64),
        ("steps_eval", C.c_uint64),
        ("steps_total", C.c_uint64),
        ("t_generate_s", C.c_double), ("t_kdtree_s", C.c_double), ("t_score_s", C.c_double),
    ]


def load(build_if_missing: bool = True) -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = os.path.join(_HERE, os.environ.get("DDDMR_ORACLE_LIB", "liboracle.so"))     # (liboracle_asan.so: `make -C oracle asan`)
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError(f"{path} missing; run `make -C oracle`")
        subprocess.check_call(["make", "-C", _HERE, "-s"])
    lib = C.CDLL(path)
    lib.oracle_velocity_iterator.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.oracle_velocity_iterator.restype = C.c_int
    lib.oracle_samples.argtypes = [C.POINTER(K.TheoryConfig), C.POINTER(K.TickInput), C.c_void_p, C.c_int]
    lib.oracle_samples.restype = C.c_int
    lib.oracle_generate.argtypes = [C.POINTER(K.TheoryConfig), C.POINTER(K.TickInput), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.oracle_generate.restype = C.c_int
    lib.oracle_radius_count.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_float, C.c_void_p]
    lib.oracle_radius_count.restype = C.c_int
    lib.oracle_path_blocked.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double,
                                        C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p]
    lib.oracle_path_blocked.restype = C.c_int
    lib.oracle_tick.argtypes = [C.POINTER(K.TheoryConfig), C.c_void_p, C.c_size_t, C.c_size_t,
                                C.c_void_p, C.c_size_t, C.POINTER(K.TickInput), C.c_uint32, C.c_uint32,
                                C.c_int, C.POINTER(OracleResult), C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]
    lib.oracle_tick.restype = C.c_int
    lib.oracle_feed.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.c_double, C.c_double, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.oracle_feed.restype = C.c_int
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def velocity_iterator(mn: float, mx: float, n: int, no_zero_insert: bool = False) -> np.ndarray:
    lib = load()
    out = np.zeros(4096, dtype=np.float64)
    k = lib.oracle_velocity_iterator(mn, mx, n, int(no_zero_insert), _ptr(out), out.size)
    return out[:k].copy()


def samples(theory: K.TheoryConfig, tick_in: K.TickInput) -> np.ndarray:
    lib = load()
    n = lib.oracle_samples(C.byref(theory), C.byref(tick_in), None, 0)
    out = np.zeros((max(n, 1), 3), dtype=np.float32)
    lib.oracle_samples(C.byref(theory), C.byref(tick_in), _ptr(out), n)
    return out[:n]


def generate(theory: K.TheoryConfig, tick_in: K.TickInput, sample, capacity: int = 4096):
    """-> (poses[S,7] f64, cuboids[S,8,3] f32, minmax[S,2,3] f32); S == 0 if rejected."""
    lib = load()
    s = np.asarray(sample, dtype=np.float32).reshape(3)
    poses = np.zeros((capacity, 7), dtype=np.float64)
    cub = np.zeros((capacity, 8, 3), dtype=np.float32)
    mm = np.zeros((capacity, 2, 3), dtype=np.float32)
    n = lib.oracle_generate(C.byref(theory), C.byref(tick_in), _ptr(s), _ptr(poses), _ptr(cub), _ptr(mm), capacity)
    assert n <= capacity
    return poses[:n], cub[:n], mm[:n]


def radius_count(cloud_xyz: np.ndarray, queries: np.ndarray, radius: float) -> np.ndarray:
    lib = load()
    cloud = np.ascontiguousarray(cloud_xyz, dtype=np.float32)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)
    counts = np.zeros(len(q), dtype=np.int32)
    lib.oracle_radius_count(_ptr(cloud), cloud.shape[0], cloud.strides[0], _ptr(q), len(q), radius, _ptr(counts))
    return counts


def path_blocked(cloud: np.ndarray, plan_xyzi: np.ndarray, check_radius: float):
    """PathBlockedStrategy::selfMark -> (blocked ratio in percent, opinion 0/1, per-point flags)."""
    lib = load()
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    if cloud.ndim != 2:
        cloud = cloud.reshape(-1, 4)
    plan = np.ascontiguousarray(plan_xyzi, dtype=np.float32).reshape(-1, 4)
    flags = np.zeros(max(len(plan), 1), dtype=np.uint8)
    ratio, op = C.c_double(0.0), C.c_int32(0)
    stride = cloud.strides[0] if len(cloud) else 16
    lib.oracle_path_blocked(_ptr(cloud), cloud.shape[0], stride, _ptr(plan), len(plan), float(check_radius),
                            C.byref(ratio), C.byref(op), _ptr(flags))
    return ratio.value, op.value, flags[: len(plan)].astype(bool)


@dataclass
class TickOut:
    result: OracleResult
    costs: np.ndarray
    steps: np.ndarray
    samples: np.ndarray
    last_poses: np.ndarray
    min_margin: np.ndarray | None


def tick(theory: K.TheoryConfig, cloud: np.ndarray, plan: np.ndarray, tick_in: K.TickInput,
         begin: int = 0, end: int = 0xFFFFFFFF, n_threads: int = 1, want_margin: bool = False) -> TickOut:
    """One oracle control tick.  cloud: [P, >=3] float32 (row stride = record
    stride), plan: [M,7] float64."""
    lib = load()
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    if cloud.ndim != 2 or (cloud.shape[0] and cloud.shape[1] < 3):
        raise ValueError("cloud must be [P, >=3]")
    plan = np.ascontiguousarray(plan, dtype=np.float64).reshape(-1, 7)
    n = lib.oracle_samples(C.byref(theory), C.byref(tick_in), None, 0)
    b = min(begin, n)
    e = max(b, min(end, n))
    nl = e - b
    costs = np.zeros(max(nl, 1), dtype=np.float64)
    steps = np.zeros(max(nl, 1), dtype=np.int32)
    smp = np.zeros((max(nl, 1), 3), dtype=np.float32)
    lastp = np.zeros((max(nl, 1), 7), dtype=np.float64)
    mm = np.zeros(max(nl, 1), dtype=np.float32) if want_margin else None
    res = OracleResult()
    stride = cloud.strides[0] if cloud.shape[0] else 16
    rc = lib.oracle_tick(C.byref(theory), _ptr(cloud), cloud.shape[0], stride, _ptr(plan), plan.shape[0],
                         C.byref(tick_in), begin, end, n_threads, C.byref(res), _ptr(costs), _ptr(steps),
                         _ptr(smp), _ptr(lastp), _ptr(mm))
    if rc != 0:
        raise RuntimeError(f"oracle_tick failed: {rc}")
    return TickOut(res, costs[:nl], steps[:nl], smp[:nl], lastp[:nl], None if mm is None else mm[:nl])


def feed(scan_xyz: np.ndarray, T_base_sensor, T_gbl_base, window: float, height: float) -> np.ndarray:
    """cbSensor local-mode feed -> [K,3] float32 in the global frame, voxel-index order."""
    lib = load()
    scan = np.ascontiguousarray(scan_xyz, dtype=np.float32)
    tbs = (C.c_double * 7)(*[float(v) for v in T_base_sensor])
    tgb = (C.c_double * 7)(*[float(v) for v in T_gbl_base])
    out = np.zeros((max(len(scan), 1), 3), dtype=np.float32)
    n = C.c_size_t(0)
    stride = scan.strides[0] if len(scan) else 12
    lib.oracle_feed(_ptr(scan), len(scan), stride, tbs, tgb, window, height, _ptr(out), len(out), C.byref(n))
    return out[: n.value].copy()


class MarkingOracle:
    """CPU restatement of the global-mode marking / clearing layer (oracle_marking.cpp)."""

    def __init__(self, cfg: K.MarkingConfig, ground: np.ndarray, static_map: np.ndarray):
        lib = load()
        lib.oracle_marking_create.argtypes = [C.POINTER(K.MarkingConfig), C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.c_size_t]
        lib.oracle_marking_create.restype = C.c_void_p
        lib.oracle_marking_destroy.argtypes = [C.c_void_p]
        lib.oracle_marking_reset.argtypes = [C.c_void_p]
        lib.oracle_marking_update.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.POINTER(K.MarkingStats)]
        lib.oracle_marking_update.restype = C.c_int
        lib.oracle_marking_get_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.oracle_marking_get_points.restype = C.c_size_t
        for f in (lib.oracle_marking_get_voxels, lib.oracle_marking_get_dgraph, lib.oracle_marking_get_lethal):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            f.restype = C.c_size_t
        lib.oracle_marking_get_decisions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.oracle_marking_get_decisions.restype = C.c_size_t
        lib.oracle_marking_trace_dgraph.argtypes = [C.c_void_p, C.c_int]
        lib.oracle_marking_get_dgraph_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.oracle_marking_get_dgraph_trace.restype = C.c_size_t
        self._lib = lib
        g = np.ascontiguousarray(ground, dtype=np.float32)
        m = np.ascontiguousarray(static_map, dtype=np.float32)
        if m.ndim != 2:
            m = m.reshape(-1, 3)
        self.n_ground = len(g)
        self._h = lib.oracle_marking_create(C.byref(cfg), _ptr(g), len(g), g.strides[0] if len(g) else 12,
                                            _ptr(m), len(m), m.strides[0] if len(m) else 12)

    def __del__(self):
        try:
            if self._h:
                self._lib.oracle_marking_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def reset(self):
        self._lib.oracle_marking_reset(self._h)

    def trace_dgraph(self, on: bool = True):
        """Record the DynamicGraph calls from here on (the graph must be in its initial state)."""
        self._lib.oracle_marking_trace_dgraph(self._h, int(on))

    def dgraph_trace(self) -> np.ndarray:
        """-> [T, 3] float64 (op, key, value): op 0 = initial(n = key, value), 1 = setValue, 2 = clearValue."""
        n = self._lib.oracle_marking_get_dgraph_trace(self._h, None, 0)
        out = np.zeros((max(n, 1), 3), dtype=np.float64)
        self._lib.oracle_marking_get_dgraph_trace(self._h, _ptr(out), n)
        return out[:n]

    def update(self, obs_gbl_xyz: np.ndarray, T_base_sensor, T_gbl_base) -> K.MarkingStats:
        obs = np.ascontiguousarray(np.asarray(obs_gbl_xyz, dtype=np.float32)[:, :3])
        tbs = (C.c_double * 7)(*[float(v) for v in T_base_sensor])
        tgb = (C.c_double * 7)(*[float(v) for v in T_gbl_base])
        st = K.MarkingStats()
        self._lib.oracle_marking_update(self._h, _ptr(obs), len(obs), tbs, tgb, C.byref(st))
        return st

    def voxels(self) -> np.ndarray:
        n = self._lib.oracle_marking_get_voxels(self._h, None, 0)
        out = np.zeros((max(n, 1), 3), dtype=np.int32)
        self._lib.oracle_marking_get_voxels(self._h, _ptr(out), len(out))
        return out[:n]

    def points(self, with_voxels: bool = False):
        """generator points of the alive markings (what the dGraph update searches the ground nodes with)"""
        n = self._lib.oracle_marking_get_points(self._h, None, None, 0)
        out = np.zeros((max(n, 1), 3), dtype=np.float32)
        vox = np.zeros((max(n, 1), 3), dtype=np.int32)
        self._lib.oracle_marking_get_points(self._h, _ptr(out), _ptr(vox), len(out))
        return (out[:n], vox[:n]) if with_voxels else out[:n]

    def dgraph(self) -> np.ndarray:
        out = np.zeros(self.n_ground + 1, dtype=np.float64)
        self._lib.oracle_marking_get_dgraph(self._h, _ptr(out), out.size)
        return out

    def lethal(self) -> np.ndarray:
        out = np.zeros(self.n_ground + 1, dtype=np.uint8)
        self._lib.oracle_marking_get_lethal(self._h, _ptr(out), out.size)
        return out.astype(bool)

    def decisions(self, which: int):
        """which = 0: selfClear (voxels, margins, removed); 1: selfMark (voxels, margins, added)."""
        n = self._lib.oracle_marking_get_decisions(self._h, which, None, None, None, 0)
        v = np.zeros((max(n, 1), 3), dtype=np.int32)
        m = np.zeros(max(n, 1), dtype=np.float32)
        f = np.zeros(max(n, 1), dtype=np.uint8)
        self._lib.oracle_marking_get_decisions(self._h, which, _ptr(v), _ptr(m), _ptr(f), n)
        return v[:n], m[:n], f[:n].astype(bool)


def in_lidar_observation(cfg: K.MarkingConfig, T_base_sensor, T_gbl_base, pts_xyz: np.ndarray):
    lib = load()
    lib.oracle_in_lidar_observation.argtypes = [C.POINTER(K.MarkingConfig), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    pts = np.ascontiguousarray(pts_xyz, dtype=np.float32).reshape(-1, 3)
    inside = np.zeros(len(pts), dtype=np.uint8)
    margin = np.zeros(len(pts), dtype=np.float32)
    tbs = (C.c_double * 7)(*[float(v) for v in T_base_sensor])
    tgb = (C.c_double * 7)(*[float(v) for v in T_gbl_base])
    lib.oracle_in_lidar_observation(C.byref(cfg), tbs, tgb, _ptr(pts), len(pts), _ptr(inside), _ptr(margin))
    return inside.astype(bool), margin
