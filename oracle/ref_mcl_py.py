"""ctypes binding of oracle/_ref/libref_mcl_*.so: mcl_3dl's own LidarMeasurementModelLikelihood::measure and
State6DOF::transform compiled from a reference checkout by `make -C oracle ref` (TEST INFRASTRUCTURE ONLY; see
oracle/ref/ref_mcl_driver.cpp)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
BUILDS = ("O0", "O2")
TRACE = ("n_ground", "avg_nx", "avg_ny", "avg_nz", "roll", "pitch", "yaw", "roll_diff")
UNTRUSTED, STEEP, ROLL = 0, 1, 2          # which of measure()'s debug lines a particle left (ref_mcl_driver.cpp)
_libs: dict = {}


def path(build: str) -> str:
    return os.path.join(REF_DIR, f"libref_mcl_{build}.so")


def available() -> bool:
    """True when both builds of the compiled reference are here (build() makes them where a reference checkout is)."""
    return all(os.path.exists(path(b)) for b in BUILDS)


def load(build: str = "O2") -> C.CDLL:
    if build in _libs:
        return _libs[build]
    lib = C.CDLL(path(build))
    vp, sz = C.c_void_p, C.c_size_t
    lib.ref_mcl_measure.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, vp, sz, vp, sz, vp, vp, sz, vp, sz, vp, sz,
                                    vp, vp, vp, vp]
    lib.ref_mcl_measure.restype = C.c_int
    lib.ref_mcl_transform.argtypes = [vp, sz, vp, sz, vp]
    lib.ref_mcl_transform.restype = None
    lib.ref_mcl_quality_minmax.argtypes = [vp, sz, vp]
    lib.ref_mcl_quality_minmax.restype = None
    _libs[build] = lib
    return lib


def _f32(a, cols):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def measure(cfg, map_xyz, ground_xyz, ground_normals, flat_xyz, less_sharp_xyzi, states, build: str = "O2") -> dict:
    """cfg: anything with match_dist_min, match_dist_flat, radius_of_ground_search, threshold_for_trusted_ground.
    -> dict(likelihood[N] f32, quality[N] f32, trace[N,8] f64 (columns TRACE; NaN where the particle's branch logged
    none), branch[N] i32 (UNTRUSTED / STEEP / ROLL), quality_min, quality_max f32)"""
    lib = load(build)
    m, g, n = _f32(map_xyz, 3), _f32(ground_xyz, 3), _f32(ground_normals, 3)
    f, l, s = _f32(flat_xyz, 3), _f32(less_sharp_xyzi, 4), _f32(states, 7)
    assert len(g) == len(n)
    N = len(s)
    like, qual = np.zeros(N, np.float32), np.zeros(N, np.float32)
    trace, branch = np.zeros((N, len(TRACE)), np.float64), np.zeros(N, np.int32)
    rc = lib.ref_mcl_measure(float(cfg.match_dist_min), float(cfg.match_dist_flat), float(cfg.radius_of_ground_search),
                             int(cfg.threshold_for_trusted_ground), _ptr(m), len(m), _ptr(g), len(g), _ptr(n), _ptr(f), len(f),
                             _ptr(l), len(l), _ptr(s), N, _ptr(like), _ptr(qual), _ptr(trace), _ptr(branch))
    if rc != 0:
        raise RuntimeError(f"ref_mcl_measure: particle {-rc - 1} left debug records of no known shape")
    mm = quality_minmax(qual, build)
    return dict(likelihood=like, quality=qual, trace=trace, branch=branch, quality_min=mm[0], quality_max=mm[1])


def transform(points_xyz, states, build: str = "O2") -> np.ndarray:
    """State6DOF::transform of [M,3] points by [N,7] states -> [N,M,3] float32"""
    lib = load(build)
    p, s = _f32(points_xyz, 3), _f32(states, 7)
    out = np.zeros((len(s), len(p), 3), np.float32)
    lib.ref_mcl_transform(_ptr(p), len(p), _ptr(s), len(s), _ptr(out))
    return out


def quality_minmax(quality, build: str = "O2") -> np.ndarray:
    """the running minimum / maximum of mcl_3dl.cpp:476-498 (restated in the driver) -> [2] float32"""
    lib = load(build)
    q = np.ascontiguousarray(quality, dtype=np.float32).reshape(-1)
    out = np.zeros(2, np.float32)
    lib.ref_mcl_quality_minmax(_ptr(q), len(q), _ptr(out))
    return out
