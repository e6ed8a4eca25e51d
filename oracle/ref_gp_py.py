"""ctypes binding of oracle/_ref/libref_gp_*.so: the reference's own A_Star_on_PreGraph::getPath, StaticGraph and
getThetaFromParent2Expanding compiled from a reference checkout by `make -C oracle ref` (TEST INFRASTRUCTURE ONLY; see
oracle/ref/ref_gp_driver.cpp), and the case file of oracle/_ref/ref_gp_asan (oracle/ref/ref_gp_asan_main.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
BUILDS = ("O0", "O2")
ASAN = os.path.join(REF_DIR, "ref_gp_asan")
MAGIC = 0x3153435047464552                 # "REFGPCS1"
_libs: dict = {}


def path(build: str) -> str:
    return os.path.join(REF_DIR, f"libref_gp_{build}.so")


def available() -> bool:
    """True when both builds of the compiled reference and the sanitizer program are here (build() makes them where a
    reference checkout is)."""
    return all(os.path.exists(path(b)) for b in BUILDS) and os.path.exists(ASAN)


def load(build: str = "O2") -> C.CDLL:
    if build in _libs:
        return _libs[build]
    lib = C.CDLL(path(build))
    vp, sz, db, u32 = C.c_void_p, C.c_size_t, C.c_double, C.c_uint32
    lib.ref_gp_plan.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, sz, db, db, db, db, db, u32, u32, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.ref_gp_plan.restype = C.c_int
    lib.ref_gp_theta.argtypes = [vp, sz, vp]
    lib.ref_gp_theta.restype = None
    _libs[build] = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def arrays(case: dict) -> dict:
    """A case -- ground [n,3], intensity [n] or None, row_start / neighbour / weight (CSR), order (the permutation in which
    edges reach insertNode; None: as stored), dgraph, cfg (a_star_expanding_radius, inscribed_radius,
    inflation_descending_rate, turning_weight; max_obstacle_distance optional), start, goal -- as the driver's arrays."""
    ground = np.ascontiguousarray(case["ground"], np.float32).reshape(-1, 3)
    n = len(ground)
    xyzi = np.zeros((n, 4), np.float32)
    xyzi[:, :3] = ground
    if case.get("intensity") is not None:
        xyzi[:, 3] = np.asarray(case["intensity"], np.float32)
    nb = np.ascontiguousarray(case["neighbour"], np.uint32)
    order = np.arange(len(nb), dtype=np.uint32) if case.get("order") is None else np.ascontiguousarray(case["order"], np.uint32)
    cfg = case["cfg"]
    par = (float(cfg["a_star_expanding_radius"]), float(cfg["inscribed_radius"]), float(cfg["inflation_descending_rate"]),
           float(cfg.get("max_obstacle_distance", 5.0)), float(cfg["turning_weight"]))
    return dict(xyzi=xyzi, row_start=np.ascontiguousarray(case["row_start"], np.uint32), neighbour=nb,
                weight=np.ascontiguousarray(case["weight"], np.float32), order=order,
                dgraph=np.ascontiguousarray(case["dgraph"], np.float64), par=par, start=int(case["start"]), goal=int(case["goal"]))


def plan(case: dict, build: str = "O2") -> dict:
    """One getPath of the reference -> path (uint32; empty when getPath left it so), per node g, f (float32), parent
    (uint32), opened, closed (bool) as read back after getPath, n_closed, set_size (f_priority_set_'s final size)."""
    lib = load(build)
    a = arrays(case)
    n = len(a["xyzi"])
    assert len(a["row_start"]) == n + 1 and len(a["weight"]) == len(a["neighbour"]) == len(a["order"])
    assert sorted(a["order"].tolist()) == list(range(len(a["order"])))
    out_path = np.zeros(n + 1, np.uint32)
    g, f, parent = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    opened, closed = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    plen, ssize = C.c_size_t(0), C.c_size_t(0)
    rc = lib.ref_gp_plan(_ptr(a["xyzi"]), n, _ptr(a["row_start"]), _ptr(a["neighbour"]), _ptr(a["weight"]), _ptr(a["order"]),
                         len(a["neighbour"]), _ptr(a["dgraph"]), len(a["dgraph"]), *a["par"], a["start"], a["goal"], _ptr(out_path),
                         len(out_path), C.byref(plen), _ptr(g), _ptr(f), _ptr(parent), _ptr(opened), _ptr(closed), C.byref(ssize))
    if rc != 0:
        raise RuntimeError(f"ref_gp_plan refused the case ({rc})")
    return dict(path=out_path[: plen.value].copy(), g=g, f=f, parent=parent, opened=opened.astype(bool), closed=closed.astype(bool),
                n_closed=int(closed.sum()), set_size=int(ssize.value))


def theta(xy, build: str = "O2") -> np.ndarray:
    """getThetaFromParent2Expanding for [n,6] float32 rows (parent x y, current x y, expanding x y) -> [n] float64"""
    lib = load(build)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 6)
    out = np.zeros(len(xy), np.float64)
    lib.ref_gp_theta(_ptr(xy), len(xy), _ptr(out))
    return out


def write_cases(file: str, cases, theta_xy=None) -> None:
    """the case file that oracle/_ref/ref_gp_asan reads"""
    with open(file, "wb") as fp:
        cases = list(cases)
        fp.write(struct.pack("<QQ", MAGIC, len(cases)))
        for case in cases:
            a = arrays(case)
            fp.write(struct.pack("<QQQII5d", len(a["xyzi"]), len(a["neighbour"]), len(a["dgraph"]), a["start"], a["goal"], *a["par"]))
            for k in ("xyzi", "row_start", "neighbour", "weight", "order", "dgraph"):
                fp.write(a[k].tobytes())
        xy = np.zeros((0, 6), np.float32) if theta_xy is None else np.ascontiguousarray(theta_xy, np.float32).reshape(-1, 6)
        fp.write(struct.pack("<Q", len(xy)))
        fp.write(xy.tobytes())
