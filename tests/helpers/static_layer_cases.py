"""The cases of the static layer's tests (tests/test_static_layer_cpu.py, tests/test_static_layer_gpu.py), generated from
fixed seeds.  A case is a dict: ground [G,3], map [M,3] float32 and cfg (static_layer_ref.config).  check_floor() states
what the floor case has to contain for the GPU tests to prove what they claim; the CPU tests run it."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

import static_layer_ref as R

F = np.float32
D = np.float64
SHIFT = (4000.0, -3000.0, 100.0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def row_lds() -> int:
    """DDDMR_STATIC_LAYER_ROW_LDS of the header: the longest row the fill pass ranks in LDS"""
    text = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    return int(re.search(r"#define\s+DDDMR_STATIC_LAYER_ROW_LDS\s+(\d+)", text).group(1))


def ground_cell(cfg) -> np.float32:
    """sl_ground_cell of static_layer_plan.hip.h"""
    r = F(R.adaptive_radius(1)) if cfg["use_adaptive_connection"] else F(cfg["radius_of_ground_connection"])
    return F(min(max(F(0.5) * (r + F(1e-3)), F(0.05)), F(64.0)))


def _floor_clouds(nx=48, ny=56, seed=7):
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(nx) * 0.25, np.arange(ny) * 0.25, indexing="ij")
    g = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1)
    g[:, :2] += rng.uniform(-0.04, 0.04, (len(g), 2))
    g[:, 2] = rng.uniform(-0.005, 0.005, len(g))
    ramp = g[:, 0] > 8.0
    g[ramp, 2] += 0.15 * (g[ramp, 0] - 8.0)                                   # a ramp
    hole = (g[:, 0] > 3.0) & (g[:, 0] < 5.0) & (g[:, 1] > 8.0) & (g[:, 1] < 10.5)
    g = g[~hole]                                                              # a hole
    lone = np.array([[-40.0, 0.0, 0.0], [0.0, -45.0, 0.2], [50.0, 50.0, 0.5]])      # more than r_101 = 20.7 m from anything
    g = np.concatenate([g, lone, g[[100]]])                                   # ... and two coincident points
    g = g.astype(F)
    # points exactly on cell borders of the ground grid (its origin is the cloud's minimum), fixed and adaptive cell size
    lo = g.min(axis=0)
    border = []
    for cfg in (R.config(), R.config(use_adaptive_connection=1)):
        c = ground_cell(cfg)
        kx, ky = np.ceil((F(2.0) - lo[0]) / c), np.ceil((F(3.0) - lo[1]) / c)
        border += [[lo[0] + F(kx) * c, 3.1, 0.0], [2.1, lo[1] + F(ky) * c, 0.0], [lo[0] + F(kx + 1) * c, lo[1] + F(ky + 1) * c, 0.0]]
    g = np.concatenate([g, np.array(border, F)]).astype(F)
    # the map: two walls along the floor's edges, a slab 0.5 m above part of the floor, clutter above head height
    zs = np.arange(11) * 0.15
    wy, wz = np.meshgrid(np.arange(0, ny * 0.25, 0.1), zs, indexing="ij")
    wall_a = np.stack([np.full(wy.size, -0.12), wy.ravel(), wz.ravel()], axis=1)
    wx, wz = np.meshgrid(np.arange(0, nx * 0.25, 0.1), zs, indexing="ij")
    wall_b = np.stack([wx.ravel(), np.full(wx.size, -0.12), wz.ravel()], axis=1)
    slab = np.stack([rng.uniform(5.5, 8.5, 420), rng.uniform(2.0, 6.0, 420), np.full(420, 0.5)], axis=1)
    clutter = np.stack([rng.uniform(0, 12, 700), rng.uniform(0, 14, 700), rng.uniform(2.0, 3.0, 700)], axis=1)
    m = np.concatenate([wall_a, wall_b, slab, clutter]).astype(F)
    return g, m


@functools.lru_cache(maxsize=None)
def floor(adaptive: bool = False, shifted: bool = False):
    g, m = _floor_clouds()
    if shifted:
        g, m = (g.astype(D) + np.array(SHIFT)).astype(F), (m.astype(D) + np.array(SHIFT)).astype(F)
    cfg = R.config(use_adaptive_connection=1, adaptive_connection_number=20) if adaptive else R.config()
    return dict(ground=g, map=m, cfg=cfg)


@functools.lru_cache(maxsize=None)
def mini(**kw):
    """a few hundred nodes of the same make, for the small cases"""
    g, m = _floor_clouds(nx=16, ny=18, seed=11)
    keep = (m[:, 0] < 4.2) & (m[:, 1] < 4.7)
    slab = np.stack([np.random.default_rng(3).uniform(1.0, 3.0, 200), np.random.default_rng(4).uniform(1.0, 3.0, 200), np.full(200, 0.5)], axis=1).astype(F)
    return dict(ground=g, map=np.concatenate([m[keep], slab]).astype(F), cfg=R.config(**kw))


@functools.lru_cache(maxsize=None)
def long_row():
    """a clump of ground points inside one ball: rows longer than the LDS row budget"""
    rng = np.random.default_rng(5)
    n = row_lds() + 40
    clump = rng.normal(0.0, 0.08, (n, 3)).clip(-0.25, 0.25) + np.array([3.0, 3.0, 0.0])
    xs, ys = np.meshgrid(np.arange(12) * 0.5, np.arange(12) * 0.5, indexing="ij")
    rest = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1)
    m = np.stack([rng.uniform(0, 6, 300), rng.uniform(0, 6, 300), rng.uniform(0, 1, 300)], axis=1)
    return dict(ground=np.concatenate([rest, clump]).astype(F), map=m.astype(F), cfg=R.config())


@functools.lru_cache(maxsize=None)
def single():
    return dict(ground=np.array([[1.0, 2.0, 0.0]], F), map=np.array([[1.2, 2.0, 0.1], [5.0, 5.0, 0.0]], F), cfg=R.config())


def small_cases():
    m = mini()
    return {
        "n_ground_1": single(),
        "empty_map": dict(ground=m["ground"], map=np.zeros((0, 3), F), cfg=R.config()),
        "graph_off": mini(generate_static_graph=0),
        "edge_off": mini(enable_edge_detection=0),
    }


def all_cases():
    c = {"floor": floor(False), "floor_adaptive": floor(True), "floor_shifted": floor(False, True), "long_row": long_row()}
    c.update(small_cases())
    return c


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """the restatement of a case, computed once and shared (callers must not write into it)"""
    c = all_cases()[name]
    return R.build(c["ground"], c["map"], c["cfg"])


INFLATION = 0.6


@functools.lru_cache(maxsize=None)
def zone_sets():
    """two zones of about 200 points over the floor; the second holds a point far from every node"""
    t = np.linspace(0.0, 1.0, 200)
    a = np.stack([2.0 + 3.0 * t, 1.0 + 0.5 * np.sin(6 * t), np.full(200, 0.02)], axis=1)
    b = np.stack([9.0 + 0.4 * np.cos(6.28 * t), 6.0 + 3.0 * t, 0.2 + 0.0 * t], axis=1)
    b = np.concatenate([b, [[20.0, 30.0, 5.0]]])
    return a.astype(F), b.astype(F)


def check_floor():
    """what the floor case must hold (else the GPU tests prove less than they claim) -> a dict of the counts found"""
    fx, ad = reference("floor"), reference("floor_adaptive")
    cfg = floor()["cfg"]
    deg = np.diff(fx["row_start"].astype(np.int64))
    d_near = np.sqrt(fx["nearest"]).astype(D)
    found = dict(
        long_rows=int((deg > 64).sum()), few_neighbours=int((fx["counts"] < R.MIN_NEIGHBOURS).sum()),
        exactly_10=int((fx["qualifying"] == 10).sum()), exactly_11=int((fx["qualifying"] == 11).sum()),
        near=int((d_near < cfg["inscribed_radius"]).sum()), not_near=int((d_near >= cfg["inscribed_radius"]).sum()),
        k1=int((ad["kidx"] == 1).sum()), k_mid=int(((ad["kidx"] > 1) & (ad["kidx"] < R.ADAPTIVE_STEPS)).sum()),
        k101=int((ad["kidx"] == R.ADAPTIVE_STEPS).sum()),
        coincident=int((fx["weight"] == 0).sum() - len(deg)),
    )
    for k, v in found.items():
        assert v > 0, (k, found)
    return found
