"""The feeds' shared voxel table (csrc/voxel_table.hip.h) is emptied by the pass that reads it, never by a memset: a call
must leave it clean for the next one, also when that next call uses a smaller part of the table or cleans slots whose
sums it never read.

For each of the three paths one context is fed A, then B, then A again, and every call is compared with what a fresh
context gives for the same input: the counts exactly, the points one to one within 1e-5 m (the figure of the paths'
own suites: the only difference left is the order of the double atomic adds).  The shapes are the smallest that reach
both ways of cleaning."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

from dddmr_navigation_amd import configs, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_feed_ref as R  # noqa: E402
import depth_image_cases as Cs  # noqa: E402

pytestmark = pytest.mark.gpu

IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
MS = 1_000_000
TBS_CAM = (0.2, 0.0, 0.3) + tuple(scenes.quat_from_rpy(0.0, 0.05, 0.0))
TGB = (-1.0, 0.2, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.02, 0.3))
ZMIN, ZMAX = 0.0, 2.0
TOL = 1e-5


def planner():
    return LocalPlanner([configs.bench_theory("C1")], max_points=40_000)


def sort_rows(p):
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def assert_same(got, ref, what):
    """got / ref: tuples of counts and point arrays.  Counts equal; points, sorted, matched one to one within TOL (a
    last-bit difference may swap two neighbours of the sorted order, so rows are paired by distance, not by rank)."""
    for g, r in zip(got, ref):
        if not isinstance(r, np.ndarray):
            assert g == r, (what, got[:-1], ref[:-1])
            continue
        assert len(g) == len(r), (what, len(g), len(r))
        if len(r):
            g, r = sort_rows(g[:, :3]), sort_rows(r[:, :3])
            d, idx = cKDTree(r).query(g)
            print(f"{what}: {len(r)} points, largest distance {d.max():.3e} m")
            assert d.max() <= TOL, (what, d.max())
            assert len(np.unique(idx)) == len(r), what


def a_b_a(feed, inputs, what):
    """feed(lp, x, k) -> (counts..., points) of the k-th call.  inputs: {"A": ..., "B": ...}"""
    fresh = {}
    for name, x in inputs.items():
        with planner() as lp:
            fresh[name] = feed(lp, x, 0)
    with planner() as lp:
        for k, name in enumerate("ABA"):
            assert_same(feed(lp, inputs[name], k), fresh[name], f"{what}, call {k} ({name})")
    return fresh


def lidar_inputs():
    scan = scenes.lidar_scan(scenes.cloud_c2(), seed=5)
    a = scan[:: max(len(scan) // 3000, 1)][:3000]
    rng = np.random.default_rng(7)
    b = rng.uniform([1.01, 0.51, 0.31], [1.09, 0.59, 0.39], size=(200, 3)).astype(np.float32)   # inside one 0.1 m voxel
    return {"A": a, "B": b}


def test_lidar_table_is_left_clean():
    tbs = (0.0, 0.0, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.0))

    def feed(lp, scan, k):
        n = lp.set_scan(scan, tbs, IDENT, 8.0, 1.8)
        return n, lp.get_cloud()

    fresh = a_b_a(feed, lidar_inputs(), "lidar")
    assert 1000 <= fresh["A"][0] <= 2000           # about 1500 voxels of about 3000 points: an 8192-slot table
    assert fresh["B"][0] == 1                      # 200 points, one voxel: the first 1024 slots of it


def depth_cloud_inputs():
    fr = scenes.depth_frame(scenes.cloud_c2(), R.compose(TGB, TBS_CAM), 640, 480, 1.5, 1.0, 8.0, seed=3)
    z = R.transform(np.nan_to_num(fr, nan=0.0), TBS_CAM)[:, 2].astype(np.float64)
    alive = np.flatnonzero(np.isfinite(fr).all(axis=1) & (z >= ZMIN) & (z <= ZMAX))
    assert len(alive) >= R.VOXELIZE_ABOVE + 1
    # only the surviving records, so the two frames also use tables of different sizes
    return {"A": fr[alive[: R.VOXELIZE_ABOVE + 1]].copy(), "B": fr[alive[:500]].copy()}


def test_depth_cloud_table_is_left_clean():
    inputs = depth_cloud_inputs()
    assert R.n_survivors(inputs["A"], TBS_CAM, ZMIN, ZMAX) == R.VOXELIZE_ABOVE + 1    # the voxelising branch
    assert R.n_survivors(inputs["B"], TBS_CAM, ZMIN, ZMAX) == 500                     # passes through: cleans unread slots

    def feed(lp, frame, k):
        if k == 0:
            lp.set_depth_source(0, ZMIN, ZMAX, 0, max_frame_points=32768, max_frames=1)
        return lp.set_depth_frame(0, frame, TBS_CAM, TGB, 10**9 + 33 * MS * k) + (lp.get_cloud(),)

    fresh = a_b_a(feed, inputs, "depth cloud")
    assert fresh["A"][0] < R.VOXELIZE_ABOVE + 1    # voxelised
    assert fresh["B"][0] == 500                    # unchanged


@pytest.mark.parametrize("step", [1, 2])           # the four-pixel and the one-pixel insert kernel
def test_depth_image_tables_are_left_clean(step):
    img, K4 = Cs.render(64, 48, 0, 1)
    assert 0.05 < (img == 0).mean() < 0.95
    inputs = {"A": img, "B": np.zeros_like(img)}   # B: one camera-frame voxel, adds to its count only

    def feed(lp, image, k):
        if k == 0:
            lp.set_depth_image_source(1, -100.0, 100.0, 64, 48, *K4, max_distance=4.0, leaf_size=0.05, sample_step=step)
        counts = lp.set_depth_image(1, image, Cs.TBO_CAM, Cs.POSES[0], 10**9 + 33 * MS * k)
        return counts + (lp.get_depth_image_cloud(1), lp.get_cloud())

    fresh = a_b_a(feed, inputs, f"depth image step {step}")
    assert fresh["A"][0] > 100                     # many camera-frame voxels
    assert fresh["B"][0] == 1 and not fresh["B"][4].any()     # one point, (0, 0, 0)
