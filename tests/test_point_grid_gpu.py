"""The point grid of csrc/point_grid.hip.h on the device -- the library's own grid_shape, grid_alloc and grid_build, then
every walk (grid_for_each with its packed fast path, grid_for_each_wave, grid_radius_count, grid_nearest,
grid_nearest_id) -- through its one entry point, selftest_point_grid, against tests/helpers/point_grid_ref.py bit for bit,
on the designed cases of tests/helpers/point_grid_cases.py.  tests/test_point_grid_cpu.py shows on the reference alone
that every neighbour lies in the box of cells of its query and that each case holds what it is for, so agreement with
the box population here means the walks lose nothing.  (The lost neighbour case is the one exception by design: its
box population misses a neighbour at pad 1e-4, the walks are expected to do what the arithmetic says, and the layers
refuse a static cloud that wide -- the last test.)"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from dddmr_navigation_amd import _capi as K, configs, depth_layer, marking
from dddmr_navigation_amd import _marshal as M
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import point_grid_cases as cases  # noqa: E402
import point_grid_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
FULL = 0x7FFFFFFF


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C1")]) as p:
        yield p


def _run(lp, case, stop_at):
    return lp.selftest_point_grid(case.pts, case.lo, case.hi, case.cell_xy, case.cell_z, case.cap_cells, case.queries, case.r_box,
                                  case.r2, stop_at)


def _check_grid(out, case, e):
    g = e["grid"]
    assert (out["nx"], out["ny"], out["nz"]) == (g.nx, g.ny, g.nz), "grid_shape: cells"
    got = np.array([out[k] for k in ("ox", "oy", "oz", "inv_xy", "inv_z")], F)
    assert np.array_equal(R.bits(got), R.bits(np.array([g.ox, g.oy, g.oz, g.inv_xy, g.inv_z], F))), "grid_shape: origin and inverse cell sizes"
    n = len(case.pts)
    want_start = R.cell_start(g, case.pts)
    assert np.array_equal(out["cell_start"], want_start) and int(out["cell_start"][-1]) == n, "cell_start is not the scan of the histogram"
    idx = out["sorted"][:, 3].astype(np.int64)
    assert np.array_equal(np.sort(idx), np.arange(n)), "the sorted records' indices are no permutation"
    assert np.array_equal(out["sorted"][:, :3], R.bits(case.pts).reshape(-1, 3)[idx]), "a sorted record does not carry its point"
    # the run of every cell holds the reference's set for it (the order inside a cell is free: the slots come from atomics)
    cell_of_slot = np.repeat(np.arange(len(want_start) - 1), np.diff(want_start.astype(np.int64)))
    assert np.array_equal(cell_of_slot, R.point_cells(g, case.pts)[3][idx]), "a point sits in the run of another cell"


def _check_queries(out, case, e, stop_at):
    box, brute = e["box"], e["brute"]
    thr, wav = out["thread"], out["wave"]
    m = len(case.queries)
    inside = box["member"] & brute["inside"]
    full = inside.sum(axis=1)
    if case.name != "lost neighbour":
        assert np.array_equal(full, brute["count"])                          # (containment, test_point_grid_cpu.py)
    for name, got in (("grid_for_each", thr[:, 5:8]), ("grid_for_each_wave", wav[:, 0:3])):
        assert np.array_equal(got[:, 0], box["visited"]), f"{name}: points visited"
        assert np.array_equal(got[:, 1], box["sum"]), f"{name}: sum of the visited indices"
        assert np.array_equal(got[:, 2], box["xor"]), f"{name}: xor of the visited indices"
    assert np.array_equal(thr[:, 1], full), "grid_radius_count: the full count"
    assert np.array_equal(thr[:, 0], np.minimum(full, stop_at)), f"grid_radius_count: stopped at {stop_at}"
    assert np.array_equal(thr[:, 2], R.bits(box["min_d2"])), "grid_nearest: the minimum over the box population"
    below = brute["min_d2"] < case.r2
    if case.name != "lost neighbour":
        assert np.array_equal(thr[below, 2], R.bits(brute["min_d2"])[below]), "grid_nearest: brute force's minimum where it is below r2"
    best, ids = R._min_and_id(brute["d2"], inside, case.r2)
    if case.name != "lost neighbour":
        assert np.array_equal(ids, brute["id"]) and np.array_equal(R.bits(best), R.bits(brute["id_d2"]))
    assert np.array_equal(thr[:, 3], ids), "grid_nearest_id: id (strict <, the smaller index among equals, kGridNone without one)"
    assert np.array_equal(thr[:, 4], R.bits(best)), "grid_nearest_id: d2 (r2 without one)"
    assert np.array_equal(wav[:, 3], thr[:, 1]) and np.array_equal(wav[:, 3], full), "wave walk: count of d2 < r2"
    assert np.array_equal(wav[:, 4], thr[:, 2]), "wave walk: wave_min of d2"
    assert len(thr) == m and len(wav) == m


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_point_grid_against_the_reference(lp, case):
    e = cases.expected(case)
    for stop_at in cases.STOP_ATS:
        out = _run(lp, case, stop_at)
        _check_grid(out, case, e)
        _check_queries(out, case, e, stop_at)


def test_empty_and_tiny_answers(lp):
    """the answers the issue spells out: nothing at all for n = 0, the smaller index for an identical pair"""
    by_name = {c.name: c for c in cases.cases()}
    case = by_name["empty"]
    out = _run(lp, case, FULL)
    m = len(case.queries)
    assert np.array_equal(out["thread"][:, :2], np.zeros((m, 2), np.uint32))
    assert (out["thread"][:, 2] == R.INF_BITS).all() and (out["wave"][:, 4] == R.INF_BITS).all()
    assert (out["thread"][:, 3] == R.GRID_NONE).all() and (out["thread"][:, 4] == R.bits(case.r2)).all()
    assert not out["thread"][:, 5:].any() and not out["wave"][:, :4].any() and not out["cell_start"].any()
    case = by_name["identical pair"]
    out = _run(lp, case, FULL)
    assert out["thread"][5, 3] == 1 and out["thread"][5, 4] == 0 and out["thread"][5, 1] == 2        # query 5 is the pair's position
    case = by_name["five in one cell"]
    assert np.count_nonzero(np.diff(_run(lp, case, FULL)["cell_start"].astype(np.int64))) == 1


def test_point_grid_refuses_what_it_cannot_hold(lp):
    pts, q = np.full((4, 3), 0.5, F), np.full((2, 3), 0.5, F)
    lo, hi = np.zeros(3, F), np.ones(3, F)
    ok = dict(points=pts, lo=lo, hi=hi, cell_xy=0.25, cell_z=0.25, cap_cells=4096, queries=q, r_box=0.1, r2=0.01, stop_at=1)
    lp.selftest_point_grid(**ok)
    bad = [dict(points=np.zeros((K_MAX_POINTS + 1, 3), F)), dict(cap_cells=0), dict(r_box=np.inf), dict(r_box=np.nan), dict(r2=np.nan),
           dict(cell_xy=0.0), dict(stop_at=0), dict(lo=hi, hi=lo), dict(points=np.array([[0.5, np.nan, 0.5]], F)),
           dict(queries=np.array([[np.inf, 0.5, 0.5]], F)), dict(cap_cells=(1 << 22) + 1)]
    for change in bad:
        with pytest.raises(RolloutError) as err:
            lp.selftest_point_grid(**{**ok, **change})
        assert err.value.code == K.ERR_BAD_ARG, change
    # a null pointer with a nonzero count, for the points and for the queries
    cell, radius, grid = np.array([0.25, 0.25], F), np.array([0.1, 0.01], F), np.zeros(8, np.uint32)
    start, srt, thr, wav = np.zeros(4097, np.uint32), np.zeros((4, 4), np.uint32), np.zeros((2, 8), np.uint32), np.zeros((2, 5), np.uint32)
    for p_ptr, q_ptr in ((None, M.ptr(q)), (M.ptr(pts), None)):
        with pytest.raises(RolloutError) as err:
            lp._call("selftest_point_grid", p_ptr, 4, M.ptr(lo), M.ptr(hi), M.ptr(cell), 4096, q_ptr, 2, M.ptr(radius), 1, M.ptr(grid),
                     M.ptr(start), M.ptr(srt), M.ptr(thr), M.ptr(wav))
        assert err.value.code == K.ERR_BAD_ARG
    lp.selftest_point_grid(**ok)                                             # ... and the context is none the worse for it


K_MAX_POINTS = 1 << 16         # DDDMR_POINT_GRID_MAX_POINTS


def test_layers_refuse_a_static_cloud_wider_than_their_pad_covers(lp):
    """marking_create and depth_layer_create: a ground or map cloud wider than kSmallPadMaxExtent (2000 m) on an axis is a
    bad argument -- past 2048 m a search box widened by 1e-4 m can lose a neighbour (tests/test_point_grid_cpu.py)"""
    rng = np.random.default_rng(14)
    def cloud(length, axis):
        c = (rng.uniform(0.0, 1.0, (64, 3)) * np.array([5.0, 5.0, 0.2])).astype(F)
        c[0, axis], c[1, axis] = 0.0, length
        return c
    small = cloud(5.0, 0)
    for axis in (0, 1):
        for ground, static_map in ((cloud(2000.5, axis), small), (small, cloud(2000.5, axis))):
            with pytest.raises(RolloutError) as err:
                marking.MarkingLayer(lp, marking.shipped_config(max_markings=64), ground, static_map)
            assert err.value.code == K.ERR_BAD_ARG and "wider than 2000 m" in str(err.value)
            with pytest.raises(RolloutError) as err:
                depth_layer.DepthLayer(lp, depth_layer.shipped_config(max_markings=64), ground, static_map)
            assert err.value.code == K.ERR_BAD_ARG and "wider than 2000 m" in str(err.value)
    marking.MarkingLayer(lp, marking.shipped_config(max_markings=64), cloud(1999.5, 0), small)      # just inside the limit: accepted
