"""GPU parity of the lidar sweep association (set_lidar_sweep_association and its getters, sweep_association.SweepAssociation)
against the restatement of the rest of LeGO-LOAM's feature-node front half (tests/helpers/sweep_association_ref.py) on top
of the sweep and feature restatements.

Compared ON BITS: segment indices, counts and the order of all four lists, i0, the outlier cloud entirely, and x y z of
every point in both frames (the association frame is the segmented point's own floats; through T_out it is the double
multiply-add the feature test compares on bits too).  Every case keeps the margins tests/test_sweep_association_cpu.py
asserts on the restatements alone, so no decision depends on the last place of an atan2f.

The intensities and the three orientations go through atan2f, which the device and the C library may round differently.
Their bound is DERIVED, not measured: one unit in the last place of atan2f at pi, u = 2^-22 (the spacing of float32 in
[2, 4), where |atan2f| <= pi lies), carried through the reference's expressions.  A float rounding of a value below 16
(every angle here is below 5 pi) moves a perturbed value by at most the perturbation plus one spacing there, 4 u:
  start = -atan2f                                        E_start = u
  end   = float(-atan2f + 2 pi), one more +- 2 pi        E_end   = u + 4 u + 4 u = 9 u
  diff  = end - start (float)                            E_diff  = E_start + E_end + spacing(diff)
  ori   = -atan2f, up to two float(ori +- 2 pi)          E_ori   = 9 u
  num   = ori - start (float)                            E_num   = E_ori + E_start + spacing(num)
  rel   = num / diff (float)                             E_rel   = E_num / |diff| + |num| E_diff / diff^2 + spacing(rel)
  intensity = float(ring + scan_period * rel)            E_int   = scan_period * E_rel + spacing(intensity)
and for a less-flat voxel of m summands, float sums in the same order on both sides, each add rounding once:
  E_avg = (sum E_int + m spacing(m max|intensity|)) / m + spacing(avg).
With scan_period 0 the intensity is the ring, exactly.  A case that needed more than this would be a finding about the
derivation (DESIGN.md 4a-2 records what an MI355X gave), not a reason to widen it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, localization, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from dddmr_navigation_amd.sweep_association import SweepAssociation
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lidar_features_ref as FR  # noqa: E402
import lidar_features_cases as FC  # noqa: E402
import mcl_measure_cases as MC  # noqa: E402
import mcl_observation_cases as OC  # noqa: E402
import sweep_association_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
U = 2.0 ** -22
TBS = (0.1, 0.0, 0.6) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.05))
TGB = (1.0, -0.5, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.3))
WINDOW, HEIGHT = 8.0, 1.8
WHAT = ("sharp", "less sharp", "flat", "less flat")


def planner(max_points=200_000):
    return LocalPlanner([configs.bench_theory("C2")], max_points=max_points)


def configure(lp, sid, k, T_out=None):
    args, kwargs = k["config"].planner_args()
    lp.set_lidar_sweep_source(sid, *args, **kwargs)
    lp.set_lidar_sweep_features(sid, k["edge"], k["surf"], T_out=T_out)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def sp(x):
    return np.spacing(np.abs(np.asarray(x, f32))).astype(f64)


def bounds(want, scan_period):
    """(E_start, E_end, E_diff, E_int per segmented point) as the module docstring derives them"""
    start, end, diff = f64(want["start"]), f64(want["end"]), f64(want["diff"])
    e_diff = U + 9 * U + sp(diff)
    t = want["times"].astype(f64)
    if len(t) == 0 or scan_period == 0.0:
        return U, 9 * U, e_diff, np.zeros(len(t))
    rel = want["rel"].astype(f64)
    num = rel * diff
    e_num = 9 * U + U + sp(num)
    e_rel = e_num / abs(diff) + np.abs(num) * e_diff / diff ** 2 + sp(rel)
    return U, 9 * U, e_diff, scan_period * e_rel + sp(t)


def got_all(sa):
    return dict(orientation=sa.orientation(), times=sa.times(), clouds=[[sa.cloud(w, fr) for w in range(4)] for fr in range(2)],
                outliers=sa.outliers())


def assert_association(got, want, scan_period, what):
    e_start, e_end, e_diff, e_int = bounds(want, scan_period)
    start, end, diff, i0 = got["orientation"]
    print(f"{what}: i0 {want['i0']} of {len(want['times'])}, orientation {want['start']:.6f} {want['end']:.6f} {want['diff']:.6f} "
          f"(device off by {abs(f64(start) - f64(want['start'])) / U:.2f} / {abs(f64(end) - f64(want['end'])) / U:.2f} / "
          f"{abs(f64(diff) - f64(want['diff'])) / U:.2f} u), less flat {want['ring_voxels']} of {want['ring_candidates']}, "
          f"{len(want['outliers'])} outliers")
    assert i0 == want["i0"], what
    assert abs(f64(start) - f64(want["start"])) <= e_start and abs(f64(end) - f64(want["end"])) <= e_end, what
    assert abs(f64(diff) - f64(want["diff"])) <= e_diff, what
    assert len(got["times"]) == len(want["times"]), what
    err = np.abs(got["times"].astype(f64) - want["times"].astype(f64))
    if len(err):
        worst = int(np.argmax(err - e_int))
        print(f"{what}: times off by at most {err.max():.3e}, closest to its bound at {worst}: {err[worst]:.3e} of {e_int[worst]:.3e}")
    assert (err <= e_int).all(), what
    np.testing.assert_array_equal(bits(got["outliers"]), bits(want["outliers"]), err_msg=what + ": outliers")
    for frame in range(2):
        for w in range(4):
            (xyzi, idx), (ref, ref_idx) = got["clouds"][frame][w], want["clouds"][frame][w]
            tag = f"{what}: {WHAT[w]}, frame {frame}"
            np.testing.assert_array_equal(idx.astype(np.int64), ref_idx, err_msg=tag + ": seg_index order")
            np.testing.assert_array_equal(bits(xyzi[:, :3]), bits(ref[:, :3]), err_msg=tag + ": xyz")
            if w < 3:
                tol = e_int[ref_idx] if len(ref_idx) else np.zeros(0)
            else:
                tol = want["less_flat_bound"](e_int)
            assert (np.abs(xyzi[:, 3].astype(f64) - ref[:, 3].astype(f64)) <= tol).all(), tag + ": intensity"


def expected(name, scan_period, node_T=False):
    """the restatement's answer, and the less-flat bound as a function of the per-point bounds"""
    want = dict(AC.expected(name, scan_period, node_T))

    def less_flat_bound(e_int):
        out = []
        for m, avg in zip(want["voxel_members"], want["clouds"][0][3][0][:, 3]):
            big = len(m) * float(np.abs(want["times"][m]).max())
            out.append((e_int[m].sum() + len(m) * sp(big)) / len(m) + sp(avg))
        return np.asarray(out, f64)
    want["less_flat_bound"] = less_flat_bound
    return want


def run(name, scan_period, node_T=False):
    k = AC.case(name)
    T = FR.node_T() if node_T else None
    with planner() as lp:
        configure(lp, 0, k, T)
        sa = SweepAssociation(lp, 0, scan_period)
        lp.set_lidar_sweep(0, k["raw"], TBS, TGB, WINDOW, HEIGHT)
        return got_all(sa)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan_period", AC.PERIODS)
@pytest.mark.parametrize("name", AC.NAMES)
def test_association_matches_the_node(name, scan_period):
    """every shape of tests/helpers/sweep_association_cases.py at both scan periods, identity T_out"""
    assert_association(run(name, scan_period), expected(name, scan_period), scan_period, f"{name}, period {scan_period}")


@pytest.mark.parametrize("name", ("counts", "16x64-g7-m0.0"))
def test_the_four_clouds_through_the_nodes_T_out(name):
    assert_association(run(name, 0.1, node_T=True), expected(name, 0.1, node_T=True), 0.1, name + ", the node's T_out")


def test_the_lists_are_the_features_lists_with_times():
    """frame 1 of sharp, less sharp and flat is get_lidar_sweep_features' x y z bit for bit, in its order, with the point
    time where it has the ring; int(intensity) is that ring"""
    k = AC.case("16x440-g7-m0.0")
    with planner() as lp:
        configure(lp, 0, k, FR.node_T())
        sa = SweepAssociation(lp, 0, 0.1)
        lp.set_lidar_sweep(0, k["raw"], TBS, TGB, WINDOW, HEIGHT)
        times = sa.times()
        for w in range(3):
            xyzr, idx = lp.get_lidar_sweep_features(0, w)
            xyzi, idx2 = sa.cloud(w, 1)
            assert len(idx) > 0
            np.testing.assert_array_equal(idx, idx2)
            np.testing.assert_array_equal(bits(xyzr[:, :3]), bits(xyzi[:, :3]))
            np.testing.assert_array_equal(bits(xyzi[:, 3]), bits(times[idx]))
            np.testing.assert_array_equal(bits(sa.cloud(w, 0)[0][:, 3]), bits(times[idx]))


# ---- 2. double buffering, state --------------------------------------------------------------------------------------------
def _refused(code, fn, *a, **kw):
    with pytest.raises(RolloutError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, code, str(e.value))


def _same(a, b, what):
    """two got_all() results, byte for byte"""
    assert a["orientation"] == b["orientation"], what
    np.testing.assert_array_equal(bits(a["times"]), bits(b["times"]), err_msg=what)
    np.testing.assert_array_equal(bits(a["outliers"]), bits(b["outliers"]), err_msg=what)
    for frame in range(2):
        for w in range(4):
            for x, y in zip(a["clouds"][frame][w], b["clouds"][frame][w]):
                np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=what)


def test_a_refused_sweep_keeps_the_previous_result_and_sweeps_repeat():
    k = AC.case("16x440-g7-m0.0")
    raw = k["raw"]
    with np.errstate(invalid="ignore"):
        small = np.ascontiguousarray(raw[raw[:, 0] > 0])
    with planner() as lp:
        configure(lp, 0, k)
        n_full = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)[1]
    with planner(max_points=n_full - 1) as lp:
        configure(lp, 0, k)
        sa = SweepAssociation(lp, 0, 0.1)
        before = got_all(sa)                                           # before the first sweep: nothing, zeros
        assert before["orientation"] == (0.0, 0.0, 0.0, 0) and len(before["times"]) == 0 and len(before["outliers"]) == 0
        assert all(len(before["clouds"][fr][w][1]) == 0 for fr in range(2) for w in range(4))
        lp.set_lidar_sweep(0, small, TBS, TGB, WINDOW, HEIGHT)
        first = got_all(sa)
        assert len(first["times"]) > 100 and len(first["clouds"][0][3][1]) > 50
        _refused(K.ERR_CAPACITY, lp.set_lidar_sweep, 0, raw, TBS, TGB, WINDOW, HEIGHT)      # the aggregate is over capacity
        _same(got_all(sa), first, "after the refused sweep")
        lp.set_lidar_sweep(0, small[::-1], TBS, TGB, WINDOW, HEIGHT)   # another sweep in between: other ends, other times
        other = got_all(sa)
        assert other["orientation"] != first["orientation"]
        lp.set_lidar_sweep(0, small, TBS, TGB, WINDOW, HEIGHT)
        _same(got_all(sa), first, "the same sweep again")


def _features(lp, c):
    return lp.get_lidar_sweep_segmented(0, c.V), [lp.get_lidar_sweep_features(0, w) for w in range(3)], lp.get_lidar_sweep_cloud(0), \
        lp.get_lidar_sweep_image(0, c.V, c.H), lp.get_cloud()


def _assert_same_features(a, b, what):
    for key in a[0]:
        np.testing.assert_array_equal(a[0][key].view(np.uint8), b[0][key].view(np.uint8), err_msg=f"{what}: {key}")
    for la, lb in zip(a[1], b[1]):
        for x, y in zip(la, lb):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=what)
    np.testing.assert_array_equal(a[2].view(np.uint8), b[2].view(np.uint8), err_msg=what)
    for x, y in zip(a[3], b[3]):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=what)
    # the aggregate: the feed's table emits in no fixed order and sums with atomics, so it is compared as
    # tests/test_lidar_features_gpu.py compares it between two sweeps of the parent's own code
    key = lambda p: p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]
    assert len(a[4]) == len(b[4]), what
    np.testing.assert_allclose(key(a[4][:, :3]), key(b[4][:, :3]), rtol=0, atol=1e-5, err_msg=what + ": aggregate")


def test_off_on_off_leaves_everything_else_byte_equal():
    k = AC.case("16x440-g7-m0.0")
    c, raw = k["config"], k["raw"]
    with planner() as lp:
        _refused(K.ERR_STATE, SweepAssociation, lp, 0)                                     # not a sweep source
        src_args, src_kwargs = c.planner_args()
        lp.set_lidar_sweep_source(0, *src_args, **src_kwargs)
        _refused(K.ERR_STATE, SweepAssociation, lp, 0)                                     # a sweep source, features off
        lp.set_lidar_sweep_features(0, k["edge"], k["surf"])
        counts_off = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        off = _features(lp, c)
        for name, args in (("get_lidar_sweep_times", (None, 0)), ("get_lidar_sweep_outliers", (None, 0)),
                           ("get_lidar_sweep_association", (3, 0, None, None, 0))):
            n = C.c_size_t(7)
            assert getattr(lp._lib, "dddmr_rollout_" + name)(lp._ctx, 0, *args, C.byref(n)) == K.ERR_STATE and n.value == 7
        assert lp._lib.dddmr_rollout_get_lidar_sweep_orientation(lp._ctx, 0, None, None) == K.ERR_STATE
        sa = SweepAssociation(lp, 0, 0.1)
        assert len(sa.times()) == 0 and len(sa.cloud(3)[1]) == 0 and len(sa.cloud(1, 1)[1]) == 0    # it holds from the NEXT sweep
        counts_on = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        assert counts_on == counts_off
        _assert_same_features(_features(lp, c), off, "association on")
        assert_association(got_all(sa), expected("16x440-g7-m0.0", 0.1), 0.1, "on")
        sa.close()
        _refused(K.ERR_STATE, sa.times)
        _refused(K.ERR_STATE, sa.orientation)
        assert lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT) == counts_off
        _assert_same_features(_features(lp, c), off, "association off again")
        sa.close()                                                                         # twice is fine
        # switching the features off, and re-configuring the source, switch it off
        sa = SweepAssociation(lp, 0, 0.0)
        lp.set_lidar_sweep_features(0, enable=False)
        _refused(K.ERR_STATE, sa.outliers)
        lp.set_lidar_sweep_features(0, k["edge"], k["surf"])
        _refused(K.ERR_STATE, sa.outliers)
        sa = SweepAssociation(lp, 0, 0.0)
        lp.set_lidar_sweep_source(0, *src_args, **src_kwargs)
        _refused(K.ERR_STATE, sa.outliers)


def test_argument_refusals_change_nothing():
    k = AC.case("16x64-g7-m0.0")
    with planner() as lp:
        configure(lp, 0, k)
        sa = SweepAssociation(lp, 0, 0.1)
        lp.set_lidar_sweep(0, k["raw"], TBS, TGB, WINDOW, HEIGHT)
        first = got_all(sa)
        for bad in (-0.1, -1e-300, float("nan"), float("inf"), -float("inf")):
            _refused(K.ERR_BAD_ARG, SweepAssociation, lp, 0, bad)
        _refused(K.ERR_BAD_ARG, SweepAssociation, lp, 7)
        for which, frame in ((4, 0), (-1, 0), (0, 2), (3, -1)):
            _refused(K.ERR_BAD_ARG, sa.cloud, which, frame)
        _refused(K.ERR_BAD_ARG, lp.get_lidar_sweep_features, 0, 3)                         # less flat has a getter of its own
        _same(got_all(sa), first, "after the refusals")
        lp.set_lidar_sweep(0, k["raw"], TBS, TGB, WINDOW, HEIGHT)
        _same(got_all(sa), first, "a sweep after the refusals: the period is still 0.1")
        # NULL outputs only report the count; a capacity below it is refused and writes nothing
        lib, n = lp._lib, C.c_size_t(0)
        assert lib.dddmr_rollout_get_lidar_sweep_association(lp._ctx, 0, 3, 0, None, None, 0, C.byref(n)) == K.OK
        assert n.value == len(first["clouds"][0][3][1]) > 1
        buf = np.zeros((n.value, 4), f32)
        assert lib.dddmr_rollout_get_lidar_sweep_association(lp._ctx, 0, 3, 0, buf.ctypes.data_as(C.c_void_p), None, n.value - 1,
                                                             C.byref(n)) == K.ERR_CAPACITY and not buf.any()
        assert lib.dddmr_rollout_get_lidar_sweep_times(lp._ctx, 0, None, 0, C.byref(n)) == K.OK and n.value == len(first["times"])
        assert lib.dddmr_rollout_get_lidar_sweep_times(lp._ctx, 0, buf.ctypes.data_as(C.c_void_p), 1, C.byref(n)) == K.ERR_CAPACITY
        assert lib.dddmr_rollout_get_lidar_sweep_outliers(lp._ctx, 0, None, 0, C.byref(n)) == K.OK and n.value == len(first["outliers"]) > 1
        assert lib.dddmr_rollout_get_lidar_sweep_outliers(lp._ctx, 0, buf.ctypes.data_as(C.c_void_p), 1, C.byref(n)) == K.ERR_CAPACITY
        assert not buf.any()
        # a new period on a source that has it on holds from the next sweep
        SweepAssociation(lp, 0, 0.0)
        _same(got_all(sa), first, "a new period, before the next sweep")
        lp.set_lidar_sweep(0, k["raw"], TBS, TGB, WINDOW, HEIGHT)
        np.testing.assert_array_equal(sa.times(), k["f"]["seg"]["row"].astype(f32))


def test_mcl_prepare_from_sweep_is_byte_equal_with_the_association_on():
    k = AC.case("16x440-g7-m0.0")
    snaps = []
    for on in (False, True):
        with planner() as lp:
            configure(lp, 0, k)
            sa = SweepAssociation(lp, 0, 0.1) if on else None
            lp.set_lidar_sweep(0, k["raw"], TBS, TGB, WINDOW, HEIGHT)
            c = MC.CFG
            pm = localization.ParticleMeasure(lp, localization.shipped_config(
                match_dist_min=c.match_dist_min, match_dist_flat=c.match_dist_flat, radius_of_ground_search=c.radius_of_ground_search,
                threshold_for_trusted_ground=c.threshold_for_trusted_ground, max_map_points=20000, max_ground_points=20000, max_particles=64,
                max_observation_points=2000, max_ground_neighbours=512))
            pm.configure_observation(localization.shipped_observation_config(
                euc_cluster_distance=OC.TOL, euc_cluster_min_size=OC.MIN_SIZE, max_flat_points=400, max_less_sharp_points=1600))
            st = pm.prepare_from_sweep(0, OC.T_B2S)
            snaps.append((bytes(st)[: K.MclObservationStats.launches.offset], [a.tobytes() for a in pm.observation()]))
            assert sa is None or len(sa.times()) > 0
    assert snaps[0] == snaps[1] and sum(len(b) for b in snaps[0][1]) > 0
