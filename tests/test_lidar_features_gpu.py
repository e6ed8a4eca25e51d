"""GPU parity of the lidar sweep features (set_lidar_sweep_features / get_lidar_sweep_segmented / get_lidar_sweep_features)
against the restatement of mcl_feature_node's feature half (tests/helpers/lidar_features_ref.py) on top of the sweep
restatement (tests/helpers/lidar_sweep_ref.py).

Everything is compared with assert_array_equal, floats on their bits: every sweep used here has zero fragile decisions
and zero tie-sensitive lists by the restatements' own reports (tests/test_lidar_features_cpu.py asserts both), and
everything else is the same IEEE operations in the same order on both sides.  No tolerance anywhere, except in the one
mcl_measure case, which keeps the tolerances tests/test_mcl_measure_gpu.py states for that entry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, localization, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lidar_sweep_ref as R  # noqa: E402
import lidar_sweep_cases as Cs  # noqa: E402
import lidar_features_ref as FR  # noqa: E402
import lidar_features_cases as FC  # noqa: E402
import mcl_measure_ref as MR  # noqa: E402
import mcl_measure_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

TBS = (0.1, 0.0, 0.6) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.05))
TGB = (1.0, -0.5, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.3))
WINDOW, HEIGHT = 8.0, 1.8
WHAT = ("sharp", "less sharp", "flat")


def planner(max_points=200_000):
    return LocalPlanner([configs.bench_theory("C2")], max_points=max_points)


def configure(lp, sid, c, **kw):
    args, kwargs = c.planner_args()
    kwargs.update(kw)
    lp.set_lidar_sweep_source(sid, *args, **kwargs)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def got_features(lp, sid, c):
    return lp.get_lidar_sweep_segmented(sid, c.V), [lp.get_lidar_sweep_features(sid, w) for w in range(3)]


def assert_features(got, f, T, what):
    seg, lists = got
    ref = f["seg"]
    print(f"{what}: {len(ref['range'])} segmented, {[len(l) for l in f['lists']]} sharp / less sharp / flat, edge breaks {f['edge_breaks']}, "
          f"flat breaks {f['flat_breaks']}, ep picks {f['ep_picks']}, slot 4 {f['slot4_pick']}, occlusion marks {f['n_occluded']}")
    assert f["n_tie_sensitive"] == 0, what                         # a condition on the input, checked on the restatement alone
    assert len(seg["range"]) == len(ref["range"]), what
    np.testing.assert_array_equal(bits(seg["xyz"]), bits(ref["xyz"]), err_msg=what + ": segmented xyz")
    np.testing.assert_array_equal(bits(seg["range"]), bits(ref["range"]), err_msg=what + ": segmented range")
    np.testing.assert_array_equal(seg["col"], ref["col"], err_msg=what + ": columns")
    np.testing.assert_array_equal(seg["ground"], ref["ground"].astype(np.uint8), err_msg=what + ": ground flags")
    np.testing.assert_array_equal(seg["start"], ref["start"], err_msg=what + ": start_ring_index")
    np.testing.assert_array_equal(seg["end"], ref["end"], err_msg=what + ": end_ring_index")
    for w in range(3):
        xyzr, idx = lists[w]
        np.testing.assert_array_equal(idx.astype(np.int64), f["lists"][w], err_msg=f"{what}: {WHAT[w]} seg_index order")
        want = FR.output(ref, f["lists"][w], T)
        np.testing.assert_array_equal(bits(xyzr[:, :3]), bits(want[:, :3]), err_msg=f"{what}: {WHAT[w]} xyz")
        np.testing.assert_array_equal(bits(xyzr[:, 3]), bits(want[:, 3]), err_msg=f"{what}: {WHAT[w]} ring")


# ---- 1. parity, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.PARITY)
def test_features_match_the_node_bit_for_bit(name):
    """4 x 8, 16 x 64 (ground_scan_index 0 / 7 / 15, mount 0 and 0.2), 16 x 440, 16 x 1000, the 16 x 2000 image (both breaks,
    column jumps) and 64 x 2048 (most rings, longest sixths); identity T_out, then the node's"""
    c, raw, ref, f = FC.case(name)
    assert ref["n_fragile"] == 0
    with planner() as lp:
        configure(lp, 0, c)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)
        n_seg = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)[0]
        assert n_seg == len(ref["cloud"])
        assert_features(got_features(lp, 0, c), f, FR.identity_T(), name)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF, T_out=FR.node_T())
        lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        assert_features(got_features(lp, 0, c), f, FR.node_T(), name + ", the node's T_out")


@pytest.mark.parametrize("name", sorted(FC.hand_cases()))
def test_hand_derived_answers_through_the_device(name):
    h = FC.hand_cases()[name]
    c, raw, ref = FC.hand_sweep(name)
    f = FR.features(ref, c, h["edge"], h["surf"])
    assert ref["n_fragile"] == 0
    with planner() as lp:
        configure(lp, 1, c)
        lp.set_lidar_sweep_features(1, h["edge"], h["surf"])
        lp.set_lidar_sweep(1, raw, TBS, TGB, WINDOW, HEIGHT)
        got = got_features(lp, 1, c)
    assert len(got[0]["range"]) == h["n_seg"]
    for w in range(3):
        assert got[1][w][1].tolist() == h["expect"][w], (name, WHAT[w])          # the answer derived by hand
    assert_features(got, f, FR.identity_T(), name)


# ---- 2. repeatability, double buffering -------------------------------------------------------------------------------------
def test_the_same_sweep_twice_gives_the_same_features():
    c, raw, ref, f = FC.case("16x440-g7-m0.0")
    other = FC.case("16x440-g7-m0.0")[1][::-1]
    with planner() as lp:
        configure(lp, 0, c)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)
        lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        first = got_features(lp, 0, c)
        assert_features(first, f, FR.identity_T(), "first")
        for what, data in (("again", raw), ("another sweep", other), ("the first again", raw)):
            lp.set_lidar_sweep(0, data, TBS, TGB, WINDOW, HEIGHT)
            got = got_features(lp, 0, c)
            if data is raw:
                for k in first[0]:
                    np.testing.assert_array_equal(got[0][k].view(np.uint8), first[0][k].view(np.uint8), err_msg=f"{what}: {k}")
                for w in range(3):
                    for a, b in zip(got[1][w], first[1][w]):
                        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{what}: {WHAT[w]}")
            else:
                r2 = R.stage_one(data, c)
                assert_features(got, FR.features(r2, c, FC.EDGE, FC.SURF), FR.identity_T(), what)


def test_a_refused_sweep_leaves_the_previous_features_in_place():
    c, raw, ref, _ = FC.case("16x440-g7-m0.0")
    with np.errstate(invalid="ignore"):
        small = np.ascontiguousarray(raw[raw[:, 0] > 0])              # the half of the scene in front: fewer observation points
    r_small = R.stage_one(small, c)
    f_small = FR.features(r_small, c, FC.EDGE, FC.SURF)
    assert r_small["n_fragile"] == 0 and f_small["n_tie_sensitive"] == 0 and all(len(l) > 0 for l in f_small["lists"])
    with planner() as lp:
        configure(lp, 0, c)
        n_full = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)[1]
    with planner(max_points=n_full - 1) as lp:
        configure(lp, 0, c)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)
        seg, lists = got_features(lp, 0, c)                         # before the first sweep: nothing
        assert len(seg["range"]) == 0 and all(len(l[1]) == 0 for l in lists)
        assert seg["start"].tolist() == [4] * c.V and seg["end"].tolist() == [-6] * c.V
        lp.set_lidar_sweep(0, small, TBS, TGB, WINDOW, HEIGHT)
        first = got_features(lp, 0, c)
        assert_features(first, f_small, FR.identity_T(), "the small sweep")
        with pytest.raises(RolloutError) as e:
            lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)     # the aggregate is over capacity
        assert e.value.code == K.ERR_CAPACITY
        assert_features(got_features(lp, 0, c), f_small, FR.identity_T(), "after the refused sweep")
        lp.set_lidar_sweep(0, small, TBS, TGB, WINDOW, HEIGHT)
        assert_features(got_features(lp, 0, c), f_small, FR.identity_T(), "the small sweep again")


# ---- 3. off means off ---------------------------------------------------------------------------------------------------------
def _refused(code, fn, *a, **kw):
    with pytest.raises(RolloutError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, code, str(e.value))


def _stage_one(lp, c, raw):
    counts = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
    rng, lab, gnd = lp.get_lidar_sweep_image(0, c.V, c.H)
    return counts, rng, lab, gnd, lp.get_lidar_sweep_cloud(0), lp.get_cloud()


def _assert_stage_one(got, ref, want_counts, want_agg, what):
    """tests/test_lidar_sweep_gpu.py's stage-one comparison, and the feed's counts and aggregate"""
    counts, rng, lab, gnd, cloud, agg = got
    np.testing.assert_array_equal(bits(rng), bits(ref["range"]), err_msg=what + ": range image")
    np.testing.assert_array_equal(gnd, ref["ground"], err_msg=what + ": ground mask")
    np.testing.assert_array_equal(lab, ref["label"], err_msg=what + ": labels")
    assert counts[0] == len(ref["cloud"]) == len(cloud), what
    np.testing.assert_array_equal(bits(cloud), bits(ref["cloud"]), err_msg=what + ": output cloud")
    if want_counts is not None:
        assert counts == want_counts, what
        assert len(agg) == len(want_agg), what
        key = lambda p: p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]
        np.testing.assert_allclose(key(agg[:, :3]), key(want_agg[:, :3]), rtol=0, atol=1e-5, err_msg=what + ": aggregate")


def test_features_off_answer_state_and_leave_the_sweep_as_it_was():
    c, raw, ref, f = FC.case("16x440-g7-m0.0")
    with planner() as lp:
        _refused(K.ERR_STATE, lp.set_lidar_sweep_features, 0, FC.EDGE, FC.SURF)            # not a sweep source
        _refused(K.ERR_STATE, lp.get_lidar_sweep_features, 0, 1)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_segmented, 0, c.V)
        configure(lp, 0, c)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_features, 0, 1)                           # a sweep source, features off
        _refused(K.ERR_STATE, lp.get_lidar_sweep_segmented, 0, c.V)
        off = _stage_one(lp, c, raw)
        _assert_stage_one(off, ref, None, None, "features never on")
        _refused(K.ERR_STATE, lp.get_lidar_sweep_features, 0, 2)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)
        on = _stage_one(lp, c, raw)
        _assert_stage_one(on, ref, off[0], off[5], "features on")
        assert_features(got_features(lp, 0, c), f, FR.identity_T(), "features on")
        lp.set_lidar_sweep_features(0, enable=False)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_features, 0, 1)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_segmented, 0, c.V)
        _assert_stage_one(_stage_one(lp, c, raw), ref, off[0], off[5], "features off again")
        lp.set_lidar_sweep_features(0, enable=False)                                       # off twice is fine
        # on again: nothing until the next sweep
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)
        seg, lists = got_features(lp, 0, c)
        assert len(seg["range"]) == 0 and all(len(l[1]) == 0 for l in lists)
        lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        assert_features(got_features(lp, 0, c), f, FR.identity_T(), "on again")
        # re-configuring the sweep source turns them off
        configure(lp, 0, c)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_features, 0, 1)
        _assert_stage_one(_stage_one(lp, c, raw), ref, off[0], off[5], "after re-configuring")


def test_argument_refusals_change_nothing():
    c, raw, ref, f = FC.case("16x64-g7-m0.0")
    T = FR.identity_T()
    with planner() as lp:
        configure(lp, 0, c)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)
        lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        for bad in (dict(edge_threshold=-0.1), dict(surf_threshold=-1e-9), dict(edge_threshold=float("nan")), dict(surf_threshold=float("inf")),
                    dict(flags=1)):
            kw = dict(edge_threshold=0.3, surf_threshold=0.3, flags=0)
            kw.update(bad)
            _refused(K.ERR_BAD_ARG, lp.set_lidar_sweep_features, 0, **kw)
        for i, v in ((0, float("nan")), (7, float("inf")), (11, -float("inf"))):
            Tb = T.copy()
            Tb.reshape(-1)[i] = v
            _refused(K.ERR_BAD_ARG, lp.set_lidar_sweep_features, 0, 0.3, 0.3, T_out=Tb)
        _refused(K.ERR_BAD_ARG, lp.set_lidar_sweep_features, 7, FC.EDGE, FC.SURF)
        _refused(K.ERR_BAD_ARG, lp.get_lidar_sweep_features, 0, 3)
        _refused(K.ERR_BAD_ARG, lp.get_lidar_sweep_features, 0, -1)
        # the refused calls changed neither the parameters nor the results
        assert_features(got_features(lp, 0, c), f, T, "after the refusals")
        lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        assert_features(got_features(lp, 0, c), f, T, "a sweep after the refusals")
        # a capacity below the count is refused; NULL outputs only report it
        cnt = C.c_size_t(0)
        assert lp._lib.dddmr_rollout_get_lidar_sweep_features(lp._ctx, 0, 1, None, None, 0, C.byref(cnt)) == K.OK and cnt.value == len(f["lists"][1]) > 1
        buf = np.zeros((cnt.value, 4), np.float32)
        assert lp._lib.dddmr_rollout_get_lidar_sweep_features(lp._ctx, 0, 1, buf.ctypes.data_as(C.c_void_p), None, cnt.value - 1,
                                                              C.byref(cnt)) == K.ERR_CAPACITY
        assert not buf.any()


# ---- 4. the point of it: the device's lists are mcl_measure's observation -----------------------------------------------------
def test_mcl_measure_takes_the_device_feature_lists():
    c, raw, ref, f = FC.case("16x440-g7-m0.0")
    parts, _, _ = MC.case("n64-o1x0")
    T = FR.node_T()
    want_flat, want_ls = FR.output(f["seg"], f["lists"][FR.FLAT], T), FR.output(f["seg"], f["lists"][FR.LESS_SHARP], T)
    # particles by rejection on the restatements alone: no fragile or tied decision for this observation
    r_all = MR.measure(MC.CFG, parts["map"], parts["ground"], parts["normals"], want_flat[:, :3], want_ls, parts["states"])
    states = parts["states"][(r_all["n_fragile"] == 0) & (r_all["n_tied"] == 0)][:16]
    assert len(states) >= 8
    with planner() as lp:
        configure(lp, 0, c)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF, T_out=T)
        lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        flat, ls = lp.get_lidar_sweep_features(0, FR.FLAT)[0], lp.get_lidar_sweep_features(0, FR.LESS_SHARP)[0]
        np.testing.assert_array_equal(bits(flat), bits(want_flat))
        np.testing.assert_array_equal(bits(ls), bits(want_ls))
        pm = localization.ParticleMeasure(lp, localization.shipped_config(
            match_dist_min=MC.CFG.match_dist_min, match_dist_flat=MC.CFG.match_dist_flat, radius_of_ground_search=MC.CFG.radius_of_ground_search,
            threshold_for_trusted_ground=MC.CFG.threshold_for_trusted_ground, max_map_points=20000, max_ground_points=20000, max_particles=64,
            max_observation_points=2000, max_ground_neighbours=512))
        pm.set_map(parts["map"], parts["ground"], parts["normals"])
        like, qual = pm.measure(np.ascontiguousarray(flat[:, :3]), ls, states)
        t = pm.terms(len(states))
    want = MR.measure(MC.CFG, parts["map"], parts["ground"], parts["normals"], flat[:, :3], ls, states)
    assert int(want["n_fragile"].sum()) == 0 and int(want["n_tied"].sum()) == 0
    print(f"mcl_measure on {len(flat)} flat + {len(ls)} less sharp device points, {len(states)} particles, matches {want['n_match'].tolist()}")
    np.testing.assert_array_equal(t["healthy"], want["healthy"])
    np.testing.assert_array_equal(t["n_match"], want["n_match"])
    np.testing.assert_array_equal(t["n_ground"], want["n_ground"])
    np.testing.assert_array_equal(bits(t["score"]), bits(want["score"]))
    np.testing.assert_array_equal(bits(qual), bits(want["quality"]))
    ulp = lambda a, b: np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))
    assert ulp(t["pos_weight"], want["pos_weight"]).max() <= 1 and ulp(like, want["likelihood"]).max() <= 2     # test_mcl_measure_gpu.py's
