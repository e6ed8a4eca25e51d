"""GPU parity of the particle filter's lidar likelihood (dddmr_rollout_mcl_*, dddmr_navigation_amd.localization) against
the NumPy restatement of mcl_3dl's measure() (tests/helpers/mcl_measure_ref.py, pinned on bits to the reference's own
code compiled against library stand-ins: tests/test_mcl_measure_pin_cpu.py; the device against that build's recorded
answers: tests/test_mcl_measure_pin_gpu.py).

For EVERY particle of every case: score_like, the match count, the ground count, the branch and the quality are
compared on bits (the same IEEE float operations in the same order on both sides); pos_weight within 1 float ulp (its
double chain goes through acos / sin / cos / asin / atan2, a few double ulp apart between the device's and the host's
libm, and is rounded to float once; the cases hold no decision of that chain within 1e-9 of its branch value, see
tests/test_mcl_measure_cpu.py); likelihood = score * pos_weight within 2 float ulp (a 1 ulp weight times an exact
score, rounded once)."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, localization, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcl_measure_ref as R  # noqa: E402
import mcl_measure_cases as Cs  # noqa: E402

pytestmark = pytest.mark.gpu


def config(cfg=Cs.CFG, **kw):
    d = dict(match_dist_min=cfg.match_dist_min, match_dist_flat=cfg.match_dist_flat, radius_of_ground_search=cfg.radius_of_ground_search,
             threshold_for_trusted_ground=cfg.threshold_for_trusted_ground, max_map_points=20000, max_ground_points=20000,
             max_particles=512, max_observation_points=2000, max_ground_neighbours=512)
    d.update(kw)
    return localization.shipped_config(**d)


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:      # (the C2 scene's cloud, for the pending tick)
        yield p


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulps(a, b):
    """distance in float32 steps between finite, same-signed or zero values"""
    ia, ib = bits(a).astype(np.int64), bits(b).astype(np.int64)
    ia, ib = np.where(ia < 0x80000000, ia, 0x80000000 - ia), np.where(ib < 0x80000000, ib, 0x80000000 - ib)
    return np.abs(ia - ib)


def run(pm, parts):
    pm.set_map(parts["map"], parts["ground"], parts["normals"])
    like, qual = pm.measure(parts["flat"], parts["ls"], parts["states"])
    return like, qual, pm.terms(len(parts["states"])), pm.last


def assert_parity(got, ref, what):
    like, qual, t, st = got
    assert int(ref["n_fragile"].sum()) == 0 and int(ref["n_tied"].sum()) == 0, what      # conditions on the input alone
    np.testing.assert_array_equal(t["healthy"], ref["healthy"], err_msg=what + ": branch")
    np.testing.assert_array_equal(t["n_ground"], ref["n_ground"], err_msg=what + ": ground neighbours")
    np.testing.assert_array_equal(t["n_match"], ref["n_match"], err_msg=what + ": matches")
    np.testing.assert_array_equal(bits(t["score"]), bits(ref["score"]), err_msg=what + ": score_like")
    np.testing.assert_array_equal(bits(qual), bits(ref["quality"]), err_msg=what + ": quality")
    uw, ul = ulps(t["pos_weight"], ref["pos_weight"]), ulps(like, ref["likelihood"])
    print(f"{what}: {len(like)} particles, {int(ref['healthy'].sum())} on trusted ground; not bit-equal: "
          f"{int((uw != 0).sum())} weights (max {int(uw.max())} ulp), {int((ul != 0).sum())} likelihoods (max {int(ul.max())} ulp)")
    assert np.isfinite(t["pos_weight"]).all() and np.isfinite(like).all(), what
    assert uw.max() <= 1, (what, "pos_weight", int(uw.argmax()), t["pos_weight"][uw.argmax()], ref["pos_weight"][uw.argmax()])
    assert ul.max() <= 2, (what, "likelihood", int(ul.argmax()), like[ul.argmax()], ref["likelihood"][ul.argmax()])
    assert bits(st.quality_min) == bits(ref["quality_min"]) and bits(st.quality_max) == bits(ref["quality_max"]), what
    assert st.n_bad_states == ref["n_bad"] and st.n_over_capacity == 0 and st.max_ground_neighbours_seen == int(ref["n_ground"].max()), what


def refused(code, fn, *a):
    with pytest.raises(RolloutError) as e:
        fn(*a)
    assert e.value.code == code, (e.value.code, str(e.value))


@pytest.mark.parametrize("name", Cs.NAMES)
def test_every_particle_matches_the_restatement(lp, name):
    """N in {1, 64, 65, 300}, (n_flat, n_ls) in {(0,1), (1,0), (1,1), (64,65), (3,130), (40,200)}, ground neighbour counts
    0 / 5 / 6 / 64 / 65 / 300, a map of one point, an empty map, the scene shifted by (3000, -7000, 40) m, the largest
    observation the library takes (600 + 1400 points: 64 000 B of dynamic LDS), and the needles: one map point decides
    each particle's single match and sits in a chosen cell of the query's 2 x 2 x 2 candidate box, every cell of it taken
    (tests/test_mcl_measure_cpu.py asserts the cell indices), so a lost cell turns a count of 1 into 0"""
    parts, ref, _ = Cs.case(name)
    pm = localization.ParticleMeasure(lp, config())
    assert_parity(run(pm, parts), ref, name)
    if name == "needles":
        assert (ref["n_match"] == 1).all()                    # a lost cell would turn a 1 into a 0 above
    if name == "ground-counts":
        assert ref["n_ground"].tolist() == list(Cs.GROUND_COUNTS) and ref["healthy"].tolist() == [False, False, True, True, True, True]


def test_known_answers_through_the_device(lp):
    pm = localization.ParticleMeasure(lp, config())
    for name, cfg, parts, exp in Cs.known_answers():
        like, qual, t, st = run(pm, parts)
        got = dict(t, likelihood=like, quality=qual)
        for k, v in exp.items():
            want = np.asarray(v, dtype=got[k].dtype)
            if want.dtype == np.float32:
                np.testing.assert_array_equal(bits(got[k]), bits(want), err_msg=f"{name}: {k}")
            else:
                np.testing.assert_array_equal(got[k], want, err_msg=f"{name}: {k}")


def test_the_same_call_twice_gives_identical_bytes(lp):
    parts, ref, _ = Cs.case("n300-o64x65")
    pm = localization.ParticleMeasure(lp, config())
    a = run(pm, parts)
    b = run(pm, parts)
    c = (pm.measure(parts["flat"], parts["ls"], parts["states"]), pm.terms(300))           # without a set_map in between
    for x in (b, (c[0][0], c[0][1], c[1])):
        assert a[0].tobytes() == x[0].tobytes() and a[1].tobytes() == x[1].tobytes()
        assert all(a[2][k].tobytes() == x[2][k].tobytes() for k in a[2])


def test_set_map_swaps_and_a_refused_one_changes_nothing(lp):
    room, ref_room, _ = Cs.case("n64-o3x130")
    other, ref_other, _ = Cs.case("ground-counts")
    pm = localization.ParticleMeasure(lp, config(max_map_points=len(room["map"]), max_ground_points=len(room["ground"])))
    refused(K.ERR_STATE, pm.measure, room["flat"], room["ls"], room["states"])            # no map yet
    assert_parity(run(pm, room), ref_room, "first map")
    assert_parity(run(pm, other), ref_other, "second map")
    # the ground-counts observation against the room: the new map's answer, not the old one's
    pm.set_map(room["map"], room["ground"], room["normals"])
    mixed = R.measure(Cs.CFG, room["map"], room["ground"], room["normals"], other["flat"], other["ls"], other["states"])
    like, qual = pm.measure(other["flat"], other["ls"], other["states"])
    np.testing.assert_array_equal(bits(qual), bits(mixed["quality"]))
    np.testing.assert_array_equal(bits(pm.terms(len(qual))["score"]), bits(mixed["score"]))
    # beyond capacity: refused, and the room still answers
    big = np.concatenate([room["map"], room["map"][:1]])
    refused(K.ERR_CAPACITY, pm.set_map, big, room["ground"], room["normals"])
    refused(K.ERR_CAPACITY, pm.set_map, room["map"], np.concatenate([room["ground"], room["ground"][:1]]),
            np.concatenate([room["normals"], room["normals"][:1]]))
    bad = room["map"].copy()
    bad[7, 1] = np.nan
    refused(K.ERR_BAD_ARG, pm.set_map, bad, room["ground"], room["normals"])
    wide = room["map"].copy()                                  # wider than the search boxes' widening covers
    wide[7, 0] = wide[:, 0].min() + np.float32(4100.0)
    refused(K.ERR_BAD_ARG, pm.set_map, wide, room["ground"], room["normals"])
    wide[7, 0] = wide[:, 0].min() + np.float32(4000.0)
    pm.set_map(wide, room["ground"], room["normals"])
    pm.set_map(room["map"], room["ground"], room["normals"])
    like, qual = pm.measure(room["flat"], room["ls"], room["states"])
    assert_parity((like, qual, pm.terms(len(like)), pm.last), ref_room, "after the refused set_map calls")


def test_capacities_and_refusals(lp):
    parts, ref, _ = Cs.case("ground-counts")
    refused(K.ERR_BAD_ARG, localization.ParticleMeasure, lp, config(threshold_for_trusted_ground=-1))
    refused(K.ERR_BAD_ARG, localization.ParticleMeasure, lp, config(match_dist_min=0.0))
    refused(K.ERR_BAD_ARG, localization.ParticleMeasure, lp, config(radius_of_ground_search=float("nan")))
    refused(K.ERR_CAPACITY, localization.ParticleMeasure, lp, config(max_ground_neighbours=1025))
    refused(K.ERR_CAPACITY, localization.ParticleMeasure, lp, config(max_observation_points=2001))
    # a particle with 300 ground neighbours against max_ground_neighbours 299 fails the call; 300 is enough
    pm = localization.ParticleMeasure(lp, config(max_ground_neighbours=299))
    pm.set_map(parts["map"], parts["ground"], parts["normals"])
    refused(K.ERR_CAPACITY, pm.measure, parts["flat"], parts["ls"], parts["states"])
    assert pm.last.n_over_capacity == 1 and pm.last.max_ground_neighbours_seen == 300
    pm = localization.ParticleMeasure(lp, config(max_ground_neighbours=300, max_particles=6, max_observation_points=133))
    assert_parity(run(pm, parts), ref, "exactly at every capacity")
    refused(K.ERR_CAPACITY, pm.measure, parts["flat"], parts["ls"], np.concatenate([parts["states"], parts["states"][:1]]))
    refused(K.ERR_CAPACITY, pm.measure, np.concatenate([parts["flat"], parts["flat"][:1]]), parts["ls"], parts["states"])
    refused(K.ERR_BAD_ARG, pm.measure, np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), parts["states"])
    like, qual = pm.measure(parts["flat"], parts["ls"], parts["states"][:0])
    assert len(like) == 0 and pm.last.quality_min == 1.0 and pm.last.quality_max == 0.0


def test_measure_during_a_pending_tick_is_refused(lp):
    parts, ref, _ = Cs.case("n64-o3x130")
    sc = scenes.bench_scene("C2")
    pm = localization.ParticleMeasure(lp, config())
    pm.set_map(parts["map"], parts["ground"], parts["normals"])
    lp.set_cloud(sc.cloud)
    lp.setPlan(sc.plan)
    lp.tick_begin(sc.theory.name.decode(), sc.tick)
    try:
        refused(K.ERR_STATE, pm.measure, parts["flat"], parts["ls"], parts["states"])
        refused(K.ERR_STATE, pm.set_map, parts["map"], parts["ground"], parts["normals"])
    finally:
        lp.tick_end()
    like, qual = pm.measure(parts["flat"], parts["ls"], parts["states"])
    assert_parity((like, qual, pm.terms(len(like)), pm.last), ref, "after the tick")


def test_non_finite_states_and_points(lp):
    parts, ref, _ = Cs.case("n65-o1x1")
    states = parts["states"].copy()
    states[3, 0], states[10, 5], states[64, 6] = np.nan, np.inf, -np.inf
    flat = np.concatenate([parts["flat"], np.array([[np.nan, 0, 0]], np.float32)])
    ls = np.concatenate([parts["ls"], np.array([[0, np.inf, 0, 1.0]], np.float32)])
    want = R.measure(Cs.CFG, parts["map"], parts["ground"], parts["normals"], flat, ls, states)
    assert want["n_bad"] == 3 and int(want["n_fragile"].sum()) == 0 and int(want["n_tied"].sum()) == 0
    pm = localization.ParticleMeasure(lp, config())
    pm.set_map(parts["map"], parts["ground"], parts["normals"])
    like, qual = pm.measure(flat, ls, states)
    assert_parity((like, qual, pm.terms(65), pm.last), want, "non-finite inputs")
    assert (like[[3, 10, 64]] == 0).all() and (qual[[3, 10, 64]] == 0).all() and pm.last.n_bad_states == 3
    ok = np.ones(65, bool)
    ok[[3, 10, 64]] = False
    # the two junk points count in the denominator only
    np.testing.assert_array_equal(pm.terms(65)["n_match"][ok], ref["n_match"][ok])
    np.testing.assert_array_equal(bits(qual[ok]), bits(ref["n_match"][ok].astype(np.float32) / np.float32(4)))
