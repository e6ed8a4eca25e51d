"""GPU tests of the localiser's sub-maps (dddmr_rollout_submap_*): the keyframe store, the warm-up's gathered clouds,
neighbours and normals against tests/helpers/submap_ref.py (UNPINNED, see there), the swap against mcl_set_map, and the
refusals.  tests/test_submap_cpu.py holds the conditions on the cases that these tests rely on."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, localization, scenes, submaps
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcl_measure_cases as MC  # noqa: E402
import submap_ref as S  # noqa: E402
import submap_cases as Cs  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def mcl_config(**kw):
    c = MC.CFG
    d = dict(match_dist_min=c.match_dist_min, match_dist_flat=c.match_dist_flat, radius_of_ground_search=c.radius_of_ground_search,
             threshold_for_trusted_ground=c.threshold_for_trusted_ground, max_map_points=20000, max_ground_points=20000,
             max_particles=512, max_observation_points=2000, max_ground_neighbours=512)
    d.update(kw)
    return localization.shipped_config(**d)


def sub_config(**kw):
    d = dict(max_keyframes=16, max_store_map_points=20000, max_store_ground_points=20000, normal_k=20)
    d.update(kw)
    return submaps.shipped_config(**d)


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:      # (the C2 scene's cloud, for the pending tick)
        yield p


@pytest.fixture(scope="module")
def lp2():
    with LocalPlanner([configs.bench_theory("C2")], max_points=1000) as p:
        yield p


def fresh(lp, **kw):
    pm = localization.ParticleMeasure(lp, mcl_config())
    return pm, submaps.SubMaps(lp, pm, sub_config(**kw))


def load(sm, kfs):
    return [sm.add_keyframe(k["corner"], k["ground"], k["position"], k["T"]) for k in kfs]


def refused(code, fn, *a):
    with pytest.raises(RolloutError) as e:
        fn(*a)
    assert e.value.code == code, (e.value.code, str(e.value))


def same_generation(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("map", "ground", "normals", "neighbours"))


@pytest.mark.parametrize("name", Cs.NAMES)
def test_warm_up_matches_the_restatement(lp, name):
    """Every case: the gathered clouds byte for byte (with transforms this pins the rounding), every neighbour row and
    position exactly, the normals' NaN pattern, and elsewhere the angle to the float64 normal within twice the
    restatement's own largest angle on the same case.  Figures measured on an MI355X: see the print below (run with -s)."""
    kfs, ids, ref = Cs.case(name)
    pm, sm = fresh(lp)
    assert load(sm, kfs) == list(range(len(kfs)))
    st = sm.warm_up(ids)
    got = sm.get(1)
    assert (st.n_keyframes, st.n_map, st.n_ground) == (len(ids), len(ref["map"]), len(ref["ground"]))
    assert st.host_waits == 1 and st.launches <= 16
    assert got["map"].tobytes() == ref["map"].tobytes() and got["ground"].tobytes() == ref["ground"].tobytes()
    np.testing.assert_array_equal(got["neighbours"], ref["neighbours"])
    nan = np.isnan(got["normals"][:, 0])
    np.testing.assert_array_equal(nan, np.isnan(ref["normals"][:, 0]))
    assert st.n_nan_normals == int(nan.sum())
    bound, n_cmp, _, _ = Cs.restatement_error(name)
    cmp_ = ~nan & ref["defined"]
    ang = S.R.angle(got["normals"][cmp_], ref["normals_f64"][cmp_]) if cmp_.any() else np.zeros(1)
    equal = int((got["normals"][~nan].view(np.uint32) == ref["normals"][~nan].view(np.uint32)).all(axis=1).sum())
    print(f"{name}: {len(nan)} ground points, {int(cmp_.sum())} compared: device to float64 at most {float(ang.max()):.3e} rad, restatement "
          f"{bound:.3e} rad; {equal} of {int((~nan).sum())} normals bit-equal to the restatement; rings {st.max_rings_searched}, "
          f"brute force {st.n_brute_force}, launches {st.launches}")
    assert int(cmp_.sum()) == n_cmp
    assert float(ang.max()) <= 2.0 * bound, (name, float(ang.max()), bound)
    if name == "f":
        assert st.n_brute_force >= 2            # the two lone points finish by the pass over the whole cloud
    # nothing became current
    assert len(sm.get(0)["ground"]) == 0


def test_same_list_same_bytes_and_the_reversed_list_reversed(lp):
    kfs, ids, ref = Cs.case("a")
    pm, sm = fresh(lp)
    load(sm, kfs)
    sm.warm_up(ids)
    a = sm.get(1)
    sm.warm_up(ids)
    assert same_generation(a, sm.get(1))
    sm.warm_up(ids[::-1])
    r = sm.get(1)
    m, g = S.concatenate(kfs, ids[::-1])
    assert r["map"].tobytes() == m.tobytes() and r["ground"].tobytes() == g.tobytes()
    np.testing.assert_array_equal(r["neighbours"], S.neighbours(g))
    # a subset of the store, and the empty list
    sm.warm_up(ids[1:3])
    assert sm.get(1)["ground"].tobytes() == S.concatenate(kfs, ids[1:3])[1].tobytes()
    st = sm.warm_up([])
    assert (st.n_map, st.n_ground) == (0, 0) and len(sm.get(1)["map"]) == 0


@pytest.mark.parametrize("n_states", (7, 60))
def test_measure_is_untouched_until_the_swap_and_then_equals_set_map(lp, lp2, n_states):
    room = MC.room_case(77, n_states, 40, 200)
    kfs, ids, ref = Cs.case("a")
    pm, sm = fresh(lp)
    pm.set_map(room["map"], room["ground"], room["normals"])
    measure = lambda p: (p.measure(room["flat"], room["ls"], room["states"]), p.terms(n_states), p.last)
    flat = lambda r: b"".join([r[0][0].tobytes(), r[0][1].tobytes()] + [r[1][k].tobytes() for k in sorted(r[1])] + [bytes(r[2])])
    before = flat(measure(pm))
    load(sm, kfs)
    sm.warm_up(ids)
    assert flat(measure(pm)) == before                       # the warm-up generation is not the current one
    old = sm.get(0)
    assert old["ground"].tobytes() == room["ground"].tobytes() and (old["neighbours"] == -1).all()
    warm = sm.get(1)
    sm.swap()
    cur = sm.get(0)
    assert same_generation(cur, warm) and len(sm.get(1)["ground"]) == 0
    after = measure(pm)
    pm2 = localization.ParticleMeasure(lp2, mcl_config())
    pm2.set_map(cur["map"], cur["ground"], cur["normals"])
    assert flat(after) == flat(measure(pm2))
    assert flat(after) != before
    refused(K.ERR_STATE, sm.swap)                            # the warm-up slot is empty again
    # mcl_set_map keeps working and replaces the current generation only
    pm.set_map(room["map"], room["ground"], room["normals"])
    assert flat(measure(pm)) == before and (sm.get(0)["neighbours"] == -1).all()


def test_refusals_change_nothing(lp):
    kfs, ids, ref = Cs.case("e")
    pm, sm = fresh(lp, max_keyframes=4, max_store_ground_points=1000, max_store_map_points=400)
    refused(K.ERR_STATE, sm.swap)                            # no warm-up yet
    load(sm, kfs)
    sm.warm_up(ids)
    warm = sm.get(1)
    refused(K.ERR_BAD_ARG, sm.warm_up, [0, 3])               # unknown id
    refused(K.ERR_BAD_ARG, sm.warm_up, [0, -1])
    refused(K.ERR_BAD_ARG, sm.warm_up, [0, 1, 0])            # repeated id
    few_c, few_g = kfs[1]["corner"][:10], kfs[1]["ground"][:20]      # (small enough for the store: the argument is what is refused)
    bad = few_g.copy()
    bad[7, 1] = np.nan
    refused(K.ERR_BAD_ARG, sm.add_keyframe, few_c, bad, (0, 0, 0))
    refused(K.ERR_BAD_ARG, sm.add_keyframe, bad[:10], few_g, (0, 0, 0))
    refused(K.ERR_BAD_ARG, sm.add_keyframe, few_c, few_g, (0, np.inf, 0))
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    T[1, 3] = np.nan
    refused(K.ERR_BAD_ARG, sm.add_keyframe, few_c, few_g, (0, 0, 0), T)
    refused(K.ERR_CAPACITY, sm.add_keyframe, kfs[1]["corner"], kfs[1]["ground"], (0, 0, 0))       # 972 + 324 > 1000 ground points
    refused(K.ERR_CAPACITY, sm.add_keyframe, np.zeros((200, 3), F), np.zeros((1, 3), F), (0, 0, 0))   # the corner store
    assert sm.add_keyframe(np.zeros((0, 3), F), kfs[1]["ground"][:20], (9, 9, 9)) == 3             # ids go on where they were
    refused(K.ERR_CAPACITY, sm.add_keyframe, np.zeros((0, 3), F), np.zeros((1, 3), F), (0, 0, 0))  # max_keyframes
    assert sm.select((9, 9, 9), 0.5).tolist() == [3]
    assert same_generation(warm, sm.get(1))
    # a cloud wider than the grids take
    wide = kfs[1]["ground"][:60].copy()
    wide[0, 0] += 5000.0
    pm_w, sm_w = fresh(lp)
    load(sm_w, kfs[:1])
    sm_w.add_keyframe(kfs[1]["corner"], wide, (0, 0, 0))
    sm_w.warm_up([0])
    keep = sm_w.get(1)
    refused(K.ERR_BAD_ARG, sm_w.warm_up, [0, 1])
    assert same_generation(keep, sm_w.get(1))
    # above the mcl state's capacity
    pm_s = localization.ParticleMeasure(lp, mcl_config(max_ground_points=500))
    sm_s = submaps.SubMaps(lp, pm_s, sub_config())
    load(sm_s, kfs)
    sm_s.warm_up([0])
    keep = sm_s.get(1)
    refused(K.ERR_CAPACITY, sm_s.warm_up, [0, 1])
    assert same_generation(keep, sm_s.get(1))
    sm_s.swap()
    assert same_generation(keep, sm_s.get(0))
    # normal_k outside 3 .. 32, and a store without an mcl state's successor
    refused(K.ERR_BAD_ARG, submaps.SubMaps, lp, pm_s, sub_config(normal_k=2))
    refused(K.ERR_BAD_ARG, submaps.SubMaps, lp, pm_s, sub_config(normal_k=33))
    assert same_generation(keep, sm_s.get(0))
    localization.ParticleMeasure(lp, mcl_config())           # a second mcl_create drops the store
    for call in (lambda: sm_s.add_keyframe(kfs[0]["corner"], kfs[0]["ground"], (0, 0, 0)), lambda: sm_s.select((0, 0, 0), 1.0),
                 lambda: sm_s.warm_up([0]), sm_s.swap, lambda: sm_s.get(0), lambda: sm_s.get(1)):
        refused(K.ERR_STATE, call)


def test_warm_up_beside_a_pending_tick_is_refused(lp):
    kfs, ids, ref = Cs.case("b")
    pm, sm = fresh(lp)
    load(sm, kfs)
    sm.warm_up(ids[:2])
    keep = sm.get(1)
    sc = scenes.bench_scene("C2")
    lp.set_cloud(sc.cloud)
    lp.setPlan(sc.plan)
    lp.tick_begin(sc.theory.name.decode(), sc.tick)
    try:
        refused(K.ERR_STATE, sm.warm_up, ids)
        refused(K.ERR_STATE, sm.swap)
    finally:
        lp.tick_end()
    assert same_generation(keep, sm.get(1))
    sm.warm_up(ids)
    assert sm.get(1)["ground"].tobytes() == ref["ground"].tobytes()


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_select_matches_the_restatement(lp, seed):
    k, q, r = Cs.select_case(seed)
    pm, sm = fresh(lp, max_keyframes=len(k))
    one = np.zeros((1, 3), F)
    for p in k:
        sm.add_keyframe(one, one, p)
    want, _ = S.select(k, q, r)
    got = sm.select(q, r)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert sm.select(q, 0.0).tolist() == [] and sm.select(q, 1e4).tolist() == list(range(len(k)))
