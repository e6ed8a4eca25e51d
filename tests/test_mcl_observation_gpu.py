"""GPU tests of the localiser's observation on the device (dddmr_rollout_mcl_prepare / _prepare_from_sweep /
_get_observation / _measure_prepared, localization.ParticleMeasure) against the NumPy restatement of mcl_3dl's
cbLeGoFeatureCloud (tests/helpers/mcl_observation_ref.py, UNPINNED: PCL cannot be built here).

The flat cloud and the cluster branch's less-sharp cloud are compared on bits, in order: the same IEEE float operations
on both sides, and the cluster order is the same std::sort replay.  The normals go through atan2f / cosf / sinf, which
differ between the device's and the host's libm in the last ulp, so they are compared by angle against the float64
answer (bound 2 * a_ref: an ulp of those functions cannot double the closed form's own float error, which is a_ref);
the dominant branch's weights are checked against the device's OWN sums and decision, bit for bit.  The conditions that
make this sound (ratios far from 1.6, few ratios near 0.5) are asserted on the restatement in
tests/test_mcl_observation_cpu.py.

Measured on an MI355X (test_normals_within_twice_the_restatements_error prints the figures, DESIGN.md 4e records them):
a_ref = 0.0252 rad (a 3-point island; 8.4e-5 rad on the walls), the device's largest deviation 0.0252 rad at the same
point, the sums within 1.5e-6 of the restatement's."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, localization, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcl_observation_ref as R  # noqa: E402
import mcl_observation_cases as Cs  # noqa: E402
import mcl_measure_cases as MC  # noqa: E402
import lidar_features_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
T = Cs.T_B2S
NO_FLAT = np.zeros((0, 3), F)
TBS = (0.1, 0.0, 0.6) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.05))
TGB = (1.0, -0.5, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.3))
WINDOW, HEIGHT = 8.0, 1.8


def mcl_config(**kw):
    c = MC.CFG
    d = dict(match_dist_min=c.match_dist_min, match_dist_flat=c.match_dist_flat, radius_of_ground_search=c.radius_of_ground_search,
             threshold_for_trusted_ground=c.threshold_for_trusted_ground, max_map_points=20000, max_ground_points=20000,
             max_particles=512, max_observation_points=2000, max_ground_neighbours=512)
    d.update(kw)
    return localization.shipped_config(**d)


def obs_config(max_flat=400, max_ls=1600, **kw):
    return localization.shipped_observation_config(euc_cluster_distance=Cs.TOL, euc_cluster_min_size=Cs.MIN_SIZE, max_flat_points=max_flat,
                                                   max_less_sharp_points=max_ls, **kw)


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:      # (the C2 scene's cloud, for the pending tick)
        yield p


@pytest.fixture()
def pm(lp):
    m = localization.ParticleMeasure(lp, mcl_config())
    m.configure_observation(obs_config())
    return m


@pytest.fixture(scope="module")
def room():
    parts = MC.room_case(4242, 60, 0, 0)
    for v in parts.values():
        v.setflags(write=False)
    return parts


def refused(code, fn, *a, **kw):
    with pytest.raises(RolloutError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, code, str(e.value))


def same(a, b):
    return np.ascontiguousarray(a, F).tobytes() == np.ascontiguousarray(b, F).tobytes()


def snapshot(pm):
    return tuple(a.copy() for a in pm.observation())


def assert_snapshot(pm, snap, what):
    for a, b in zip(pm.observation(), snap):
        assert a.shape == b.shape and same(a, b), what


# ---- 1. flat lists ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Cs.FLAT_COUNTS)
def test_flat_cloud_bit_for_bit(pm, n):
    f, want = Cs.flat_case(n)
    ls, _, _ = Cs.case("mixed-5")
    st = pm.prepare(f, ls, T)
    flat, _, _ = pm.observation()
    assert (st.n_flat_in, st.n_flat_out) == (n, len(want)) and flat.shape == want.shape
    assert same(flat, want)
    assert st.host_waits == 1 and 1 <= st.launches <= 2


# ---- 2. the cluster branch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Cs.CLUSTER)
def test_cluster_branch_bit_for_bit(lp, name):
    ls, ref, _ = Cs.case(name)
    pm = localization.ParticleMeasure(lp, mcl_config())
    big = len(ls) > 1600
    pm.configure_observation(obs_config(100, 1900) if big else obs_config())
    flat = Cs.flat_case(100)[0] if big else Cs.flat_case(1)[0] if len(ls) == 0 else NO_FLAT
    st = pm.prepare(flat, ls, T)
    f, l, nrm = pm.observation()
    assert st.branch == K.MCL_BRANCH_CLUSTERS == ref["branch"]
    assert (st.n_less_sharp_in, st.n_less_sharp_out, st.n_clusters, st.n_small_clusters, st.n_nan_normals) == \
        (len(ls), len(ref["ls"]), ref["n_clusters"], ref["n_small_clusters"], ref["n_nan_normals"])
    assert l.shape == ref["ls"].shape and same(l, ref["ls"]), name
    assert len(nrm) == len(ls) and len(f) == st.n_flat_out
    assert st.host_waits == 1 and st.launches == (2 if ref["n_clusters"] else 1)


# ---- 3. the dominant branches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Cs.DOMINANT)
def test_dominant_branch(pm, name):
    ls, ref, _ = Cs.case(name)
    st = pm.prepare(NO_FLAT, ls, T)
    _, l, nrm = pm.observation()
    assert st.branch == ref["branch"] != K.MCL_BRANCH_CLUSTERS
    assert st.n_less_sharp_out == len(ls) and l.shape == (len(ls), 4)
    assert same(l[:, :3], ref["pts"])                                             # every point, input order
    # every intensity is what step 5 gives from the device's own sums: float(0.05 * sy / sx) (mirrored for y), or 1
    sx, sy = st.sum_normal_x, st.sum_normal_y
    low = F(0.05 * sy / sx) if st.branch == K.MCL_BRANCH_X_DOMINANT else F(0.05 * sx / sy)
    is_low, is_one = l[:, 3].view(np.uint32) == np.array(low, F).view(np.uint32), l[:, 3] == F(1.0)
    assert (is_low | is_one).all() and low != F(1.0)
    # ... and the decision is the restatement's wherever its ratio is not within 0.02 of 0.5
    r = ref["ratio"].astype(np.float64)
    far = ~(np.abs(r - 0.5) < Cs.NEAR_HALF)
    want_low = (~np.isnan(ref["normals"][:, 0])) & (r >= 0.5)
    assert far.mean() >= 0.98
    assert (is_low[far] == want_low[far]).all()
    # the device's own normals give the same decision at every point (the ratio is one float division)
    own = R.dominant_intensity(st.branch, nrm, sx, sy)
    assert same(l[:, 3], own)


def test_fewer_than_three_points_give_nan_normals_and_the_cluster_branch(pm):
    for name in ("mixed-1", "mixed-2"):
        ls, ref, _ = Cs.case(name)
        st = pm.prepare(Cs.flat_case(1)[0], ls, T)
        _, l, nrm = pm.observation()
        assert np.isnan(nrm).all() and len(nrm) == len(ls)
        assert st.n_nan_normals == len(ls) and st.branch == K.MCL_BRANCH_CLUSTERS and len(l) == 0 and st.n_clusters == 0


# ---- 4. normals ---------------------------------------------------------------------------------------------------------------
def test_normals_within_twice_the_restatements_error(pm):
    bound = 2.0 * Cs.a_ref()
    worst_a = worst_s = 0.0
    pm.configure_observation(obs_config(100, 1900))
    for name in Cs.NAMES:
        ls, ref, _ = Cs.case(name)
        if len(ls) < 3:
            continue
        st = pm.prepare(NO_FLAT, ls, T)
        _, _, nrm = pm.observation()
        want = R.normals_f64(ref["pts"], ref["nb"])
        assert (np.isnan(nrm[:, 0]) == np.isnan(ref["normals"][:, 0])).all(), name
        a = R.angle(nrm, want)
        a = a[~np.isnan(a)]
        ds = max(abs(st.sum_normal_x - ref["sum_x"]), abs(st.sum_normal_y - ref["sum_y"]))
        print(f"{name}: largest angle to the float64 normal {a.max():.3g} rad (bound {bound:.3g}), sums off by {ds:.3g} (bound {len(ls) * bound:.3g})")
        worst_a, worst_s = max(worst_a, float(a.max())), max(worst_s, ds / len(ls))
        assert a.max() <= bound, name
        assert ds <= len(ls) * bound, name
    print(f"largest deviation: {worst_a:.6g} rad; sums: {worst_s:.3g} per point")


# ---- 5. measure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (7, 60))
def test_measure_prepared_equals_measure_on_the_read_back_arrays(pm, room, n):
    pm.set_map(room["map"], room["ground"], room["normals"])
    states = room["states"][:n]
    for name, nf in (("islands", 100), ("x-walls", 2)):
        pm.prepare(Cs.flat_case(nf)[0], Cs.case(name)[0], T)
        f, l, _ = pm.observation()
        like, qual = pm.measure_prepared(states)
        st, terms = pm.last, pm.terms(n)
        like2, qual2 = pm.measure(f, l, states)
        st2, terms2 = pm.last, pm.terms(n)
        assert same(like, like2) and same(qual, qual2) and len(like) == n
        assert bytes(st) == bytes(st2) and st.launches == 3
        for k in terms:
            assert terms[k].tobytes() == terms2[k].tobytes(), k
        assert qual.max() > 0.0                                                    # (the observation does match the room somewhere)


# ---- 6. the sweep path -----------------------------------------------------------------------------------------------------------
def sweep_planner(max_points=200_000):
    return LocalPlanner([configs.bench_theory("C2")], max_points=max_points)


def configure_sweep(p, c):
    args, kwargs = c.planner_args()
    p.set_lidar_sweep_source(0, *args, **kwargs)
    p.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)


def lists_of(p):
    return p.get_lidar_sweep_features(0, 2)[0], p.get_lidar_sweep_features(0, 1)[0]


def test_prepare_from_sweep_equals_prepare_on_the_read_back_lists():
    c, raw, _, _ = FC.case("16x1000-g7-m0.0")
    with sweep_planner() as p:
        configure_sweep(p, c)
        p.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        flat, ls = lists_of(p)
        assert len(flat) > 0 and len(ls) > 0 and len(flat) + len(ls) <= 2000
        m = localization.ParticleMeasure(p, mcl_config())
        m.configure_observation(obs_config(len(flat), len(ls)))
        st = m.prepare_from_sweep(0, T)
        a = snapshot(m)
        st2 = m.prepare(flat[:, :3], ls, T)                                       # (a [n,4] array: the stride skips the ring)
        assert_snapshot(m, a, "prepare on the lists")
        assert bytes(st)[: K.MclObservationStats.launches.offset] == bytes(st2)[: K.MclObservationStats.launches.offset]
        assert (st.n_flat_in, st.n_less_sharp_in) == (len(flat), len(ls)) and len(a[0]) + len(a[1]) > 0
        refused(K.ERR_STATE, m.prepare_from_sweep, 1, T)                          # not a sweep source
        p.set_lidar_sweep_features(0, enable=False)
        refused(K.ERR_STATE, m.prepare_from_sweep, 0, T)                          # features off
        assert_snapshot(m, a, "after the refusals")


def test_prepare_from_sweep_after_a_refused_sweep():
    c, raw, _, _ = FC.case("16x440-g7-m0.0")
    with np.errstate(invalid="ignore"):
        small = np.ascontiguousarray(raw[raw[:, 0] > 0])
    with sweep_planner() as p:
        configure_sweep(p, c)
        n_full = p.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)[1]
    with sweep_planner(max_points=n_full - 1) as p:
        configure_sweep(p, c)
        p.set_lidar_sweep(0, small, TBS, TGB, WINDOW, HEIGHT)
        flat, ls = lists_of(p)
        m = localization.ParticleMeasure(p, mcl_config())
        m.configure_observation(obs_config())
        m.prepare_from_sweep(0, T)
        a = snapshot(m)
        assert len(a[0]) + len(a[1]) > 0
        refused(K.ERR_CAPACITY, p.set_lidar_sweep, 0, raw, TBS, TGB, WINDOW, HEIGHT)
        m.prepare(NO_FLAT, Cs.case("mixed-5")[0], T)                              # something else in between
        m.prepare_from_sweep(0, T)
        assert_snapshot(m, a, "the previous sweep's features")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(lp, room):
    m = localization.ParticleMeasure(lp, mcl_config())
    ls, flat = Cs.case("mixed-65")[0], Cs.flat_case(100)[0]
    refused(K.ERR_STATE, m.prepare, flat, ls, T)                                  # no configuration
    refused(K.ERR_STATE, m.measure_prepared, room["states"][:7])
    for kw in (dict(euc_cluster_min_size=-1), dict(euc_cluster_distance=0.0), dict(euc_cluster_distance=-0.8),
               dict(euc_cluster_distance=float("nan")), dict(euc_cluster_distance=float("inf")), dict(flags=1)):
        refused(K.ERR_BAD_ARG, m.configure_observation, localization.shipped_observation_config(**kw))
    refused(K.ERR_CAPACITY, m.configure_observation, obs_config(401, 1600))
    m.configure_observation(obs_config(100, 65))
    m.set_map(room["map"], room["ground"], room["normals"])
    refused(K.ERR_BAD_ARG, m.measure_prepared, room["states"][:7])                # no observation point yet
    f0, l0, n0 = m.observation()
    assert len(f0) == len(l0) == len(n0) == 0
    m.prepare(flat, ls, T)
    snap = snapshot(m)
    like, qual = m.measure_prepared(room["states"][:7])

    def unchanged(what):
        assert_snapshot(m, snap, what)
        l2, q2 = m.measure_prepared(room["states"][:7])
        assert same(like, l2) and same(qual, q2), what

    refused(K.ERR_CAPACITY, m.prepare, Cs.flat_case(384)[0], ls, T)
    refused(K.ERR_CAPACITY, m.prepare, flat, Cs.case("mixed-600")[0], T)
    unchanged("capacity")
    for bad in (np.nan, np.inf, -np.inf):
        b = ls.copy()
        b[3, 1] = bad
        refused(K.ERR_BAD_ARG, m.prepare, flat, b, T)
        b = flat.copy()
        b[99, 2] = bad
        refused(K.ERR_BAD_ARG, m.prepare, b, ls, T)
        Tb = np.array(T)
        Tb[1, 3] = bad
        refused(K.ERR_BAD_ARG, m.prepare, flat, ls, Tb)
        refused(K.ERR_BAD_ARG, m.prepare_from_sweep, 0, Tb)
    unchanged("bad arguments")
    refused(K.ERR_STATE, m.prepare_from_sweep, 0, T)                              # source 0 is no sweep source here
    refused(K.ERR_BAD_ARG, m.prepare_from_sweep, 99, T)
    rc = lp._lib.dddmr_rollout_mcl_get_observation(lp._ctx, snap[0].ctypes.data, 1, K.C.byref(K.C.c_size_t()), None, 0,
                                                   K.C.byref(K.C.c_size_t()), None, 0)
    assert rc == K.ERR_CAPACITY
    unchanged("state")
    sc = scenes.bench_scene("C2")
    lp.set_cloud(sc.cloud)
    lp.setPlan(sc.plan)
    lp.tick_begin(sc.theory.name.decode(), sc.tick)
    try:
        refused(K.ERR_STATE, m.prepare, flat, ls, T)
        refused(K.ERR_STATE, m.measure_prepared, room["states"][:7])
        refused(K.ERR_STATE, m.observation)
    finally:
        lp.tick_end()
    unchanged("a pending tick")
    m.configure_observation(None)
    refused(K.ERR_STATE, m.prepare, flat, ls, T)


# ---- 8. non-interference ----------------------------------------------------------------------------------------------------------
def test_prepare_leaves_measure_as_it_was(pm, room):
    parts, _, _ = MC.case("n64-o3x130")
    pm.set_map(parts["map"], parts["ground"], parts["normals"])
    before = pm.measure(parts["flat"], parts["ls"], parts["states"])
    tb = pm.terms(len(parts["states"]))
    pm.prepare(Cs.flat_case(100)[0], Cs.case("islands")[0], T)
    pm.measure_prepared(room["states"][:7])
    after = pm.measure(parts["flat"], parts["ls"], parts["states"])
    ta = pm.terms(len(parts["states"]))
    assert same(before[0], after[0]) and same(before[1], after[1])
    for k in tb:
        assert tb[k].tobytes() == ta[k].tobytes(), k


# ---- 9. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_prepares_give_the_same_bytes(pm):
    ls, flat = Cs.case("islands")[0], Cs.flat_case(100)[0]
    st = pm.prepare(flat, ls, T)
    a = snapshot(pm)
    pm.prepare(Cs.flat_case(2)[0], Cs.case("x-walls")[0], T)                       # (the other buffer, another branch)
    st2 = pm.prepare(flat, ls, T)
    assert_snapshot(pm, a, "the second prepare")
    assert bytes(st)[: K.MclObservationStats.host_waits.offset] == bytes(st2)[: K.MclObservationStats.host_waits.offset]
