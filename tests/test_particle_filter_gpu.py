"""GPU parity of mcl_3dl's particle set on the device (dddmr_rollout_mcl_filter_*, localization.ParticleFilter) against
the NumPy restatement (tests/helpers/particle_filter_ref.py, which tests/test_particle_filter_cpu.py pins on bits to the
reference's own pf.h / state_6dof.h / motion model through tests/golden/REF_MCL_PF_*.npz).

Every stage is tested on its own: the device's state before the stage is downloaded and handed to the restatement, the
state after is compared.  Bit for bit wherever the device evaluates no transcendental: set_noise, reset_integ,
add_noise, measure with supplied likelihoods and no state_prev (probabilities, weight_sum, both means' sums and means,
the max index and state, p_num, all 36 covariances), resample (states, noise, probabilities, counts), and the same stages
against the reference's recorded answers.  predict (sinf / cosf) and the bias (acosf / expf) are compared with the
restatement evaluated in float64; the allowed difference is twice the float32 restatement's own distance to that
float64 answer on the same inputs.

Measured on an MI355X (the two tolerance tests print the figures; DESIGN.md 4e records them): predict at most 2.28e-7 m
(position), 1.48e-7 (rotation), 2.32e-8 / 9.59e-9 (integrals) from the float64 answer, every particle bit-equal to the
float32 restatement; the bias at most 9.84e-9 from the float64 answer, 728 of 1000 values bit-equal."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, localization, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import particle_filter_ref as R  # noqa: E402
import particle_filter_cases as Cs  # noqa: E402
import mcl_measure_cases as MC  # noqa: E402
import mcl_observation_cases as OC  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
CAP = 4096


def mcl_config(**kw):
    c = MC.CFG
    d = dict(match_dist_min=c.match_dist_min, match_dist_flat=c.match_dist_flat, radius_of_ground_search=c.radius_of_ground_search,
             threshold_for_trusted_ground=c.threshold_for_trusted_ground, max_map_points=20000, max_ground_points=20000,
             max_particles=CAP, max_observation_points=2000, max_ground_neighbours=512)
    d.update(kw)
    return localization.shipped_config(**d)


def filter_config(**kw):
    d = dict(max_particles=CAP, odom_err_integ_lin_tc=Cs.LIN_TC, odom_err_integ_ang_tc=Cs.ANG_TC, bias_var_dist=Cs.VAR_DIST,
             bias_var_ang=Cs.VAR_ANG)
    d.update(kw)
    return localization.shipped_filter_config(**d)


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:      # (the C2 scene's cloud, for the pending tick)
        yield p


@pytest.fixture(scope="module")
def both(lp):
    pm = localization.ParticleMeasure(lp, mcl_config())
    return pm, localization.ParticleFilter(lp, filter_config())


@pytest.fixture()
def pf(both):
    return both[1]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b, what):
    a, b = np.asarray(a, F), np.asarray(b, F)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(bits(a) != bits(b))
    assert len(bad) == 0, (what, f"{len(bad)} of {a.size} differ", tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


def arr(x):
    return np.array(x[:], F)


def refused(code, fn, *a, **kw):
    with pytest.raises(RolloutError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def assert_set(pf, states, prob, noise4, what):
    got = pf.particles()
    same(got["states"], states, what + ": states")
    same(got["probability"], prob, what + ": probabilities")
    same(got["noise4"], noise4, what + ": noise")
    return got


def assert_estimate(est, ref, what):
    same(arr(est.sums_biased), ref["sums_biased"], what + ": biased sums")
    same(arr(est.sums), ref["sums"], what + ": unbiased sums")
    same(arr(est.mean_biased), ref["mean_biased"], what + ": biased mean")
    same(arr(est.mean), ref["mean"], what + ": mean")
    same(arr(est.max_state), ref["max_state"], what + ": max state")
    same(arr(est.cov).reshape(6, 6), ref["cov"], what + ": covariance")
    assert (est.p_num, est.max_index) == (ref["p_num"], ref["max_index"]), what
    assert bits(est.bias_sum) == bits(ref["sums_biased"][0]) and est.host_waits == 1, what


# ---- 1. the plain stages ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Cs.SIZES)
def test_set_noise_reset_integ_add_noise_on_bits(pf, n):
    s, z = Cs.particles(n)
    pf.set_particles(s)
    got = assert_set(pf, s, np.full(n, F(1.0 / np.float64(n)), F), np.zeros((n, 4), F), "set_particles")
    assert not got["bias"].any()
    p = Cs.probability(n, "normalised")
    pf.set_particles(s, p, z)
    assert_set(pf, s, p, z, "set_particles with probabilities and noise")
    z2 = Cs.particles(n, 1)[1]
    pf.set_noise(z2)
    assert_set(pf, s, p, z2, "set_noise")
    rows = Cs.noise_rows(n)
    pf.add_noise(rows)
    s2, z3 = R.add_noise(s, rows)
    assert_set(pf, s2, p, z3, "add_noise")
    pf.reset_integ()
    s2[:, 7:13] = 0
    assert_set(pf, s2, p, z3, "reset_integ")


# ---- 2. measure with supplied likelihoods ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("normalised", "sum1.5"))
@pytest.mark.parametrize("n", Cs.SIZES)
def test_measure_with_supplied_likelihoods_on_bits(pf, n, kind):
    s, z = Cs.particles(n)
    p = Cs.probability(n, kind)
    broke = False
    for lk_kind in Cs.LIKELIHOODS:
        what = f"n={n} {kind} {lk_kind}"
        lk = Cs.likelihood(n, lk_kind)
        qual = (lk * F(0.5)).astype(F)
        pf.set_particles(s, p, z)
        est = pf.measure(lk, qual)
        p2, total, restored = R.weigh(p, lk)
        ref = R.estimate(s, p2, np.ones(n, F))
        got = assert_set(pf, s, p2, z, what)
        same(got["bias"], np.ones(n, F), what + ": bias")
        assert bits(est.weight_sum) == bits(total) and est.restored == restored == int(lk_kind == "all-zero"), what
        assert_estimate(est, ref, what)
        assert bits(est.quality_min) == bits(min(F(1), qual.min())) and bits(est.quality_max) == bits(max(F(0), qual.max())), what
        broke |= ref["p_num"] < n
    assert broke or kind != "sum1.5" or n <= 2, "expectation(1.0)'s break falls inside the array"


# ---- 3. resample -----------------------------------------------------------------------------------------------------
def run_resample(pf, s, z, p, u, rows, what):
    pf.set_particles(s, p, z)
    ref = R.resample(s, z, p, u, rows)
    st = pf.resample(u, rows)
    assert (st.n_duplicates, st.n_at_end, st.n_ties) == (ref["n_duplicates"], ref["n_at_end"], ref["n_ties"]), what
    assert_set(pf, ref["states"], ref["probability"], ref["noise4"], what)
    return ref


@pytest.mark.parametrize("n", Cs.SIZES + (100,))
def test_resample_on_bits(pf, n):
    s, z = Cs.particles(n)
    rows = Cs.noise_rows(n)
    ties = ends = 0
    for lk_kind in ("unweighted", "plain", "third-zero", "tiny"):
        p = Cs.probability(n, "normalised")
        if lk_kind != "unweighted":
            p = R.weigh(p, Cs.likelihood(n, lk_kind))[0]
        for u in (0.0, 0.37, float(Cs.U_MAX)):
            ref = run_resample(pf, s, z, p, u, rows, f"n={n} {lk_kind} u={u}")
            ties, ends = ties + ref["n_ties"], ends + ref["n_at_end"]
            if ref["n_duplicates"]:                       # one row short: refused, nothing changes
                pf.set_particles(s, p, z)
                refused(K.ERR_CAPACITY, pf.resample, u, rows[: ref["n_duplicates"] - 1])
                assert pf.last_resample.n_duplicates == ref["n_duplicates"]
                assert_set(pf, s, p, z, f"n={n} {lk_kind} u={u}: after the refusal")
    assert ties > 0 or n < 3
    assert ends > 0 or n != 100, "n = 100 was chosen because the largest u reaches the end() branch there"


# ---- 4. the reference's recorded answers -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", Cs.GOLDEN_SIZES)
def test_stages_without_device_transcendentals_match_the_reference_on_bits(pf, n):
    g = Cs.golden(n)
    what = f"golden n={n}"
    pf.set_particles(g["predict_states"], g["in_probability"], g["predict_noise4"])
    est = pf.measure(g["likelihood"])
    assert_set(pf, g["measure_states"], g["measure_probability"], g["measure_noise4"], what + " measure")
    same(arr(est.mean), g["measure_mean"], what + ": mean")
    same(arr(est.max_state), g["measure_max_state"], what + ": max")
    same(arr(est.cov).reshape(6, 6), g["measure_cov"], what + ": covariance")
    # the probabilities times 1.5 (restored by an all-zero likelihood): expectation(1.0) breaks inside the array
    pf.set_particles(g["scaled_states"], g["scaled_probability"], g["scaled_noise4"])
    est = pf.measure(np.zeros(n, F))
    assert est.restored == 1 and (est.p_num < n or n <= 2)
    same(arr(est.mean), g["scaled_mean"], what + ": scaled mean")
    same(arr(est.cov).reshape(6, 6), g["scaled_cov"], what + ": scaled covariance")
    # resample and pf::noise, the rows from the engine's recorded draws
    rows = np.stack([R.noise_row(d) for d in g["resample_draws"]])
    pf.set_particles(g["measure_states"], g["measure_probability"], g["measure_noise4"])
    st = pf.resample(float(g["resample_u"][0]), rows)
    assert st.n_ties == int(g["resample_ties"][0])
    assert_set(pf, g["resample_states"], g["resample_probability"], g["resample_noise4"], what + " resample")
    pf.add_noise(np.stack([R.noise_row(d) for d in g["add_noise_draws"]]))
    assert_set(pf, g["add_noise_states"], g["add_noise_probability"], g["add_noise_noise4"], what + " add_noise")


# ---- 5. predict and the bias: sinf / cosf / acosf / expf on the device -------------------------------------------------
def group_errors(got, f32, f64):
    """per group of state components: (device's distance to float64, the float32 restatement's)"""
    out = {}
    for name, sl in (("pos", slice(0, 3)), ("rot", slice(3, 7)), ("integ_lin", slice(7, 10)), ("integ_ang", slice(10, 13))):
        out[name] = (float(np.abs(got[:, sl].astype(np.float64) - f64[:, sl]).max()), float(np.abs(f32[:, sl].astype(np.float64) - f64[:, sl]).max()))
    return out


def test_predict_within_twice_the_restatements_error(pf):
    worst = {}
    inputs = [(f"n={n}", *Cs.particles(n), Cs.ODOM_PREV, Cs.ODOM_CUR, Cs.DT, Cs.LIN_TC, Cs.ANG_TC) for n in (1, 65, 1000)]
    for n in Cs.GOLDEN_SIZES:
        g = Cs.golden(n)
        inputs.append((f"golden n={n}", g["in_states"], g["in_noise4"], g["odom_prev"], g["odom_cur"], *g["predict_params"]))
    for what, s, z, a, b, dt, lin_tc, ang_tc in inputs:
        o = R.set_odoms(a, b, dt, lin_tc, ang_tc)
        assert (F(lin_tc), F(ang_tc)) == (F(Cs.LIN_TC), F(Cs.ANG_TC))
        pf.set_particles(s, None, z)
        pf.predict(a, b, float(dt))
        got = pf.particles()
        same(got["noise4"], z, what)
        f32, f64 = R.predict(s, z, o), R.predict_f64(s, z, o)
        assert np.isfinite(got["states"]).all(), what
        for name, (dev, ref) in group_errors(got["states"], f32, f64).items():
            print(f"{what} {name}: device {dev:.3g}, float32 restatement {ref:.3g} from the float64 answer")
            assert dev <= 2.0 * ref, (what, name, dev, ref)
            worst[name] = max(worst.get(name, (0.0, 0.0)), (dev, ref))
        n_equal = int((bits(got["states"]) == bits(f32)).all(axis=1).sum())
        print(f"{what}: {n_equal} of {len(s)} particles bit-equal to the float32 restatement")
    print("largest distances to the float64 answer (device, float32 restatement):", worst)


def test_bias_within_twice_the_restatements_error_and_biased_sums_on_bits(pf):
    worst = (0.0, 0.0)
    for n in (1, 65, 1000):
        s, z = Cs.particles(n)
        p, lk = Cs.probability(n, "normalised"), Cs.likelihood(n, "plain")
        pf.set_particles(s, p, z)
        est = pf.measure(lk, None, Cs.STATE_PREV)
        got = pf.particles()
        f32, f64 = R.bias(s, Cs.STATE_PREV, Cs.VAR_DIST, Cs.VAR_ANG), R.bias_f64(s, Cs.STATE_PREV, Cs.VAR_DIST, Cs.VAR_ANG)
        dev, ref = float(np.abs(got["bias"].astype(np.float64) - f64).max()), float(np.abs(f32.astype(np.float64) - f64).max())
        print(f"n={n} bias: device {dev:.3g}, float32 restatement {ref:.3g} from the float64 answer; "
              f"{int((bits(got['bias']) == bits(f32)).sum())} of {n} bit-equal")
        assert np.isfinite(got["bias"]).all() and dev <= 2.0 * ref, (n, dev, ref)
        worst = max(worst, (dev, ref))
        # everything after the bias, fed the device's own bias, on bits
        p2 = R.weigh(p, lk)[0]
        same(got["probability"], p2, f"n={n}")
        assert_estimate(est, R.estimate(s, p2, got["bias"]), f"n={n} with the device's bias")
    print("largest distance to the float64 bias (device, float32 restatement):", worst)


# ---- 6. the lidar model on the resident poses, and the closed loop -----------------------------------------------------
@pytest.fixture(scope="module")
def room():
    parts = MC.room_case(4242, 60, 0, 0)
    for v in parts.values():
        v.setflags(write=False)
    return parts


def prepare_room(pm, room):
    pm.configure_observation(localization.shipped_observation_config(euc_cluster_distance=OC.TOL, euc_cluster_min_size=OC.MIN_SIZE))
    pm.set_map(room["map"], room["ground"], room["normals"])
    pm.prepare(OC.flat_case(100)[0], OC.case("islands")[0], OC.T_B2S)


def room_states(room, n):
    s = np.zeros((n, 13), F)
    s[:, :7] = room["states"][:n]
    return s


def test_measure_on_the_resident_poses_equals_measure_prepared_then_measure(both, room):
    pm, pf = both
    prepare_room(pm, room)
    n = 60
    s, p = room_states(room, n), Cs.probability(n, "normalised")
    pf.set_particles(s, p)
    est = pf.measure(None, None, Cs.STATE_PREV)
    st, terms, after = pf.last, pm.terms(n), pf.particles()
    like, qual = pm.measure_prepared(np.ascontiguousarray(s[:, :7]))
    assert like.max() > 0 and est.launches == 7 and est.host_waits == 1
    for k, v in pm.terms(n).items():
        assert terms[k].tobytes() == v.tobytes(), k
    assert bytes(st)[: K.MclStats.launches.offset] == bytes(pm.last)[: K.MclStats.launches.offset]
    pf.set_particles(s, p)
    est2 = pf.measure(like, qual, Cs.STATE_PREV)
    again = pf.particles()
    for k in after:
        same(after[k], again[k], k)
    skip = K.MclFilterEstimate.launches.offset
    assert bytes(est)[:skip] == bytes(est2)[:skip]
    assert bits(est.quality_min) == bits(qual.min()) and bits(est.quality_max) == bits(qual.max())


def test_closed_loop_of_twenty_steps(both, room):
    """predict, measure, resample, set_noise at N = 60: the restatement is fed the device's own predict and bias outputs
    (their distance to the host's transcendentals is test 5's), everything else is compared on bits at every step"""
    pm, pf = both
    prepare_room(pm, room)
    n = 60
    rng = np.random.default_rng(77)
    s = room_states(room, n)
    z = (rng.standard_normal((n, 4)) * np.array([0.6, 0.3, 0.3, 0.6]) * 0.1).astype(F)
    pf.set_particles(s, None, z)
    prob = pf.particles()["probability"]
    state_prev = s[0, :7].copy()
    odom = Cs.ODOM_PREV.copy()
    n_dup = 0
    for step in range(20):
        what = f"step {step}"
        cur = odom.copy()
        cur[:3] += np.array([0.004, 0.002, 0.0], F)
        cur[3:7] = R.qnormalized(R.qmul(R.quat_from_rpy(np.array([0, 0, 0.002], F)), odom[3:7]))
        pf.predict(odom, cur, 0.1)
        odom = cur
        s = pf.particles()["states"]                                   # the device's predict output
        like = pm.measure_prepared(np.ascontiguousarray(s[:, :7]))[0]
        est = pf.measure(None, None, state_prev)
        got = pf.particles()
        prob, total, restored = R.weigh(prob, like)
        same(got["probability"], prob, what)
        assert (bits(est.weight_sum), est.restored) == (bits(total), restored), what
        assert_estimate(est, R.estimate(s, prob, got["bias"]), what)
        state_prev = arr(est.mean_biased)
        state_prev[3:7] = R.qnormalized(state_prev[3:7])              # src/mcl_3dl.cpp:545
        u = float(F(rng.uniform(0, 1)))
        rows = np.stack([R.noise_row(d) for d in (rng.standard_normal((n, 6)) * np.array([0.02, 0.02, 0.02, 0.01, 0.01, 0.01])).astype(F)])
        ref = R.resample(s, z, prob, u, rows)
        st = pf.resample(u, rows)
        assert (st.n_duplicates, st.n_at_end, st.n_ties) == (ref["n_duplicates"], ref["n_at_end"], ref["n_ties"]), what
        assert_set(pf, ref["states"], ref["probability"], ref["noise4"], what + " resample")
        n_dup += st.n_duplicates
        prob = ref["probability"]
        z = (rng.standard_normal((n, 4)) * np.array([0.6, 0.3, 0.3, 0.6]) * 0.1).astype(F)
        pf.set_noise(z)
        assert_set(pf, ref["states"], prob, z, what + " set_noise")
    assert n_dup > 0


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:
        refused(K.ERR_STATE, localization.ParticleFilter, p, filter_config())                    # before mcl_create
        localization.ParticleMeasure(p, mcl_config(max_particles=64))
        refused(K.ERR_CAPACITY, localization.ParticleFilter, p, filter_config(max_particles=65))
        for bad in (dict(odom_err_integ_lin_tc=0.0), dict(odom_err_integ_ang_tc=float("nan")), dict(bias_var_dist=-1.0),
                    dict(bias_var_ang=float("inf")), dict(max_particles=0), dict(bias_var_ang=1e-60)):
            refused(K.ERR_BAD_ARG, localization.ParticleFilter, p, filter_config(**dict(dict(max_particles=64), **bad)))
        f = localization.ParticleFilter(p, filter_config(max_particles=64))
        f.n = 4
        for call in (f.particles, f.reset_integ, lambda: f.predict(Cs.ODOM_PREV, Cs.ODOM_CUR, 0.1), lambda: f.set_noise(np.zeros((4, 4), F)),
                     lambda: f.measure(np.ones(4, F)), lambda: f.resample(0.5, np.zeros((4, 10), F)), lambda: f.add_noise(np.zeros((4, 10), F))):
            refused(K.ERR_STATE, call)                                                            # before set_particles
        s, z = Cs.particles(4)
        refused(K.ERR_CAPACITY, f.set_particles, Cs.particles(65)[0])
        bad = s.copy()
        bad[2, 5] = np.nan
        refused(K.ERR_BAD_ARG, f.set_particles, bad)
        refused(K.ERR_BAD_ARG, f.set_particles, s, np.array([0.25, -0.25, 0.5, 0.5], F))
        refused(K.ERR_BAD_ARG, f.set_particles, s, np.array([0.25, np.inf, 0.5, 0.5], F))
        p0 = Cs.probability(4, "normalised")
        f.set_particles(s, p0, z)
        refused(K.ERR_BAD_ARG, f.resample, 1.0, np.zeros((4, 10), F))
        refused(K.ERR_BAD_ARG, f.resample, -0.1, np.zeros((4, 10), F))
        refused(K.ERR_BAD_ARG, f.measure, np.array([1, -1, 1, 1], F))
        refused(K.ERR_BAD_ARG, f.measure, np.array([1, np.nan, 1, 1], F))
        refused(K.ERR_BAD_ARG, f.measure, None, np.ones(4, F))                                    # quality without likelihood
        refused(K.ERR_STATE, f.measure)                                                           # no observation configuration
        refused(K.ERR_BAD_ARG, f.predict, Cs.ODOM_PREV, Cs.ODOM_CUR, float("nan"))
        f.n = 3
        refused(K.ERR_BAD_ARG, f.set_noise, np.zeros((3, 4), F))
        refused(K.ERR_BAD_ARG, f.add_noise, np.zeros((3, 10), F))
        refused(K.ERR_BAD_ARG, f.measure, np.ones(3, F))
        f.n = 4
        assert_set(f, s, p0, z, "after the refusals")
        # beside a pending tick
        sc = scenes.bench_scene("C2")
        p.set_cloud(sc.cloud)
        p.setPlan(sc.plan)
        p.tick_begin(sc.theory.name.decode(), sc.tick)
        try:
            for call in (f.particles, f.reset_integ, lambda: f.predict(Cs.ODOM_PREV, Cs.ODOM_CUR, 0.1), lambda: f.set_noise(z),
                         lambda: f.measure(np.ones(4, F)), lambda: f.resample(0.5, np.zeros((4, 10), F)),
                         lambda: f.add_noise(np.zeros((4, 10), F)), lambda: f.set_particles(s),
                         lambda: localization.ParticleFilter(p, filter_config(max_particles=64))):
                refused(K.ERR_STATE, call)
        finally:
            p.tick_end()
        assert_set(f, s, p0, z, "after the tick")
        localization.ParticleMeasure(p, mcl_config(max_particles=64))                            # a second mcl_create drops the filter
        refused(K.ERR_STATE, f.particles)
