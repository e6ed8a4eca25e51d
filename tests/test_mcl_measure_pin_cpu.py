"""The pin of the particle-measure restatement (tests/helpers/mcl_measure_ref.py) to mcl_3dl's own
LidarMeasurementModelLikelihood::measure and State6DOF::transform, compiled from a reference checkout against the
stand-ins of oracle/ref/shim/ (oracle/ref/ref_mcl_driver.cpp, `make -C oracle ref`).

Live part (skipped where oracle/_ref/libref_mcl_*.so is absent): transform on bits; every case on bits against the O0
build -- quality, the match count recovered from it, the ground count, the branch, the float averages of the normals,
roll and roll_diff as doubles, the likelihood (Python's math functions and the O0 build call the same glibc functions
separately); the O2 build within the reference's own O0-to-O2 gap, which is measured here over all the pin's particles
and not fixed in advance (measured: at most 154 double ulp of roll, on 4 of 2286 rolls, 6.7e-17 on a roll of -0.0035;
0 float ulp of likelihood).

Golden part (runs everywhere): the inputs rebuilt from the case generators hash to what tests/golden/REF_MCL_*.npz
were computed from, and the restatement reproduces the stored O2 answers within the stored gap.

The targeted cases' own conditions (which side of which decision each particle sits on) are asserted from the
restatement's reports alone."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcl_measure_ref as R  # noqa: E402
import mcl_measure_cases as Cs  # noqa: E402
import mcl_measure_pin_cases as Pc  # noqa: E402
import mcl_measure_golden as G  # noqa: E402
from oracle import ref_mcl_py as M  # noqa: E402

F = np.float32
IDS = [f"{f[8:]}:{n}" if len(G.FILES[f][0]) > 1 else n for f, n in G.CASES]

live = pytest.mark.skipif(not M.available(), reason="oracle/_ref/libref_mcl_O0.so / libref_mcl_O2.so are absent (no compiled "
                          "reference): run `make -C oracle ref REFERENCE=<checkout>`")


def b32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same64(a, b):
    """equal on bits, or both NaN (a NaN's sign and payload say nothing)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (b64(a) == b64(b)) | (np.isnan(a) & np.isnan(b))


_runs: dict = {}


def reference(file, name, build):
    if (file, name, build) not in _runs:
        cfg, parts, _, _ = G.load_case(file, name)
        _runs[(file, name, build)] = M.measure(cfg, parts["map"], parts["ground"], parts["normals"], parts["flat"], parts["ls"],
                                               parts["states"], build)
    return _runs[(file, name, build)]


def n_obs(parts):
    return len(parts["flat"]) + len(parts["ls"])


def assert_restatement(ref, parts, got, what, gap_roll=0, gap_like=0):
    """ref: the restatement's answer; got: the compiled reference's (or a golden's) likelihood, quality, trace, branch"""
    assert int(ref["n_fragile"].sum()) == 0 and int(ref["n_tied"].sum()) == 0 and ref["n_bad"] == 0, what
    tr, br = got["trace"], got["branch"]
    np.testing.assert_array_equal(b32(ref["quality"]), b32(got["quality"]), err_msg=what + ": quality")
    # num / n_obs in float recovers num: |error| <= num * 2^-24 * n_obs / n_obs < 0.5 for n_obs <= 2000
    n_match = np.rint(got["quality"].astype(np.float64) * n_obs(parts)).astype(np.int64)
    np.testing.assert_array_equal(ref["n_match"], n_match, err_msg=what + ": match count")
    np.testing.assert_array_equal(ref["n_ground"], tr[:, 0], err_msg=what + ": ground neighbours")
    np.testing.assert_array_equal(Pc.branch(ref), br, err_msg=what + ": branch")
    h, chain = br > 0, br == 2
    assert np.isnan(tr[~h, 1:]).all() and np.isnan(tr[br == 1, 4:]).all(), what
    avg = tr[h, 1:4].astype(np.float32)
    assert (avg.astype(np.float64) == tr[h, 1:4]).all() or np.isnan(tr[h, 1:4]).any(), what      # floats widened to double
    np.testing.assert_array_equal(b32(ref["avg"][h]), b32(avg), err_msg=what + ": averaged normals")
    assert not np.isnan(tr[chain, 7]).any(), what
    if gap_roll == 0:
        assert same64(ref["roll"][chain], tr[chain, 4]).all(), (what + ": roll", ref["roll"][chain], tr[chain, 4])
        assert same64(ref["roll_diff"][chain], tr[chain, 7]).all(), (what + ": roll_diff", ref["roll_diff"][chain], tr[chain, 7])
    else:
        assert G.ulps64(ref["roll"][chain], tr[chain, 4]).max(initial=0) <= gap_roll, what + ": roll"
    if gap_like == 0:
        np.testing.assert_array_equal(b32(ref["likelihood"]), b32(got["likelihood"]), err_msg=what + ": likelihood")
    else:
        assert G.ulps32(ref["likelihood"], got["likelihood"]).max(initial=0) <= gap_like, what + ": likelihood"


# ---- 3a: State6DOF::transform --------------------------------------------------------------------------------------

def transform_inputs():
    rng = np.random.default_rng(20)
    n, m = 400, 260                                                   # 104 000 point-state pairs
    rpy = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-math.pi, math.pi, n)], axis=1)
    rpy[:8, 2] = [math.pi, -math.pi, np.nextafter(math.pi, 0), -np.nextafter(math.pi, 0), math.pi, -math.pi, math.pi, -math.pi]
    rpy[4:8, :2] = [[0.5, 0.5], [-0.5, 0.5], [0.5, -0.5], [-0.5, -0.5]]
    rpy[8:12] = 0.0
    states = np.zeros((n, 7))
    states[:, 3:] = [Cs.quat_rpy(*a) for a in rpy]
    states[:, 3:] *= np.concatenate([[0.5, 2.0, 1.0, 1.0], rng.uniform(0.5, 2.0, n - 4)])[:, None]
    states[:, :3] = rng.uniform(-1, 1, (n, 3)) * [5, 5, 1]
    far = rng.random(n) < 0.5
    states[far, :3] += Cs.SHIFT.astype(np.float64)
    states[12, :3] = Cs.SHIFT
    pts = rng.uniform(-30, 30, (m, 3)) * [1, 1, 0.2]
    pts[:4] = [[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, 1]]
    return pts.astype(F), states.astype(F)


@live
@pytest.mark.parametrize("build", M.BUILDS)
def test_transform_on_bits(build):
    """raw quaternions of norm 0.5 to 2, yaw at +-pi, roll and pitch to 0.5 rad, positions out to (3000, -7000, 40)"""
    pts, states = transform_inputs()
    norms = np.linalg.norm(states[:, 3:].astype(np.float64), axis=1)
    assert len(pts) * len(states) >= 100_000 and norms.min() < 0.51 and norms.max() > 1.99
    assert (np.abs(states[:, :3]).max(axis=0) >= np.abs(Cs.SHIFT)).all()
    want = M.transform(pts, states, build)
    got = R.transform(states[:, :3], states[:, 3:], pts)
    assert np.isfinite(want).all()
    np.testing.assert_array_equal(b32(got), b32(want))


# ---- 3b, 3d: every case against the O0 build, on bits ----------------------------------------------------------------

@live
@pytest.mark.parametrize("file,name", G.CASES, ids=IDS)
def test_case_against_the_O0_build_on_bits(file, name):
    cfg, parts, ref, _ = G.load_case(file, name)
    got = reference(file, name, "O0")
    assert_restatement(ref, parts, got, name)
    assert b32(got["quality_min"]) == b32(ref["quality_min"]) and b32(got["quality_max"]) == b32(ref["quality_max"]), name


# ---- 3c: the reference's own O0-to-O2 gap, measured, and the restatement against O2 within it ----------------------------

@live
def test_O2_build_within_the_references_own_gap():
    gap_roll = gap_like = n = 0
    for file, name in G.CASES:
        o0, o2 = reference(file, name, "O0"), reference(file, name, "O2")
        for k in ("quality", "branch"):
            assert o0[k].tobytes() == o2[k].tobytes(), (name, k)               # counts, branches, quality: identical
        assert o0["trace"][:, 0].tobytes() == o2["trace"][:, 0].tobytes(), name
        assert b32(o0["trace"][:, 1:4].astype(F)).tobytes() == b32(o2["trace"][:, 1:4].astype(F)).tobytes(), name
        gap_roll = max(gap_roll, int(G.ulps64(o0["trace"][:, 4], o2["trace"][:, 4]).max(initial=0)))
        gap_like = max(gap_like, int(G.ulps32(o0["likelihood"], o2["likelihood"]).max(initial=0)))
        n += len(o0["likelihood"])
    print(f"{n} particles: O0 to O2 at most {gap_roll} double ulp of roll, {gap_like} float ulp of likelihood")
    for file, name in G.CASES:
        cfg, parts, ref, _ = G.load_case(file, name)
        assert_restatement(ref, parts, reference(file, name, "O2"), name + " (O2)", gap_roll, gap_like)
    stored = G.read(*G.CASES[0])
    assert (stored["gap_roll_ulp"], stored["gap_like_ulp"]) == (gap_roll, gap_like), \
        "the goldens were written with another O0-to-O2 gap: regenerate them with tests/golden/make_ref_mcl_golden.py"


# ---- 4: the goldens (no reference needed) -------------------------------------------------------------------------------

@pytest.mark.parametrize("file,name", G.CASES, ids=IDS)
def test_restatement_reproduces_the_golden(file, name):
    cfg, parts, ref, draws = G.load_case(file, name)
    stored = G.read(file, name)
    G.check_inputs(file, name, parts, stored)
    assert int(stored["draws"]) == draws and stored["cfg"].tobytes() == G.cfg_array(cfg).tobytes(), name
    assert_restatement(ref, parts, stored, name + " (golden)", stored["gap_roll_ulp"], stored["gap_like_ulp"])
    assert b32(stored["quality_minmax"]).tolist() == [b32(ref["quality_min"]), b32(ref["quality_max"])], name


@live
@pytest.mark.parametrize("file", list(G.FILES))
def test_goldens_are_the_O2_builds_answers(file):
    for name in G.FILES[file][0]:
        stored, got = G.read(file, name), reference(file, name, "O2")
        for k in ("likelihood", "quality", "trace", "branch"):
            assert stored[k].tobytes() == got[k].tobytes(), f"{file}: {name}: {k}: regenerate with tests/golden/make_ref_mcl_golden.py"


# ---- 3d: what the targeted cases hold, from the restatement's reports alone -------------------------------------------------

def test_ground_counts_around_the_threshold():
    for name, thr in (("counts-5-6-7", 6), ("counts-2-3-4-threshold-3", 3)):
        cfg, _, ref, _ = Pc.case(name)
        assert cfg.threshold_for_trusted_ground == thr and ref["n_ground"].tolist() == [thr - 1, thr, thr + 1]
        assert ref["healthy"].tolist() == [False, True, True]


def test_three_times_test_from_both_sides():
    """24 patches: x and y, both signs, 1 to 3 float steps either side of |avg| = 3 |avg_nz|"""
    _, parts, ref, _ = Pc.case("three-times")
    steep = np.isnan(ref["roll_diff"]).reshape(4, 6)
    avg = ref["avg"].astype(np.float64).reshape(4, 6, 3)
    assert ref["healthy"].all() and steep.any(axis=1).all() and (~steep).any(axis=1).all()
    for v, axis in enumerate((0, 0, 1, 1)):
        m = np.abs(avg[v, :, axis]) - 3.0 * np.abs(avg[v, :, 2])
        assert ((m >= 0) == steep[v]).all() and np.abs(m).max() < 5 * 2.0 ** -24 and np.abs(m).min() >= R.MARGIN
        assert (ref["pos_weight"].reshape(4, 6)[v][steep[v]] == F(0.2)).all()
    assert (avg[1, :, 0] < 0).all() and (avg[3, :, 1] < 0).all()


def test_negative_z_normals():
    _, parts, ref, _ = Pc.case("negative-z")
    nz = parts["normals"][:, 2].reshape(3, 6)
    assert (nz[0] < 0).all() and (nz[1] < 0).sum() == 3 and (nz[2] < 0).sum() == 1
    assert (ref["avg"][:, 2] > 0.9).all() and Pc.branch(ref).tolist() == [2, 2, 2]
    # without the fabs the second patch's average would fail the 3x test
    assert abs(float(nz[1].sum())) < 1e-6 and abs(float(ref["avg"][1, 0])) > 0.25


def test_rolls_in_every_band_and_beside_every_edge():
    _, _, ref, _ = Pc.case("rolls")
    roll, diff, targets = ref["roll"], ref["roll_diff"], Pc.roll_targets()
    assert len(roll) == len(targets) == 17 and (np.abs(roll - targets) < 5e-7).all() and (Pc.branch(ref) == 2).all()
    ar = np.abs(roll)
    first, second = (ar > 2.6) & (ar < 3.1415926), ar < 0.5
    assert first.sum() >= 6 and second.sum() >= 5 and (~first & ~second).sum() >= 6
    assert (diff[first] == 3.1415926 - ar[first]).all() and (diff[second] == ar[second]).all() and (diff[~first & ~second] == 0.55).all()
    for e in Pc.ROLL_EDGES:
        d = ar - e
        near = np.abs(d) < 1e-5
        assert (np.abs(d[near]) >= Pc.ROLL_MARGIN).all()
        assert (d[near] < 0).sum() == 2 and (d[near] > 0).sum() == (0 if e > 3 else 2)        # nothing fits between 3.1415926 and pi
    assert (roll[near] > 0).any() and (roll[near] < 0).any()


def test_up_normal_gives_a_nan_roll_and_0_55():
    _, _, ref, _ = Pc.case("up-normal")
    assert ref["avg"].tolist() == [[0, 0, 1], [0, 0, 1]] and np.isnan(ref["roll"]).all() and (ref["roll_diff"] == 0.55).all()
    assert (ref["pos_weight"] > 0.3).all()


def test_weights_that_go_negative_and_the_nearest_point_at_one():
    _, parts, ref, _ = Pc.case("far-floor")
    assert ref["healthy"].all() and Pc.branch(ref).tolist() == [2] and ref["pos_weight"].tolist() == [F(0.01)]
    assert R.l2(parts["ground"], parts["states"][0, :3]).min() > 1.4 and ref["n_match"][0] > 0 and ref["likelihood"][0] > 0
    _, parts, ref, _ = Pc.case("untrusted-nn-just-beyond-one")
    d2 = R.l2(parts["map"], parts["states"][0, :3])[0]
    assert not ref["healthy"][0] and F(1) < d2 < R.NN_D2 and ref["pos_weight"].tolist() == [F(0.01)] and ref["n_match"][0] == 2
    _, parts, ref, _ = Pc.case("trusted-nn-at-one")
    assert R.l2(parts["ground"], parts["states"][0, :3]).min() == F(1) and Pc.branch(ref).tolist() == [2]
    assert ref["pos_weight"].tolist() == [F(0.0)]
    _, parts, ref, _ = Pc.case("trusted-nn-one-float-above-one")
    assert R.l2(parts["ground"], parts["states"][0, :3]).min() == np.nextafter(F(1), F(2)) and Pc.branch(ref).tolist() == [2]
    assert ref["pos_weight"].tolist() == [F(0.0)]                          # sqrtf of the float above 1 is 1


def test_flat_loop_edges_in_both_trees():
    """one float inside match_dist_min matches, on it and above it do not; below match_dist_flat the term is that of
    match_dist_flat; a flat point with no neighbour does not inherit the previous one's; intensities 0.5, 1 and 3"""
    mdm, mdf = F(0.3), F(0.05)
    term = lambda d: F(F(mdm - max(F(d), mdf)) * F(mdm - max(F(d), mdf)))
    score = F(0)
    for t in (term(np.nextafter(mdm, F(0))), term(0.04), term(0.2), term(0.1)):
        score = F(score + t)
    for t, w in ((term(0.1), 0.5), (term(0.1), 1.0), (term(0.1), 3.0), (term(0.25), 1.7)):
        score = F(score + F(t / F(w)))
    assert term(0.04) == term(0.0) == F(F(0.25) * F(0.25))
    for name, healthy in (("flat-edges-on-ground", True), ("flat-edges-on-map-weight-one", False)):
        _, parts, ref, _ = Pc.case(name)
        assert parts["ls"][:, 3].tolist() == [0.5, 1.0, 3.0, F(1.7)]
        assert ref["healthy"].tolist() == [healthy] * 2 and ref["n_match"].tolist() == [8, 8], name
        assert b32(ref["score"]).tolist() == [b32(score)] * 2, name
    assert ref["pos_weight"].tolist() == [F(1), F(1)] and b32(ref["likelihood"]).tolist() == [b32(score)] * 2


def test_weight_one_room_isolates_the_score_sum():
    _, parts, ref, _ = Pc.case("weight-one-room")
    assert not ref["healthy"].any() and (ref["pos_weight"] == F(1)).all() and len(ref["score"]) == 20
    assert b32(ref["likelihood"]).tolist() == b32(ref["score"]).tolist() and ref["n_match"].min() >= 30 and len(set(b32(ref["score"]).tolist())) == 20


def test_random_rooms_cover_every_branch():
    n = np.zeros(3, np.int64)
    total = negative = 0
    for name in Pc.ROOMS:
        cfg, parts, ref, _ = Pc.case(name)
        assert len(parts["map"]) <= 3000
        n += np.bincount(Pc.branch(ref), minlength=3)
        total += len(ref["likelihood"])
        negative += int(((ref["pos_weight"] == F(0.01)) & ref["healthy"]).sum())
    print(f"{total} particles in {len(Pc.ROOMS)} rooms: untrusted / 3x / roll chain = {n.tolist()}, trusted with a negative weight {negative}")
    assert total == 2000 and n.min() >= 100
