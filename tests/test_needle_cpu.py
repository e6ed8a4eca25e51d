"""Without a GPU: the lone-point cases of tests/helpers/needle_cases.py pinned on the oracle alone, so that what
tests/test_needle_gpu.py expects of the device is what the oracle does.  The float64 box test over every step and point
gives oracle.tick's verdicts on every trajectory outside the band; every needle is what its class says (a needle meant
to collide makes its target a clear collision, a needle beyond the 1 m ball leaves it clear); fragile (trajectory,
needle) pairs stay under 0.5 % per scene; and a crowd never takes the decision from the needle on every trajectory."""
import collections
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import needle_cases as N  # noqa: E402
import oracle  # noqa: E402

PINNED = N.SMALL + N.SHIFTED


def test_the_scenes_are_the_shapes_they_are_named_after():
    assert [len(oracle.samples(N.BY_NAME[n].theory, N.BY_NAME[n].tick)) for n in ("dd55", "omni275_long", "rotate", "c3")] == [55, 275, 2, 16384]
    assert N.geo("rotate").steps.tolist() == [252, 252]                    # one long row per trajectory
    g = N.geo("omni275_long")
    assert np.linalg.norm(g.verts.astype(np.float64) - g.pose[:, None, :], axis=-1).max() > 1.3    # corners beyond the ball
    e = N.geo("jitter_mm").box.A[0]
    assert np.abs(e @ e.T - np.eye(3)).max() > 0.01                        # not a box: the general vertex path
    for name in N.SHIFTED:
        sc = N.BY_NAME[name]
        assert 2e-4 < sc.band < 1.2e-3 and sc.depth == 0.004 and np.abs(sc.shift).max() > 1000.0
    assert N.BY_NAME["dd55"].band == 1e-4 and N.BY_NAME["dd55"].depth == 0.002


@pytest.mark.parametrize("name", PINNED)
def test_every_class_and_crowd_size_is_there(name):
    nds = N.needles(name)
    kinds = collections.Counter(nd.kind for nd in nds)
    print(name, len(nds), dict(kinds))
    assert 250 <= len(nds) <= 340
    want = {"face-in", "face-out", "corner", "line"}
    if name == "omni275_long":
        want |= {"ball-in", "ball-out"}                 # (its front face lies beyond the ball: no tip there)
    else:
        want |= {"tip"}
    if name == "jitter_mm":
        want |= {"sliver", "aabb-in", "aabb-out"}
    assert want <= set(kinds) and kinds["line"] == N.LINE_N
    for kind in ("face-in", "corner"):
        assert {nd.crowd for nd in nds if nd.kind == kind} == set(N.CROWDS)
    assert {nd.crowd for nd in nds} == set(N.CROWDS)
    for nd in nds:
        assert nd.cloud.dtype == np.float32 and nd.cloud.shape == (5 + nd.crowd, 4)
        if nd.crowd:                                    # within 0.25 m of the needle in x and y (float rounding aside)
            assert np.abs(nd.cloud[5:, :2].astype(np.float64) - nd.cloud[0, :2]).max() <= 0.25 + 1e-3


@pytest.mark.parametrize("name", PINNED)
def test_float64_verdicts_are_the_oracles(name):
    r = N.pin(name)
    print(name, {k: v for k, v in r.items() if not isinstance(v, list)})
    n = len(N.needles(name))
    assert r["compared"] == ((n + 9) // 10 if name in N.SHIFTED else n)      # every tenth needle of the shifted scenes
    assert r["mismatch"] == []


@pytest.mark.parametrize("name", PINNED)
def test_every_needle_is_what_its_class_says(name):
    r = N.pin(name)
    assert r["bad_target"] == []
    assert sum(nd.expect == "collide" for nd in N.needles(name)) >= 80
    assert r["fewest_touched"] >= 1


@pytest.mark.parametrize("name", PINNED)
def test_fragile_pairs_stay_under_the_cap(name):
    r = N.pin(name)
    print(name, "fragile", r["fragile"], "of", r["pairs"])
    assert r["fragile"] <= N.MAX_SHARE * r["pairs"]


@pytest.mark.parametrize("name", PINNED)
def test_a_crowd_never_takes_every_decision_from_its_needle(name):
    r = N.pin(name)
    assert r["undecided"] == []
    assert r["decided"] > 0


def test_ball_needles_are_decided_by_the_radius_test():
    g = N.geo("omni275_long")
    pairs = [nd for nd in N.needles("omni275_long") if nd.kind.startswith("ball")]
    assert len(pairs) >= 8
    for nd in pairs:
        j = g.flat(nd.i, nd.s)
        p = nd.cloud[:1, :3].astype(np.float64)
        assert g.box.margin(p)[j, 0] < -0.01                               # well inside the step's box either way
        r = float(np.linalg.norm(p[0] - g.pose[j])) - 1.0
        assert abs(r - (0.005 if nd.kind == "ball-out" else -0.005)) < 1e-6


def test_sliver_needles_lie_outside_the_vertices():
    g = N.geo("jitter_mm")
    sl = [nd for nd in N.needles("jitter_mm") if nd.kind == "sliver"]
    assert len(sl) >= 9
    for nd in sl:
        j = g.flat(nd.i, nd.s)
        p = nd.cloud[0, :3].astype(np.float64)
        assert N._outside_hull(g.verts[j], p) and g.box.margin(p[None])[j, 0] <= -N.BY_NAME["jitter_mm"].depth + 1e-6


def test_c3_needles():
    sc = N.BY_NAME["c3"]
    nds = N.needles("c3")
    assert len(nds) == N.N_C3 and {nd.kind for nd in nds} == {"tip", "face-in", "face-out"}
    pairs = fragile = 0
    for n, nd in enumerate(nds):
        o, decided = N.c3_expected(n)
        pairs += len(o.costs)
        fragile += int((np.abs(o.min_margin) < sc.band).sum())
        if nd.expect == "collide":
            assert o.costs[nd.i] == -1.0 and o.min_margin[nd.i] <= -sc.band
        if nd.crowd:
            assert decided.any()
    assert fragile <= N.MAX_SHARE * pairs


def test_the_committed_seeds_are_what_find_seed_finds():
    for name in ("dd55", "dd55_far_b"):
        seed = N.BY_NAME[name].seed
        try:
            assert N.find_seed(name, tries=3) == seed
        finally:
            N.BY_NAME[name].seed = seed
            N._NEEDLES.pop(name, None)
            N._PIN.pop(name, None)
