"""Lone-point collision tests of the tick: every cloud of tests/helpers/needle_cases.py is ONE needle that decides the
verdict (plus four far points and, in some cases, a crowd just outside the needle's face), so that one candidate lost by
k_bin_count / k_bin_scatter or by k_score's candidate search is one wrong verdict -- on the dense clouds of the other
GPU tests a neighbour in the same cuboid gives the same -1.  The expectation is the helper's float64 box test over every
step and point (pinned on the oracle by tests/test_needle_cpu.py); for c3 it is oracle.tick's, per needle."""
import json
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd.local_planner import LocalPlanner
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import needle_cases as N  # noqa: E402

pytestmark = pytest.mark.gpu
# every tick starts from poisoned per-trajectory outputs (see tests/test_random_gpu.py)
os.environ["DDDMR_POISON"] = "1"

ALL = [s.name for s in N.SCENES]
# launch shapes and hand-off paths that must change nothing
FORCED = [{"DDDMR_NO_TAB": "1"}, {"DDDMR_GNZ_ONE": "1"}, {"DDDMR_NO_BOXFAST": "1"}, {"DDDMR_CELL": "0.2"}, {"DDDMR_CELL": "0.5"},
          {"DDDMR_TILE": "3"}, {"DDDMR_THREADS": "256"}, {"DDDMR_PROBE": "0"}, {"DDDMR_PROBE": "1"}, {"DDDMR_RT": "7"}]
FORCED_C3 = FORCED + [{"DDDMR_TAIL_ROUND": "1"}, {"DDDMR_FINAL": "0"}]

# per scene: needles, compared (trajectory, needle) pairs, needle-decided trajectories, fragile exemptions; written to
# parity_stats_needle.json beside the random suite's statistics at the end of the module, quoted in DESIGN.md section 5
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_stats():
    yield
    out = _stats_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_stats_needle.json"), "w") as f:
        json.dump(STATS, f, indent=1)
    print("\n[parity stats, needle suite]", json.dumps(STATS))


def _stats_dir():
    """the checkout's ignored output directory (`..._out/` in .gitignore), where tests/test_random_gpu.py writes
    parity_stats_random.json"""
    with open(os.path.join(ROOT, ".gitignore")) as f:
        names = [ln.strip().rstrip("/") for ln in f if ln.strip().endswith("_out/")]
    assert len(names) == 1, names
    return os.path.join(ROOT, names[0])


def _last_argmin(costs):
    best, m = -1, 9999999.0
    for i, c in enumerate(costs):
        if c >= 0 and c <= m:
            best, m = i, c
    return best


def _planner(sc):
    kw = dict(max_trajectories=1 << 15) if sc.big else {}
    return LocalPlanner([sc.theory], max_points=64, max_steps=512, **kw)


def _run(name, which, ticks=1):
    """one LocalPlanner for the scene; per needle set_cloud, tick (`ticks` times), debug() -> [needle][tick] outputs"""
    sc, nds = N.BY_NAME[name], N.needles(name)
    out = []
    with _planner(sc) as lp:
        lp.setPlan(sc.plan)
        for n in which:
            lp.set_cloud(nds[n].cloud)
            per = []
            for _ in range(ticks):
                res = lp.tick("t", sc.tick)
                costs, steps, smp = (a.copy() for a in lp.debug())
                per.append((res.best_index, res.best_cost, (res.vx, res.vy, res.wz), res.key, costs, steps, smp))
            out.append(per)
    return out


def _expected(name, n):
    """-> (costs, steps, samples, fragile, decided) of needle n"""
    if N.BY_NAME[name].big:
        o, decided = N.c3_expected(n)
        return o.costs, o.steps, o.samples, np.abs(o.min_margin) < N.BY_NAME[name].band, decided
    v = N.verdict(name, N.needles(name)[n])
    g = N.geo(name)
    return N.expected_costs(name, v), g.steps, g.samples, v.fragile, v.decided


def _spread(name, k):
    return [int(v) for v in np.unique(np.linspace(0, len(N.needles(name)) - 1, k).astype(int))]


@pytest.mark.parametrize("name", ALL)
def test_every_needle_decides_its_verdicts(name):
    nds = N.needles(name)
    got = _run(name, range(len(nds)))
    st = STATS[name] = dict(needles=len(nds), pairs=0, needle_decided=0, exempt=0, crowded_needles=0, fewest_decided_with_a_crowd=None)
    for n, nd in enumerate(nds):
        bi, bc, _, _, costs, steps, smp = got[n][0]
        want, want_steps, want_smp, fragile, decided = _expected(name, n)
        where = (name, n, nd.kind, nd.i, nd.s, nd.crowd)
        np.testing.assert_array_equal(steps, want_steps, err_msg=str(where))
        np.testing.assert_array_equal(smp, want_smp, err_msg=str(where))
        assert not np.isnan(costs).any(), where
        neg = (costs < 0) | (want < 0)
        bad = neg & (costs != want) & ~fragile
        assert not bad.any(), (where, np.nonzero(bad)[0][:5], costs[bad][:5], want[bad][:5])
        both = (costs >= 0) & (want >= 0)
        if both.any():
            assert float(np.max(np.abs(costs[both] - want[both]))) <= N.TOL, where
        # exact by construction: the winner is the last exact minimum of the engine's own costs
        assert bi == _last_argmin(costs), where
        if bi >= 0:
            assert bc == costs[bi], where
        st["pairs"] += int((want_steps > 0).sum())
        st["exempt"] += int(fragile.sum())
        st["needle_decided"] += int(decided.sum())
        if nd.crowd:
            assert decided.any(), where
            st["crowded_needles"] += 1
            k = int(decided.sum())
            st["fewest_decided_with_a_crowd"] = k if st["fewest_decided_with_a_crowd"] is None else min(k, st["fewest_decided_with_a_crowd"])
    st["exempt_share"] = st["exempt"] / st["pairs"]
    print(name, json.dumps(st))
    assert st["exempt"] <= N.MAX_SHARE * st["pairs"]
    assert st["needle_decided"] > 0


@pytest.mark.parametrize("name", ALL)
def test_a_second_tick_changes_nothing(name):
    """every fifth needle ticked twice: the second tick deals the trajectories by the load the first one measured and
    chooses its probe by the first one's collided share; costs, steps and key must not move by a bit"""
    for per in _run(name, range(0, len(N.needles(name)), 5), ticks=2):
        (bi0, bc0, v0, k0, c0, s0, m0), (bi1, bc1, v1, k1, c1, s1, m1) = per
        assert (bi1, bc1, k1) == (bi0, bc0, k0) and tuple(v1) == tuple(v0)
        np.testing.assert_array_equal(c1, c0)
        np.testing.assert_array_equal(s1, s0)
        np.testing.assert_array_equal(m1, m0)


@pytest.mark.parametrize("name", ["dd55", "omni275_long", "jitter_mm", "c3"])
def test_forced_shapes_change_no_needle(name):
    """60 needles (c3: all of its) again under every forced launch shape, set at create time: bit-equal to the default"""
    which = range(len(N.needles(name))) if N.BY_NAME[name].big else _spread(name, 60)
    base = _run(name, which)
    for env in (FORCED_C3 if N.BY_NAME[name].big else FORCED):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            got = _run(name, which)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        for n, b, g in zip(which, base, got):
            (bi, bc, bv, bk, c0, s0, m0), (gi, gc, gv, gk, c1, s1, m1) = b[0], g[0]
            assert (gi, gc, gk) == (bi, bc, bk) and tuple(gv) == tuple(bv), (env, n)
            np.testing.assert_array_equal(c1, c0, err_msg=str((env, n)))
            np.testing.assert_array_equal(s1, s0, err_msg=str((env, n)))
            np.testing.assert_array_equal(m1, m0, err_msg=str((env, n)))
