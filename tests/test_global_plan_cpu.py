"""CPU tests of the pre-graph global planner's restatement, cases and pure arithmetic: the conditions the GPU tests
(tests/test_global_plan_gpu.py) rest on.  The restatement (tests/helpers/global_plan_ref.py) is pinned to the reference's
own compiled planner by tests/test_global_plan_pin_cpu.py, see there."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import global_plan_ref as G  # noqa: E402
import global_plan_cases as Cs  # noqa: E402

CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
F = np.float32
D = np.float64


def test_struct_sizes_and_constants():
    """the two structs the sizeof table does not know (global_plan.hip.h pins the same numbers with a static_assert)"""
    assert C.sizeof(K.GlobalPlanConfig) == 48 and C.sizeof(K.GlobalPlanResult) == 32
    assert (K.GLOBAL_PLAN_FOUND, K.GLOBAL_PLAN_NO_PATH, K.GLOBAL_PLAN_BUDGET, K.GLOBAL_PLAN_OPEN_FULL) == (G.FOUND, G.NO_PATH, G.BUDGET, G.OPEN_FULL)
    assert K.GLOBAL_PLAN_NONE == G.NONE and K.STACK_START == Cs.STACK_START
    text = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    for name, v in (("MAX_QUERIES", K.GLOBAL_PLAN_MAX_QUERIES), ("FOUND", 0), ("NO_PATH", 1), ("BUDGET", 2), ("OPEN_FULL", 3)):
        assert f"#define DDDMR_GLOBAL_PLAN_{name} {v}\n" in text, name


def test_cases_hold_what_the_gpu_tests_rely_on():
    found = Cs.check_cases()
    print(found)
    labels = [q[0] for q in Cs.queries()]
    assert len(set(labels)) == len(labels)
    want = {"same": G.FOUND, "goal_lone": G.NO_PATH, "goal_in_disc": G.NO_PATH, "start_in_disc": G.FOUND, "hole": G.FOUND, "ramp": G.FOUND,
            "start_lone": G.NO_PATH, "start_in_pocket": G.NO_PATH}
    for k, v in want.items():
        assert Cs.reference(k)["status"] == v, k
    # the two older no-path queries end on a set emptied by discards, where the reference has no defined answer; the two
    # newer ones end on a set that a pop of an open node left empty (a_star_on_pre_graph.cpp:213), where it has
    assert found["no_path_defined"] == 2 and found["no_path_on_emptied_set"] == 2
    assert Cs.reference("goal_lone")["ended_on_emptied_set"] and Cs.reference("goal_in_disc")["ended_on_emptied_set"]
    lone, pocket = Cs.reference("start_lone"), Cs.reference("start_in_pocket")
    assert (lone["n_expanded"], lone["n_pushed"], lone["n_discarded_closed"], lone["set_size"]) == (1, 1, 0, 0)
    assert 1 < pocket["n_expanded"] < 10 and pocket["stats"]["updates"] == 0 and pocket["n_discarded_closed"] == 0 and pocket["set_size"] == 0
    same = Cs.reference("same")
    assert len(same["path"]) == 1 and same["n_expanded"] == 1                      # start == goal: one node after one expansion
    # the start inside the disc is lethal itself; the goal inside it is never entered
    fl = Cs.case("floor")
    q = {x[0]: x for x in Cs.queries()}
    assert fl["dgraph"][q["start_in_disc"][2]] < 0.5 and fl["dgraph"][q["goal_in_disc"][3]] < 0.5
    # the disc forces a detour: without it the corner path is cheaper
    free = Cs.run(q["corner_tw0.0"], dgraph=np.minimum(Cs.static_ref("floor")["dgraph"], Cs.STACK_START))
    assert free["status"] == G.FOUND and free["g_goal"] < Cs.reference("corner_tw0.0")["g_goal"]
    # every path is a walk along kept edges from start to goal
    for lab in labels:
        r, qq = Cs.reference(lab), q[lab]
        if r["status"] != G.FOUND:
            assert len(r["path"]) == 0
            continue
        g = Cs.static_ref(qq[1])
        assert r["path"][0] == qq[2] and r["path"][-1] == qq[3]
        for a, b in zip(r["path"][:-1], r["path"][1:]):
            row = g["neighbour"][g["row_start"][a]: g["row_start"][a + 1]]
            assert b in row, lab


def _moved(fn, ulps):
    def f(x):
        y = np.asarray(fn(x), D)
        for _ in range(abs(ulps)):
            y = np.nextafter(y, D(np.inf) if ulps > 0 else D(-np.inf))
        return y
    return f


@pytest.mark.parametrize("label", [q[0] for q in Cs.queries()])
def test_cases_do_not_hang_on_the_last_bits_of_exp_and_acos(label):
    """Every exp result moved by +2 and by -2 double ulps, and the double acos likewise before its rounding to float: the
    same path, status and counters.  A condition on the committed inputs (two libraries of at most 1 ulp each can differ
    by 2), not a tolerance: the GPU tests compare bit for bit."""
    q = {x[0]: x for x in Cs.queries()}[label]
    ref = Cs.reference(label)
    for kw in (dict(exp=_moved(np.exp, 2)), dict(exp=_moved(np.exp, -2)), dict(acos=_moved(np.arccos, 2)), dict(acos=_moved(np.arccos, -2))):
        got = Cs.run(q, **kw)
        assert got["status"] == ref["status"], kw
        assert got["path"].tolist() == ref["path"].tolist(), kw
        assert (got["n_expanded"], got["n_pushed"], got["n_discarded_closed"]) == (ref["n_expanded"], ref["n_pushed"], ref["n_discarded_closed"]), kw
        assert F(got["g_goal"]).view(np.uint32) == F(ref["g_goal"]).view(np.uint32), kw


def test_restatement_against_an_independent_search():
    """turning_weight 0 and zero weights: the cost of the restatement's path against a plain best-first search in double
    (path cost only: a sanity check of the restatement, not a pin)"""
    q = {x[0]: x for x in Cs.queries()}
    for lab in ("corner_tw0.0", "lattice_row_tw0"):
        qq = q[lab]
        c = Cs.case(qq[1])
        want = G.dijkstra_cost(Cs.static_ref(qq[1]), c["ground"], c["dgraph"], Cs.plan_cfg(qq), qq[2], qq[3])
        got = float(Cs.reference(lab)["g_goal"])
        assert np.isfinite(want) and abs(got - want) <= 1e-4 * want, (lab, got, want)
    qq = q["goal_lone"]
    c = Cs.case(qq[1])
    assert G.dijkstra_cost(Cs.static_ref(qq[1]), c["ground"], c["dgraph"], Cs.plan_cfg(qq), qq[2], qq[3]) == float("inf")


def test_limits_of_the_restatement():
    q = {x[0]: x for x in Cs.queries()}["corner_tw0.1"]
    c = Cs.case(q[1])
    r = G.plan(Cs.static_ref(q[1]), c["ground"], c["dgraph"], None, Cs.plan_cfg(q, max_expansions=10), q[2], q[3])
    assert r["status"] == G.BUDGET and r["n_expanded"] == 10 and len(r["path"]) == 0
    r = G.plan(Cs.static_ref(q[1]), c["ground"], c["dgraph"], None, Cs.plan_cfg(q, max_open_entries=16), q[2], q[3])
    assert r["status"] == G.OPEN_FULL and len(r["path"]) == 0


def test_nearest_and_probe_restatement_edges():
    g = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [3, 0, 0]], F)
    ids = G.nearest(g, [[0.5, 0, 0], [0.25, 0, 0], [1.0, 0.1, 0], [2.0, 0, 0], [3.4999, 0, 0]])
    assert ids.tolist() == [G.NONE, 0, 1, G.NONE, 3]                           # exactly 0.5 m is outside; equal distances: the lowest index
    cnt, blocked = G.probe(g, np.array([1.0, 0.2, 1.0, 1.0, 9.0]), [[1.1, 0, 0], [0.25, 0, 0], [0.2, 0, 0]], 0.5)
    assert cnt.tolist() == [2, 0, 1] and blocked.tolist() == [True, False, False]


# ---- the plan header's pure functions through a stand-alone C++ program ----
def _hex(v):
    v = np.asarray(v)
    return "%08x" % int(v.astype(F).view(np.uint32)) if v.dtype != D else "%016x" % int(v.view(np.uint64))


def _lines():
    rng = np.random.default_rng(3)
    L, want = [], []
    # keys: order against std::set, negative f, -inf, equal f (index decides), equal pairs (collapse)
    fs = np.concatenate([rng.uniform(-5, 5, 24), [0.0, 1.5, 1.5, 1.5, -2.25, -2.25, np.inf, -np.inf, 1e-45, -1e-45, 3e38, -3e38]]).astype(F)
    idx = rng.integers(0, 1 << 24, len(fs))
    pairs = list(zip(fs.tolist(), idx.tolist())) + [(float(fs[3]), int(idx[3])), (1.5, 0), (1.5, 0xFFFFFFFE)]
    L.append("O " + " ".join(f"{_hex(F(f))}:{i}" for f, i in pairs))
    order = " ".join(str(i) for _, i in sorted(set(pairs)))
    want.append(f"O {order} | {order}")
    for f, i in ((1.5, 7), (-0.75, 123456), (0.0, 0)):
        L.append(f"K {_hex(F(f))} {i}")
        hi = int(F(f).view(np.uint32))
        hi = (~hi & 0xFFFFFFFF) if hi & 0x80000000 else hi | 0x80000000
        want.append("K %016x %s %d" % ((hi << 32) | i, _hex(F(f)), i))
    # theta: a straight line, a right angle, a small angle under the cap, a zero vector on either side, |vx1| == |vx2|
    for p in ([0, 0, 1, 0, 2, 0], [0, 0, 1, 0, 1, 1], [0, 0, 1, 0, 2, 0.2], [0, 0, 0, 0, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 1, 0.5, 2, -3],
              [0.3, 0.1, 1.7, 0.9, 1.1, 2.4], [4000.25, -3000.5, 4000.5, -3000.25, 4000.5, -2999.75]):
        p = np.array(p, F)
        L.append("T " + " ".join(_hex(v) for v in p))
        vx1, vy1, vx2, vy2 = F(p[2] - p[0]), F(p[3] - p[1]), np.array([p[4] - p[2]], F), np.array([p[5] - p[3]], F)
        c = G.cos_theta(vx1, vy1, vx2, vy2)
        with np.errstate(invalid="ignore"):
            th = G.theta_rules(vx1, vy1, vx2, vy2, np.arccos(c.astype(D)))
        want.append(f"T {_hex(c[0])} {_hex(D(th[0]))}")
    for _ in range(6):
        g, w, i = F(rng.uniform(0, 30)), F(rng.uniform(0, 1)), F(rng.uniform(0, 0.3))
        fac, th, tw = D(rng.uniform(0, 1)), D(rng.uniform(0.35, 3.1)), D(0.1)
        L.append(f"G {_hex(g)} {_hex(w)} {_hex(fac)} {_hex(th)} {_hex(tw)} {_hex(i)}")
        want.append("G " + _hex(G.new_g(g, np.array([w]), np.array([fac]), np.array([th]), tw, i)[0]))
    for w, r, d, ins in ((0.5, 0.5, 3.0, 0.5), (np.nextafter(F(0.5), F(1)), 0.5, 3.0, 0.5), (0.3, 0.5, 0.49, 0.5), (0.3, 0.5, 0.5, 0.5), (0.3, 0.5, 99999.9, 0.5)):
        L.append(f"E {_hex(F(w))} {_hex(D(r))} {_hex(D(d))} {_hex(D(ins))} {_hex(D(2.0))}")
        want.append("E %d %s" % (int(D(F(w)) > r or d < ins), _hex(D(np.exp(-1.0 * D(2.0) * (D(d) - D(ins)))))))
    for rec in ("1 1 3f800000 40000000 3f000000 3fc00000", "0 0 00000000 00000000 3f800000 40000000", "0 1 3f800000 40000000 3f800000 40000000",
                "0 1 3f800000 40000000 3f000000 3fc00000", "0 1 3f800000 40000000 3f7fffff 40000000"):
        L.append("F " + rec)
    want += ["F 0", "F 2", "F 0", "F 2", "F 1"]
    a, b = np.array([4000.1, -3000.2, 100.3], F), np.array([4003.7, -2999.1, 100.9], F)
    L.append("D " + " ".join(_hex(v) for v in np.concatenate([a, b])))
    want.append("D " + _hex(G.dist(a, b)))
    return L, want


def _build(tmp, *flags):
    exe = os.path.join(tmp, "global_plan_plan_test")
    r = subprocess.run([CXX, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "global_plan_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _check(exe):
    L, want = _lines()
    r = subprocess.run([exe], input="\n".join(L) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for g, w, l in zip(got, want, L):
        assert g == w, (l, g, w)


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_plan_header_against_the_restatement():
    with tempfile.TemporaryDirectory() as tmp:
        _check(_build(tmp))


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_plan_header_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        _check(_build(tmp, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
