"""The cases of the cloud planner's tests (tests/test_global_plan_cloud_cpu.py, tests/test_global_plan_cloud_gpu.py), from
fixed seeds.  A case is a dict: ground, map, cfg (the static layer's), lethal (the aggregate lethal cloud, duplicates
included), dgraph (what get_min_dGraphValue serves: the distance to the nearest lethal point, capped by the stack's start
value), intensity and node_weights (random), plan_cfg overrides and shift.  A query is (label, case, start, goal,
turning_weight, weighted, with_lethal).  check_cases() states what the cases have to contain for the GPU tests to prove
what they claim; the CPU test runs it.

floor: a 24 x 24 floor at 0.25 m with +-0.04 m of jitter (no equal distances), a 3-node island 2.5 m off and a lone node
6 m off.  Lethal: a wall of ground nodes across most of the floor, one isolated node, one node listed twice.  Every
coordinate is a multiple of 2^-10 m, so that the floor shifted by static_layer_cases.SHIFT has the same differences bit
for bit."""
from __future__ import annotations

import functools

import numpy as np

import global_plan_cloud_ref as R
import static_layer_cases as Sc
import static_layer_ref as Sr

F = np.float32
D = np.float64
STACK_START = 99999.9            # get_min_dGraphValue's start value (stacked_perception.cpp:116)
N_SIDE = 24


def _snap(a):
    return (np.round(np.asarray(a, D) * 1024.0) / 1024.0).astype(F)


def _dgraph(ground, lethal):
    g, l = np.asarray(ground, D), np.asarray(lethal, D).reshape(-1, 3)
    d = np.full(len(g), STACK_START) if len(l) == 0 else np.sqrt(((g[:, None, :] - l[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    return np.concatenate([np.minimum(d, STACK_START), [STACK_START]])


def _map(shift):
    rng = np.random.default_rng(21)
    m = np.stack([rng.uniform(0, 6, 100), rng.uniform(0, 6, 100), rng.uniform(2.0, 3.0, 100)], axis=1)
    return (m + shift).astype(F)


def node(ix, iy) -> int:
    return ix * N_SIDE + iy


def _floor(shift):
    rng = np.random.default_rng(5)
    xs, ys = np.meshgrid(np.arange(N_SIDE) * 0.25, np.arange(N_SIDE) * 0.25, indexing="ij")
    g = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1)
    g += rng.uniform(-0.04, 0.04, g.shape) * np.array([1.0, 1.0, 0.25])
    island = np.array([[8.25, 2.0, 0.0], [8.25, 2.27, 0.01], [8.47, 2.1, 0.0]])
    lone = np.array([[-6.0, 3.0, 0.0]])
    g = _snap(np.concatenate([g, island, lone]))
    wall = [node(12, iy) for iy in range(18)]
    lethal_ids = wall + [node(5, 20), node(18, 5), node(18, 5)]                # the wall, an isolated node, a node listed twice
    sh = np.asarray(shift, D)
    ground = (g.astype(D) + sh).astype(F)
    assert np.array_equal((ground.astype(D) - sh).astype(F), g)                # (the shift is exact)
    return ground, np.array(lethal_ids)


def _lattice():
    """an exact 0.25 m lattice, z = 0, with inscribed_radius 0.125: equal distances everywhere, and edges of exactly
    2 * inscribed_radius.  Lethal: two points (one listed twice) off the nodes, beside the middle of an edge."""
    xs, ys = np.meshgrid(np.arange(N_SIDE) * 0.25, np.arange(N_SIDE) * 0.25, indexing="ij")
    g = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1).astype(F)
    a = g[node(10, 10)]
    lethal = np.array([a + F([0.125, 0.1, 0.0]), a + F([0.125, 0.1, 0.0]), a + F([0.125, -0.1, 0.0]), g[node(4, 15)], g[node(4, 16)], g[node(4, 17)]], F)
    return g, lethal


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    rng = np.random.default_rng(9)
    shift = np.array(Sc.SHIFT if name == "floor_shifted" else (0.0, 0.0, 0.0))
    plan_cfg = {}
    if name in ("floor", "floor_shifted"):
        ground, ids = _floor(shift)
        lethal = ground[ids]
    elif name == "lattice":
        ground, lethal = _lattice()
        plan_cfg = dict(inscribed_radius=0.125)
    elif name == "cluster":
        # 1100 nodes inside one radius (ROW_FULL), and a few outside
        p = rng.normal(size=(1100, 3))
        p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(0.0, 0.2, (1100, 1)) * np.array([1.0, 1.0, 0.2])
        ground = _snap(np.concatenate([p + np.array([1.0, 1.0, 0.0]), np.array([[3.0 + 0.25 * i, 1.0, 0.0] for i in range(10)])]))
        lethal = np.zeros((0, 3), F)
    elif name == "far_lone":
        # a lone start 700 m from its 8 nearest: marches of more than LOS_MAX_SAMPLES samples
        xs, ys = np.meshgrid(np.arange(3) * 0.25, np.arange(3) * 0.25, indexing="ij")
        ground = np.concatenate([np.stack([xs.ravel(), ys.ravel(), np.zeros(9)], axis=1) + np.array([0.01, 0.0, 0.0]) * np.arange(9)[:, None],
                                 [[700.0, 0.3, 0.0]]]).astype(F)
        lethal = np.zeros((0, 3), F)
    else:
        raise KeyError(name)
    n = len(ground)
    return dict(name=name, ground=ground, map=_map(shift), cfg=Sr.config(), lethal=np.asarray(lethal, F), dgraph=_dgraph(ground, lethal),
                intensity=rng.uniform(0.0, 0.3, n).astype(F), node_weights=rng.uniform(0.0, 0.2, n).astype(F), plan_cfg=plan_cfg, shift=shift)


N_FLOOR = N_SIDE * N_SIDE
ISLAND, LONE = N_FLOOR, N_FLOOR + 3


@functools.lru_cache(maxsize=None)
def queries() -> tuple:
    """(label, case, start, goal, turning_weight, weighted, with_lethal)"""
    q = []
    for fl, pre in (("floor", ""), ("floor_shifted", "shifted_")):
        q.append((pre + "across_the_wall", fl, node(4, 4), node(20, 4), 0.1, False, True))
        q.append((pre + "across_weighted", fl, node(4, 4), node(20, 4), 0.1, True, True))
        if pre:
            continue
        q.append(("across_no_lethal", fl, node(4, 4), node(20, 4), 0.1, False, False))
        q.append(("past_the_isolated_node", fl, node(2, 21), node(9, 19), 0.0, False, True))
        q.append(("past_the_double_node", fl, node(15, 4), node(21, 6), 0.1, False, True))
        q.append(("same", fl, node(7, 7), node(7, 7), 0.1, False, True))
        q.append(("goal_on_the_island", fl, node(20, 8), ISLAND + 1, 0.1, False, True))
        q.append(("start_on_the_island", fl, ISLAND + 2, node(20, 8), 0.1, False, True))
        q.append(("start_lone", fl, LONE, node(3, 12), 0.1, True, True))
    la = "lattice"
    q.append(("lattice_diagonal", la, node(2, 2), node(20, 20), 0.1, False, True))
    q.append(("lattice_past_the_pair", la, node(8, 10), node(13, 10), 0.0, False, True))
    q.append(("lattice_weighted", la, node(20, 3), node(3, 18), 0.1, True, True))
    return tuple(q)


CAP_QUERIES = (("row_full", "cluster", 0, 1105, 0.1, False, False), ("sample_cap", "far_lone", 9, 4, 0.1, False, False))


def plan_cfg(q, **kw) -> dict:
    return R.config(turning_weight=q[4], **{**case(q[1])["plan_cfg"], **kw})


def run(q, stats=None, lethal=None, dgraph=None, **kw) -> dict:
    c = case(q[1])
    if lethal is None:
        lethal = c["lethal"] if q[6] else None
    return R.plan(c["ground"], c["dgraph"] if dgraph is None else dgraph, lethal, c["intensity"] if q[5] else None, c["node_weights"] if q[5] else None,
                  plan_cfg(q, **kw), q[2], q[3], stats=stats)


@functools.lru_cache(maxsize=None)
def reference(label: str) -> dict:
    """the restatement of a query, computed once and shared (callers must not write into it)"""
    q = {x[0]: x for x in queries() + CAP_QUERIES}[label]
    st = {}
    out = run(q, stats=st)
    out["stats"] = st
    return out


def check_cases() -> dict:
    """what the cases must hold (else the GPU tests prove less than they claim) -> the counts found"""
    found = dict(marched=0, blocked=0, single_point_samples=0, blocked_by_one_node_twice=0, fallbacks=0, fallback_reach_over_1m=0, march_over_16=0,
                 threshold_equal_clear=0, threshold_equal_blocked=0, found=0, no_path=0, lethal_skipped=0, updates=0)
    for q in queries():
        r = reference(q[0])
        assert r["n_los_capped"] == 0 and r["max_successors"] <= R.MAX_SUCCESSORS, q[0]
        found["marched"] += r["n_los_tested"]
        found["blocked"] += r["n_los_blocked"]
        found["fallbacks"] += r["n_knn_fallbacks"]
        found["lethal_skipped"] += r["n_lethal_skipped"]
        found["march_over_16"] += r["stats"]["longest_march"] > 16
        for k in ("single_point_samples", "blocked_by_one_node_twice", "fallback_reach_over_1m", "threshold_equal_clear", "threshold_equal_blocked", "updates"):
            found[k] += r["stats"][k]
        found["found"] += r["status"] == R.FOUND
        found["no_path"] += r["status"] == R.NO_PATH
    for k, v in found.items():
        assert v > 0, (k, found)
    a, b = reference("across_the_wall"), reference("across_no_lethal")
    assert a["status"] == b["status"] == R.FOUND and a["path"].tolist() != b["path"].tolist(), "the lethal cloud changes the path"
    found["path_with_lethal"], found["path_without"] = len(a["path"]), len(b["path"])
    s = reference("shifted_across_the_wall")
    assert s["path"].tolist() == a["path"].tolist(), "the far-away floor plans the same path"
    assert reference("goal_on_the_island")["status"] == R.NO_PATH and reference("start_on_the_island")["status"] == R.FOUND
    assert reference("start_lone")["status"] == R.FOUND
    r = reference("row_full")
    assert r["status"] == R.ROW_FULL and r["max_successors"] >= 1100
    r = reference("sample_cap")
    assert r["n_los_capped"] > 0 and r["n_los_blocked"] == r["n_los_capped"] and r["status"] == R.NO_PATH
    return found
