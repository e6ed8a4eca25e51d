"""The cases of the global planner's tests (tests/test_global_plan_cpu.py, tests/test_global_plan_gpu.py), from fixed
seeds, on the static layer's cases (static_layer_cases).  A case is a dict: ground, map, cfg (the static layer's), dgraph
(what get_min_dGraphValue serves: the static dGraph under a lethal disc, capped by the stack's start value), disc (the
layer a host slot of the stack is given), weights (random node weights) and plan_cfg overrides.  A query is (case, start,
goal, turning_weight, weighted).  check_cases() states what the cases have to contain for the GPU tests to prove what they
claim; the CPU tests run it."""
from __future__ import annotations

import functools

import numpy as np

import global_plan_ref as G
import static_layer_cases as Cs
import static_layer_ref as R

F = np.float32
D = np.float64
STACK_START = 99999.9            # get_min_dGraphValue's start value (stacked_perception.cpp:116)


def _lattice_clouds(n=40):
    """an exact 0.25 m lattice, z = 0: many equal f, and edges of exactly 0.5 m"""
    xs, ys = np.meshgrid(np.arange(n) * 0.25, np.arange(n) * 0.25, indexing="ij")
    g = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1).astype(F)
    rng = np.random.default_rng(21)
    m = np.stack([rng.uniform(0, 10, 200), rng.uniform(0, 10, 200), rng.uniform(2.0, 3.0, 200)], axis=1).astype(F)   # above head height
    return g, m


RING = ((9.0, 3.0), 0.8)         # the floor's ring of obstacle: centre and radius


def _disc(ground, centre, radius, ring=None):
    """a stack-style layer: the distance to a disc of obstacle, 0 inside it (node n keeps the start value).  ring: also a
    thin circle of obstacle; what lies within 0.5 m of it is lethal, so the few nodes around its centre are a component of
    their own (the pocket)"""
    g = np.asarray(ground, D)
    d = np.maximum(np.hypot(g[:, 0] - centre[0], g[:, 1] - centre[1]) - radius, 0.0)
    if ring is not None:
        d = np.minimum(d, np.abs(np.hypot(g[:, 0] - ring[0][0], g[:, 1] - ring[0][1]) - ring[1]))
    return np.concatenate([d, [STACK_START]])


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    if name == "lattice":
        g, m = _lattice_clouds()
        base = dict(ground=g, map=m, cfg=R.config())
        centre, shift = (5.0, 5.0), np.zeros(3)
    else:
        base = dict(Cs.all_cases()[name])
        shift = np.array(Cs.SHIFT) if name == "floor_shifted" else np.zeros(3)
        centre = (6.0, 9.0) if name.startswith("floor") else (1.5, 4.5)
    c = dict(base)
    c["name"] = name
    c["shift"] = shift
    ref = static_ref(name)
    c["disc"] = _disc(c["ground"].astype(D) - shift, centre, 0.6, RING if name.startswith("floor") else None)
    # (long_row's random map leaves hardly a node clear of obstacles: there the disc is the only layer)
    c["dgraph"] = np.minimum(np.minimum(ref["dgraph"], c["disc"]), STACK_START) if name != "long_row" else np.minimum(c["disc"], STACK_START)
    c["weights"] = np.random.default_rng(9).uniform(0.0, 0.3, len(c["ground"])).astype(F)
    c["plan_cfg"] = dict(a_star_expanding_radius=1.0) if name == "long_row" else {}
    return c


@functools.lru_cache(maxsize=None)
def static_ref(name: str):
    if name == "lattice":
        g, m = _lattice_clouds()
        return R.build(g, m, R.config())
    return Cs.reference(name)


def node_at(name: str, x, y, free=True) -> int:
    """the node nearest to (x, y) in the case's unshifted frame; free: among those the planner may enter"""
    c = case(name)
    g = c["ground"].astype(D) - c["shift"]
    d = np.hypot(g[:, 0] - x, g[:, 1] - y)
    if free:
        d = np.where(c["dgraph"][:-1] < 0.5, np.inf, d)
    return int(np.argmin(d))


@functools.lru_cache(maxsize=None)
def queries() -> tuple:
    """(label, case, start, goal, turning_weight, weighted)"""
    q = []
    fl = "floor"
    lone = int(np.flatnonzero(np.all(case(fl)["ground"] == F([-40.0, 0.0, 0.0]), axis=1))[0])
    corner = (node_at(fl, 1.0, 1.0), node_at(fl, 11.0, 13.0))
    hole = (node_at(fl, 2.6, 9.25), node_at(fl, 5.4, 9.6))
    ramp = (node_at(fl, 6.0, 12.0), node_at(fl, 11.3, 7.0))
    same = node_at(fl, 2.0, 2.0)
    in_disc = node_at(fl, 6.0, 9.0, free=False)
    # a start the disc makes lethal, at its rim, so that it has neighbours that are not (the reference does not test the start)
    rim = case(fl)["disc"][:-1]
    at_rim = int(np.argmax(np.where(rim < 0.5, rim, -1.0)))
    for tw in (0.1, 0.0):
        q.append((f"corner_tw{tw}", fl, *corner, tw, False))
    q.append(("corner_weighted", fl, *corner, 0.1, True))
    q.append(("hole", fl, *hole, 0.1, False))
    q.append(("hole_weighted_tw0", fl, *hole, 0.0, True))
    q.append(("ramp", fl, *ramp, 0.1, False))
    q.append(("same", fl, same, same, 0.1, False))
    q.append(("goal_lone", fl, corner[0], lone, 0.1, False))
    q.append(("goal_in_disc", fl, hole[0], in_disc, 0.1, False))
    q.append(("start_in_disc", fl, at_rim, corner[0], 0.1, True))
    q.append(("back_across", fl, corner[1], hole[0], 0.1, False))
    # no-path queries on which the reference is defined: its loop ends at :213 on a set that a pop of an open node left empty
    q.append(("start_lone", fl, lone, corner[0], 0.1, False))                  # one pop, no successor but the node itself
    q.append(("start_in_pocket", fl, node_at(fl, *RING[0]), corner[0], 0.1, False))  # the ring's inside, exhausted without an update
    sh = "floor_shifted"
    q.append(("shifted_corner", sh, node_at(sh, 1.0, 1.0), node_at(sh, 11.0, 13.0), 0.1, False))
    q.append(("shifted_hole", sh, node_at(sh, 2.6, 9.25), node_at(sh, 5.4, 9.6), 0.1, True))
    lr = "long_row"
    q.append(("long_row_through", lr, node_at(lr, 0.5, 0.5), node_at(lr, 5.0, 5.0), 0.1, False))
    q.append(("long_row_into", lr, node_at(lr, 5.5, 0.5), node_at(lr, 3.0, 3.05), 0.0, True))
    la = "lattice"
    q.append(("lattice_diagonal", la, node_at(la, 0.75, 0.75), node_at(la, 9.0, 9.0), 0.1, False))
    q.append(("lattice_row_tw0", la, node_at(la, 0.75, 5.0), node_at(la, 9.25, 5.0), 0.0, False))
    q.append(("lattice_weighted", la, node_at(la, 9.0, 0.75), node_at(la, 1.0, 8.0), 0.1, True))
    return tuple(q)


def plan_cfg(q, **kw) -> dict:
    return G.config(turning_weight=q[4], **{**case(q[1])["plan_cfg"], **kw})


def run(q, dgraph=None, stats=None, **kw) -> dict:
    c = case(q[1])
    return G.plan(static_ref(q[1]), c["ground"], c["dgraph"] if dgraph is None else dgraph, c["weights"] if q[5] else None, plan_cfg(q), q[2], q[3],
                  stats=stats, **kw)


@functools.lru_cache(maxsize=None)
def reference(label: str) -> dict:
    """the restatement of a query, computed once and shared (callers must not write into it)"""
    q = {x[0]: x for x in queries()}[label]
    st = {}
    out = run(q, stats=st)
    out["stats"] = st
    return out


def check_cases() -> dict:
    """what the cases must hold (else the GPU tests prove less than they claim) -> the counts found"""
    found = dict(tie_pops=0, updates=0, discarded=0, radius_skipped=0, radius_equal_kept=0, theta_above_cap=0, theta_below_cap=0, rows_over_256=0,
                 found=0, no_path=0, no_path_defined=0, no_path_on_emptied_set=0)
    for q in queries():
        r = reference(q[0])
        for k in ("tie_pops", "updates", "radius_skipped", "radius_equal_kept", "theta_above_cap", "theta_below_cap", "rows_over_256"):
            found[k] += r["stats"][k]
        found["discarded"] += r["n_discarded_closed"]
        found["found"] += r["status"] == G.FOUND
        found["no_path"] += r["status"] == G.NO_PATH
        found["no_path_defined"] += r["status"] == G.NO_PATH and not r["ended_on_emptied_set"]
        found["no_path_on_emptied_set"] += r["status"] == G.NO_PATH and r["ended_on_emptied_set"]
    for k, v in found.items():
        assert v > 0, (k, found)
    return found
