"""GPU tests of the global planner's default A* on the device (dddmr_rollout_global_plan_plan_on_cloud, _set_lethal_points,
_set_graph_node_weights): status, path, every counter and the goal's g bit for bit against
tests/helpers/global_plan_cloud_ref.py, which is NOT pinned to compiled reference code yet.
tests/test_global_plan_cloud_cpu.py holds the conditions on the cases that these tests rely on."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, global_plan, scenes, stack, static_layer
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import global_plan_cloud_ref as R  # noqa: E402
import global_plan_cloud_cases as Cs  # noqa: E402
import global_plan_cases as Pc  # noqa: E402  (the pre-graph planner's cases, for the interleaved calls)

pytestmark = pytest.mark.gpu
F = np.float32
MAX_NODES = 4096
QS = {x[0]: x for x in Cs.queries() + Cs.CAP_QUERIES}


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:      # (the C2 scene's cloud, for the pending tick)
        yield p


@pytest.fixture(scope="module")
def lp2():
    with LocalPlanner([configs.bench_theory("C2")], max_points=1000) as p:
        yield p


def refused(code, fn, *a):
    with pytest.raises(RolloutError) as e:
        fn(*a)
    assert e.value.code == code, (e.value.code, str(e.value))


def layer(lp, name, dgraph=None, **cfg):
    """the static layer built on a case, and a stack whose one host slot holds the case's dGraph"""
    c = Cs.case(name)
    sl = static_layer.StaticLayer(lp, static_layer.shipped_config(max_ground_points=MAX_NODES, max_map_points=8192, max_edges=400_000, **{**c["cfg"], **cfg}))
    sl.build(c["ground"], c["map"])
    st = stack.PerceptionStack(lp, host_layers=(c["dgraph"] if dgraph is None else dgraph,), n_ground=len(c["ground"]), max_changes=len(c["ground"]) + 1)
    st.update()
    return sl, st


def planner(lp, q=None, **kw):
    d = dict(max_open_entries=1 << 16, max_expansions=MAX_NODES, inscribed_radius=R.CFG["inscribed_radius"])
    if q is not None:
        d.update(turning_weight=q[4], **Cs.case(q[1])["plan_cfg"])
    d.update(kw)
    return global_plan.GlobalPlan(lp, global_plan.shipped_config(**d), MAX_NODES)


def arm(gp, q):
    """the planner's three arrays as the query wants them"""
    c = Cs.case(q[1])
    gp.set_node_weights(c["intensity"] if q[5] else None)
    gp.set_graph_node_weights(c["node_weights"] if q[5] else None)
    gp.set_lethal_points(c["lethal"] if q[6] else None)


def same(got, ref, name=""):
    print(f"{name}: status {got.status}, {len(got.path)} nodes, expanded {got.n_expanded}, pushed {got.n_pushed}, discarded {got.n_discarded_closed}, "
          f"g {got.g_goal!r}, " + ", ".join(f"{k} {getattr(got, k)}" for k in R.COUNTERS)
          + f" | restatement {ref['status']}, {len(ref['path'])}, {ref['n_expanded']}, {ref['n_pushed']}, {ref['n_discarded_closed']}, {ref['g_goal']!r}, "
          + ", ".join(f"{ref[k]}" for k in R.COUNTERS))
    assert got.status == ref["status"], name
    assert got.path.tolist() == ref["path"].tolist(), name
    assert (got.n_expanded, got.n_pushed, got.n_discarded_closed) == (ref["n_expanded"], ref["n_pushed"], ref["n_discarded_closed"]), name
    assert {k: getattr(got, k) for k in R.COUNTERS} == {k: int(ref[k]) for k in R.COUNTERS}, name
    assert F(got.g_goal).view(np.uint32) == F(ref["g_goal"]).view(np.uint32), name


@pytest.mark.parametrize("name", ("floor", "floor_shifted", "lattice"))
def test_every_query_matches_the_restatement(lp, name):
    """the lethal cloud through set_lethal_points, the dGraph through a host-only stack slot (no device layer: no mask bit):
    every query of the case, one plan each; then again in the same state (the stamps)"""
    layer(lp, name)
    for q in Cs.queries():
        if q[1] != name:
            continue
        gp = planner(lp, q)
        arm(gp, q)
        ref = Cs.reference(q[0])
        first = gp.plan_on_cloud(q[2], q[3])
        same(first, ref, q[0])
        assert first.host_waits == 1
        same(gp.plan_on_cloud(q[2], q[3]), ref, q[0] + " again")
    if name == "floor_shifted":                                                # bit-equal to the unshifted restatement's path
        q = QS["shifted_across_the_wall"]
        gp = planner(lp, q)
        arm(gp, q)
        assert gp.plan_on_cloud(q[2], q[3]).path.tolist() == Cs.reference("across_the_wall")["path"].tolist()


def test_the_device_layers_lethal_nodes():
    """a lidar marking layer, a depth layer and a stack on one ground: the lethal cloud is ground[stack.lethal_nodes()], a
    node that both layers hold lethal twice; the same points added again through set_lethal_points count again"""
    import test_stack_gpu as TS
    import depth_mark_cases as mc
    with TS.T.planner() as lp3:
        rig = TS.Rig(lp3, max_changes=8192)
        u = rig.ups[0]
        rig.feed(u)
        rig.stack.set_host_layer(0, np.where(np.isfinite(rig.static), rig.static, 9999.0))   # (stack_cases plants a NaN and an inf)
        rig.stack.update(mc.TBS_LIDAR, u["t_gb"])
        ground = rig.ground
        n = len(ground)
        ids = rig.stack.lethal_nodes()
        mask = rig.stack.lethal_mask()[:n]
        twice = int((np.bincount(ids, minlength=n) > 1).sum())
        print(f"{n} nodes, {len(ids)} lethal points, {twice} nodes in two layers")
        assert len(ids) > 0 and len(ids) == int(sum(bin(int(m)).count('1') for m in mask))
        sl = static_layer.StaticLayer(lp3, static_layer.shipped_config(max_ground_points=8192, max_map_points=1024, max_edges=16, generate_static_graph=0))
        sl.build(ground, np.zeros((0, 3), F))
        dgraph = rig.stack.min_dgraph()
        assert np.isfinite(dgraph).all()
        gp = global_plan.GlobalPlan(lp3, global_plan.shipped_config(max_open_entries=1 << 16, max_expansions=8192, inscribed_radius=0.15), 8192)
        lethal = ground[ids]
        first = lethal.astype(np.float64)[0]                                    # one obstacle: the lethal nodes around the first one
        centre = lethal.astype(np.float64)[np.hypot(lethal[:, 0] - first[0], lethal[:, 1] - first[1]) < 0.8].mean(axis=0)
        free = np.where(rig.stack.min_dgraph()[:n] >= 0.3, 0.0, np.inf)

        def near(dx, dy):
            return int(np.argmin(np.hypot(ground[:, 0] - (centre[0] + dx), ground[:, 1] - (centre[1] + dy)) + free))
        blocked = 0
        for s, g in ((near(-0.9, 0.05), near(0.9, -0.05)), (near(0.05, -0.9), near(-0.05, 0.9))):
            ref = R.plan(ground, dgraph, lethal, None, None, R.config(), s, g)
            same(gp.plan_on_cloud(s, g), ref, f"device layers {s} -> {g}")
            blocked += ref["n_los_blocked"]
            gp.set_lethal_points(lethal)
            ref2 = R.plan(ground, dgraph, np.concatenate([lethal, lethal]), None, None, R.config(), s, g)
            same(gp.plan_on_cloud(s, g), ref2, f"device layers and the same points again {s} -> {g}")
            assert ref2["n_los_blocked"] >= ref["n_los_blocked"]
            gp.set_lethal_points(None)
        assert blocked > 0


def test_the_static_layers_own_dgraph_has_no_lethal_point(lp):
    """dgraph_source 1: no stack, no device lethal point; every edge is clear"""
    sl, _ = layer(lp, "floor")
    own = sl.dgraph()
    q = QS["across_the_wall"]
    gp = planner(lp, q, dgraph_source=1)
    gp.set_lethal_points(None)
    ref = Cs.run(q, lethal=np.zeros((0, 3), F), dgraph=own)
    got = gp.plan_on_cloud(q[2], q[3])
    same(got, ref, "static dGraph")
    assert got.n_los_blocked == 0 and got.n_los_tested > 0
    # ... and the host layers' points are then the whole cloud
    gp.set_lethal_points(Cs.case("floor")["lethal"])
    ref = Cs.run(q, dgraph=own)
    same(gp.plan_on_cloud(q[2], q[3]), ref, "static dGraph, lethal points")
    assert ref["n_los_blocked"] > 0
    gp.set_lethal_points(None)


def test_a_batch_equals_its_single_plans_and_the_other_search_does_not_show(lp):
    layer(lp, "floor")
    qs = [q for q in Cs.queries() if q[1] == "floor" and not q[5] and q[6]]
    assert len(qs) >= 6
    qs = [qs[i % len(qs)] for i in range(16)]
    gp = planner(lp, qs[0], turning_weight=0.1)
    arm(gp, qs[0])
    refs = [Cs.run(q[:4] + (0.1,) + q[5:]) for q in qs[:len(set(qs))]]
    refs = [refs[i % len(refs)] for i in range(16)]
    singles = [gp.plan_on_cloud(q[2], q[3]) for q in qs]
    batch = gp.plan_many_on_cloud([q[2] for q in qs], [q[3] for q in qs])
    at = 0
    for q, one, got, raw, ref in zip(qs, singles, batch, gp.last_results, refs):
        same(got, ref, q[0])
        same(one, ref, q[0] + " alone")
        assert got.host_waits == 1 and raw.plan.path_offset == at
        at += raw.plan.path_len
    # interleaved with the pre-graph search on the same records: each answers as it does alone
    pre = [gp.plan(q[2], q[3]) for q in qs[:4]]
    for q, one, p in zip(qs[:4], singles, pre):
        again = gp.plan_on_cloud(q[2], q[3])
        assert again.path.tolist() == one.path.tolist() and again.n_pushed == one.n_pushed
        p2 = gp.plan(q[2], q[3])
        assert p2.path.tolist() == p.path.tolist() and p2.n_pushed == p.n_pushed and p2.n_expanded == p.n_expanded
    many = gp.plan_many([q[2] for q in qs[:4]], [q[3] for q in qs[:4]])
    assert [m.path.tolist() for m in many] == [p.path.tolist() for p in pre]
    # paths beyond path_capacity: refused, the results filled; more queries than max_queries
    refused(K.ERR_CAPACITY, gp.plan_many_on_cloud, [qs[0][2]], [qs[0][3]], 3)
    assert gp.last_results[0].plan.status == K.GLOBAL_PLAN_FOUND and gp.last_results[0].plan.path_len == len(singles[0].path)
    small = planner(lp, qs[0], max_queries=4)
    refused(K.ERR_CAPACITY, small.plan_many_on_cloud, [qs[0][2]] * 5, [qs[0][3]] * 5)


def test_a_static_layer_without_a_graph_is_enough(lp):
    layer(lp, "floor", generate_static_graph=0)
    q = QS["across_the_wall"]
    gp = planner(lp, q)
    arm(gp, q)
    same(gp.plan_on_cloud(q[2], q[3]), Cs.reference(q[0]), q[0] + " without sGraph")
    refused(K.ERR_STATE, gp.plan, q[2], q[3])                                  # the pre-graph search has no rows to walk


@pytest.mark.parametrize("label", ("row_full", "sample_cap"))
def test_caps(lp, label):
    q = QS[label]
    layer(lp, q[1], generate_static_graph=0)                                   # (1100 nodes in one ball: more than a million edges)
    gp = planner(lp, q)
    arm(gp, q)
    ref = Cs.reference(label)
    if label == "row_full":
        refused(K.ERR_CAPACITY, gp.plan_on_cloud, q[2], q[3])
        r = gp.last_results[0]
        assert r.plan.status == K.GLOBAL_PLAN_ROW_FULL == ref["status"] and r.plan.path_len == 0
        assert r.max_successors == ref["max_successors"] == 1100 and r.plan.n_expanded == 0
    else:
        got = gp.plan_on_cloud(q[2], q[3])
        same(got, ref, label)
        assert got.n_los_capped > 0 and got.n_los_blocked == got.n_los_capped


def test_refusals(lp, lp2):
    c = Cs.case("floor")
    n = len(c["ground"])
    q = QS["across_the_wall"]
    cfg = dict(max_ground_points=MAX_NODES, max_map_points=8192, max_edges=400_000, **c["cfg"])
    sl = static_layer.StaticLayer(lp2, static_layer.shipped_config(**cfg))
    gp = planner(lp2, q, dgraph_source=1)
    refused(K.ERR_STATE, gp.plan_on_cloud, q[2], q[3])                         # no build
    refused(K.ERR_STATE, gp.set_lethal_points, c["lethal"])
    refused(K.ERR_STATE, gp.set_graph_node_weights, c["node_weights"])
    sl.build(c["ground"][:7], c["map"])
    refused(K.ERR_STATE, gp.plan_on_cloud, 0, 1)                               # fewer than 8 ground nodes
    sl.build(c["ground"], c["map"])
    assert gp.plan_on_cloud(q[2], q[3]).status == K.GLOBAL_PLAN_FOUND
    refused(K.ERR_STATE, planner(lp2, q).plan_on_cloud, q[2], q[3])            # dgraph_source 0 without a stack
    zero = planner(lp2, q, dgraph_source=1, inscribed_radius=0.0)              # global_plan_create keeps accepting it
    refused(K.ERR_BAD_ARG, zero.plan_on_cloud, q[2], q[3])
    gp = planner(lp2, q, dgraph_source=1)
    refused(K.ERR_BAD_ARG, gp.plan_on_cloud, n, q[3])                          # an id >= n_ground
    refused(K.ERR_BAD_ARG, gp.plan_on_cloud, q[2], K.GLOBAL_PLAN_NONE)
    w = np.zeros(n, F)
    w[7] = -0.01
    refused(K.ERR_BAD_ARG, gp.set_graph_node_weights, w)                       # a negative weight
    w[7] = np.nan
    refused(K.ERR_BAD_ARG, gp.set_graph_node_weights, w)
    refused(K.ERR_BAD_ARG, gp.set_graph_node_weights, np.zeros(n - 1, F))
    bad = c["lethal"].copy()
    bad[3, 1] = np.inf
    refused(K.ERR_BAD_ARG, gp.set_lethal_points, bad)
    bad[3, 1] = np.nan
    refused(K.ERR_BAD_ARG, gp.set_lethal_points, bad)
    refused(K.ERR_CAPACITY, gp.set_lethal_points, np.zeros((MAX_NODES + 1, 3), F))
    refused(K.ERR_CAPACITY, gp.plan_many_on_cloud, [q[2]] * 17, [q[3]] * 17)   # too many queries
    refused(K.ERR_CAPACITY, gp.plan_many_on_cloud, [q[2]], [q[3]], 2)          # a path capacity that is too small
    assert gp.plan_on_cloud(q[2], q[3]).status == K.GLOBAL_PLAN_FOUND          # (a refused set_lethal_points left no cloud behind)


def test_every_entry_is_refused_beside_a_pending_tick(lp):
    layer(lp, "floor")
    q = QS["across_the_wall"]
    c = Cs.case("floor")
    gp = planner(lp, q)
    arm(gp, q)
    before_plan = gp.plan_on_cloud(q[2], q[3])
    sc = scenes.bench_scene("C2")
    lp.set_cloud(sc.cloud)
    lp.setPlan(sc.plan)
    name = sc.theory.name.decode()
    before = lp.tick(name, sc.tick)
    lp.tick_begin(name, sc.tick)
    try:
        for call in (lambda: gp.plan_on_cloud(q[2], q[3]), lambda: gp.set_lethal_points(c["lethal"]), lambda: gp.set_graph_node_weights(c["node_weights"])):
            refused(K.ERR_STATE, call)
    finally:
        lp.tick_end()
    same(gp.plan_on_cloud(q[2], q[3]), Cs.reference(q[0]), "after the tick")
    assert gp.plan_on_cloud(q[2], q[3]).path.tolist() == before_plan.path.tolist()
    after = lp.tick(name, sc.tick)
    upto = K.RolloutResult.device_ms.offset                                    # everything but the two timings
    assert bytes(after)[:upto] == bytes(before)[:upto]
