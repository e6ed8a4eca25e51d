"""GPU tests of the pre-graph global planner on the device graph (dddmr_rollout_global_plan_*): status, path, counters and
the goal's g bit for bit against tests/helpers/global_plan_ref.py (pinned to the reference's own compiled planner by
tests/test_global_plan_pin_cpu.py; tests/test_global_plan_pin_gpu.py holds the device to its answers), the nearest-node search and the
goal probe against brute force in NumPy float32, batches, limits and refusals.  tests/test_global_plan_cpu.py holds the
conditions on the cases that these tests rely on."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, global_plan, scenes, stack, static_layer
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import global_plan_ref as G  # noqa: E402
import global_plan_cases as Cs  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MAX_NODES = 4096


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


def layer(lp, name):
    """the static layer built on a case, and a stack whose one host slot holds the case's dGraph"""
    c = Cs.case(name)
    sl = static_layer.StaticLayer(lp, static_layer.shipped_config(max_ground_points=MAX_NODES, max_map_points=8192, max_edges=400_000, **c["cfg"]))
    sl.build(c["ground"], c["map"])
    st = stack.PerceptionStack(lp, host_layers=(c["dgraph"],), n_ground=len(c["ground"]), max_changes=len(c["ground"]) + 1)
    st.update()
    return sl, st


def planner(lp, q=None, **kw):
    d = dict(max_open_entries=1 << 16, max_expansions=MAX_NODES)
    if q is not None:
        d.update(turning_weight=q[4], **Cs.case(q[1])["plan_cfg"])
    d.update(kw)
    return global_plan.GlobalPlan(lp, global_plan.shipped_config(**d), MAX_NODES)


def same(got, ref, name=""):
    print(f"{name}: status {got.status}, {len(got.path)} nodes, expanded {got.n_expanded}, pushed {got.n_pushed}, discarded {got.n_discarded_closed}, "
          f"g {got.g_goal!r} | restatement {ref['status']}, {len(ref['path'])}, {ref['n_expanded']}, {ref['n_pushed']}, {ref['n_discarded_closed']}, {ref['g_goal']!r}")
    assert got.status == ref["status"], name
    assert got.path.tolist() == ref["path"].tolist(), name
    assert (got.n_expanded, got.n_pushed, got.n_discarded_closed) == (ref["n_expanded"], ref["n_pushed"], ref["n_discarded_closed"]), name
    assert F(got.g_goal).view(np.uint32) == F(ref["g_goal"]).view(np.uint32), name


@pytest.mark.parametrize("name", ("floor", "floor_shifted", "long_row", "lattice"))
def test_every_query_matches_the_restatement(lp, name):
    """dgraph_source 0 through a host-only stack slot: every query of the case, one plan each; then again in the same state
    (the stamps: no record of the first plan shows in the second)"""
    layer(lp, name)
    c = Cs.case(name)
    for q in Cs.queries():
        if q[1] != name:
            continue
        gp = planner(lp, q)
        gp.set_node_weights(c["weights"] if q[5] else None)
        ref = Cs.reference(q[0])
        first = gp.plan(q[2], q[3])
        same(first, ref, q[0])
        assert first.host_waits == 1
        same(gp.plan(q[2], q[3]), ref, q[0] + " again")
        if q[5]:
            gp.set_node_weights(None)                                          # back to all zero: another answer
            assert gp.plan(q[2], q[3]).g_goal != first.g_goal


def test_bound_static_dgraph_and_the_static_layers_own(lp):
    """the floor's dGraph bound device to device into slot 0 and the disc in slot 1: the stack's minimum is the case's
    dGraph; then dgraph_source 1, the static layer's own dGraph without the disc"""
    c = Cs.case("floor")
    n = len(c["ground"])
    sl = static_layer.StaticLayer(lp, static_layer.shipped_config(max_ground_points=MAX_NODES, max_map_points=8192, max_edges=400_000, **c["cfg"]))
    sl.build(c["ground"], c["map"])
    st = stack.PerceptionStack(lp, host_layers=(None, c["disc"]), n_ground=n, max_changes=n + 1)
    sl.bind(0, 0)
    st.update()
    assert st.min_dgraph().tobytes() == c["dgraph"].tobytes()
    qs = {x[0]: x for x in Cs.queries()}
    for lab in ("corner_tw0.1", "hole", "goal_in_disc"):
        same(planner(lp, qs[lab]).plan(qs[lab][2], qs[lab][3]), Cs.reference(lab), lab)
    own = sl.dgraph()
    assert own.tobytes() == Cs.static_ref("floor")["dgraph"].tobytes()
    for lab in ("corner_tw0.1", "goal_in_disc"):
        ref = Cs.run(qs[lab], dgraph=own)
        got = planner(lp, qs[lab], dgraph_source=1).plan(qs[lab][2], qs[lab][3])
        same(got, ref, lab + " (static)")
        assert got.status == K.GLOBAL_PLAN_FOUND                               # (no disc: its inside can be entered)


def test_a_batch_equals_its_single_plans(lp):
    layer(lp, "floor")
    qs = [q for q in Cs.queries() if q[1] == "floor" and q[4] == 0.1 and not q[5]]
    assert len(qs) >= 7
    qs = (qs + qs[:2])[:8]
    qs[7] = qs[0]                                                              # the same query twice in one batch
    gp = planner(lp, qs[0])
    singles = [gp.plan(q[2], q[3]) for q in qs]
    batch = gp.plan_many([q[2] for q in qs], [q[3] for q in qs])
    at = 0
    for q, one, got, raw in zip(qs, singles, batch, gp.last_results):
        same(got, Cs.reference(q[0]), q[0])
        assert got.path.tolist() == one.path.tolist() and got.n_pushed == one.n_pushed
        assert got.host_waits == 1 and raw.path_offset == at                  # one wait whatever q; the paths follow one another
        at += raw.path_len
    assert batch[7].path.tolist() == batch[0].path.tolist() and len(batch[0].path) > 1
    for n_q in (4, 16):
        many = gp.plan_many([qs[i % 8][2] for i in range(n_q)], [qs[i % 8][3] for i in range(n_q)])
        assert all(m.host_waits == 1 for m in many)
        assert [m.path.tolist() for m in many] == [singles[i % 8].path.tolist() for i in range(n_q)]
    # paths beyond path_capacity: refused, the results filled
    refused(K.ERR_CAPACITY, gp.plan_many, [qs[0][2]], [qs[0][3]], 3)
    assert gp.last_results[0].status == K.GLOBAL_PLAN_FOUND and gp.last_results[0].path_len == len(singles[0].path)
    refused(K.ERR_CAPACITY, planner(lp, qs[0], max_queries=4).plan_many, [qs[0][2]] * 5, [qs[0][3]] * 5)


def test_a_plan_after_another_build(lp):
    """floor, then the lattice in the same static layer: the second plan is the lattice's, and the floor's node weights are gone"""
    qs = {x[0]: x for x in Cs.queries()}
    sl, _ = layer(lp, "floor")
    gp = planner(lp, qs["corner_weighted"])
    gp.set_node_weights(Cs.case("floor")["weights"])
    same(gp.plan(*qs["corner_weighted"][2:4]), Cs.reference("corner_weighted"), "corner_weighted")
    c = Cs.case("lattice")
    sl.build(c["ground"], c["map"])
    refused(K.ERR_BAD_ARG, gp.plan, *qs["lattice_diagonal"][2:4])              # the stack still has the floor's n_ground
    st = stack.PerceptionStack(lp, host_layers=(c["dgraph"],), n_ground=len(c["ground"]), max_changes=len(c["ground"]) + 1)
    st.update()
    same(gp.plan(*qs["lattice_diagonal"][2:4]), Cs.reference("lattice_diagonal"), "lattice_diagonal")
    refused(K.ERR_BAD_ARG, gp.set_node_weights, Cs.case("floor")["weights"])   # as many weights as the floor has nodes


def test_nearest_and_probe_against_brute_force(lp):
    rng = np.random.default_rng(17)
    for name in ("lattice", "floor", "floor_shifted"):
        layer(lp, name)
        c = Cs.case(name)
        g = c["ground"]
        gp = planner(lp)
        pts = [g[rng.integers(0, len(g), 300)] + rng.uniform(-0.6, 0.6, (300, 3)).astype(F) * F([1, 1, 0.3])]
        pts.append(g[rng.integers(0, len(g), 40)])                            # on a node
        if name == "lattice":
            edge = g[np.argmax(g[:, 0])]
            pts.append(np.array([edge + F([0.5, 0, 0]), edge + F([0.25, 0, 0]),                     # exactly 0.5 m: outside; 0.25 m: inside 0.5, outside 0.25
                                 g[0] + F([0.125, 0, 0]), g[41] + F([0.125, 0.125, 0])], F))       # two and four equidistant nodes
        else:
            pts.append(g[[100, len(g) - 7]])                                   # the coincident pair: the lower index
            pts.append(g[:3] + F([30.0, 30.0, 9.0]))                           # far from every node
        pts = np.concatenate(pts).astype(F)
        ids = gp.nearest(pts)
        want = G.nearest(g, pts)
        np.testing.assert_array_equal(ids, want, err_msg=name)
        cnt, blocked = gp.probe(pts)
        wc, wb = G.probe(g, c["dgraph"], pts, 0.5)
        np.testing.assert_array_equal(cnt, wc, err_msg=name)
        np.testing.assert_array_equal(blocked, wb, err_msg=name)
        print(f"{name}: {len(pts)} points, {int((ids == K.GLOBAL_PLAN_NONE).sum())} without a node, {int((cnt == 0).sum())} empty probes, {int(blocked.sum())} blocked")
        assert (ids == K.GLOBAL_PLAN_NONE).any() and (ids != K.GLOBAL_PLAN_NONE).any() and blocked.any() and (~blocked & (cnt > 0)).any()
        if name == "lattice":
            assert ids[-4] == K.GLOBAL_PLAN_NONE and ids[-3] != K.GLOBAL_PLAN_NONE and cnt[-3] == 0 and ids[-2] == 0 and ids[-1] == 41
        else:
            assert ids[340] == ids[341] == 100
        assert gp.nearest(np.zeros((0, 3), F)).size == 0
        bad = pts[:4].copy()
        bad[2, 1] = np.inf
        refused(K.ERR_BAD_ARG, gp.nearest, bad)
        refused(K.ERR_BAD_ARG, gp.probe, bad)


def test_limits(lp):
    layer(lp, "floor")
    q = {x[0]: x for x in Cs.queries()}["corner_tw0.1"]
    c = Cs.case("floor")
    ref = G.plan(Cs.static_ref("floor"), c["ground"], c["dgraph"], None, Cs.plan_cfg(q, max_expansions=10), q[2], q[3])
    got = planner(lp, q, max_expansions=10).plan(q[2], q[3])
    same(got, ref, "budget")
    assert got.status == K.GLOBAL_PLAN_BUDGET and got.n_expanded == 10 and len(got.path) == 0
    ref = G.plan(Cs.static_ref("floor"), c["ground"], c["dgraph"], None, Cs.plan_cfg(q, max_open_entries=16), q[2], q[3])
    gp = planner(lp, q, max_open_entries=16)
    refused(K.ERR_CAPACITY, gp.plan, q[2], q[3])
    r = gp.last_results[0]
    assert r.status == K.GLOBAL_PLAN_OPEN_FULL == ref["status"] and r.path_len == 0
    assert (r.n_expanded, r.n_pushed, r.n_discarded_closed) == (ref["n_expanded"], ref["n_pushed"], ref["n_discarded_closed"])
    # a second query of the same batch is answered although the first one overflowed
    gp = planner(lp, q, max_open_entries=16)
    s = {x[0]: x for x in Cs.queries()}["same"]
    refused(K.ERR_CAPACITY, gp.plan_many, [q[2], s[2]], [q[3], s[3]])
    assert [r.status for r in gp.last_results] == [K.GLOBAL_PLAN_OPEN_FULL, K.GLOBAL_PLAN_FOUND]


def test_refusals(lp, lp2):
    c = Cs.case("floor")
    n = len(c["ground"])
    q = {x[0]: x for x in Cs.queries()}["hole"]
    cfg = global_plan.shipped_config(max_open_entries=1 << 16, max_expansions=MAX_NODES)
    refused(K.ERR_STATE, global_plan.GlobalPlan, lp2, cfg, MAX_NODES)          # no static_layer_create
    sl = static_layer.StaticLayer(lp2, static_layer.shipped_config(max_ground_points=MAX_NODES, max_map_points=8192, max_edges=400_000, **c["cfg"]))
    for bad in (dict(max_queries=0), dict(max_queries=17), dict(dgraph_source=2), dict(max_open_entries=0), dict(max_expansions=0), dict(turning_weight=float("nan"))):
        refused(K.ERR_BAD_ARG, lambda: planner(lp2, None, **bad))
    gp = planner(lp2, q)
    refused(K.ERR_STATE, gp.plan, q[2], q[3])                                  # no build
    refused(K.ERR_STATE, gp.nearest, c["ground"][:2])
    sl.build(c["ground"], c["map"])
    refused(K.ERR_STATE, gp.plan, q[2], q[3])                                  # dgraph_source 0 without a stack
    refused(K.ERR_STATE, gp.probe, c["ground"][:2])
    assert gp.nearest(c["ground"][5:6]).tolist() == [5]                        # (needs no dGraph)
    own = planner(lp2, q, dgraph_source=1)
    assert own.plan(q[2], q[3]).status == K.GLOBAL_PLAN_FOUND
    refused(K.ERR_BAD_ARG, own.plan, n, q[3])                                  # an id >= n_ground
    refused(K.ERR_BAD_ARG, own.plan, q[2], K.GLOBAL_PLAN_NONE)
    w = np.zeros(n, F)
    w[7] = -0.01
    refused(K.ERR_BAD_ARG, own.set_node_weights, w)                            # a negative weight
    w[7] = np.nan
    refused(K.ERR_BAD_ARG, own.set_node_weights, w)
    refused(K.ERR_BAD_ARG, own.set_node_weights, np.zeros(n - 1, F))
    stack.PerceptionStack(lp2, host_layers=(np.full(n + 3, 7.0),), n_ground=n + 2, max_changes=8).update()
    gp = planner(lp2, q)                                                       # (a context has one planner, the last one created: dgraph_source 0 again)
    refused(K.ERR_BAD_ARG, gp.plan, q[2], q[3])                                # a stack of another n_ground
    refused(K.ERR_BAD_ARG, gp.probe, c["ground"][:2])
    own = planner(lp2, q, dgraph_source=1)
    # a build without generate_static_graph: no rows to walk
    sl2 = static_layer.StaticLayer(lp2, static_layer.shipped_config(max_ground_points=MAX_NODES, max_map_points=8192, max_edges=400_000,
                                                                    **{**c["cfg"], "generate_static_graph": 0}))
    sl2.build(c["ground"], c["map"])
    refused(K.ERR_STATE, own.plan, q[2], q[3])
    # a static layer created again with more ground points than the planner was sized for
    static_layer.StaticLayer(lp2, static_layer.shipped_config(max_ground_points=2 * MAX_NODES, max_map_points=8192, max_edges=400_000, **c["cfg"]))
    refused(K.ERR_STATE, own.plan, q[2], q[3])


def test_every_entry_is_refused_beside_a_pending_tick(lp):
    layer(lp, "floor")
    q = {x[0]: x for x in Cs.queries()}["hole"]
    c = Cs.case("floor")
    gp = planner(lp, q)
    before_plan = gp.plan(q[2], q[3])
    sc = scenes.bench_scene("C2")
    lp.set_cloud(sc.cloud)
    lp.setPlan(sc.plan)
    name = sc.theory.name.decode()
    before = lp.tick(name, sc.tick)
    lp.tick_begin(name, sc.tick)
    try:
        for call in (lambda: gp.plan(q[2], q[3]), lambda: gp.nearest(c["ground"][:3]), lambda: gp.probe(c["ground"][:3]),
                     lambda: gp.set_node_weights(c["weights"]), lambda: planner(lp, q)):
            refused(K.ERR_STATE, call)
    finally:
        lp.tick_end()
    same(gp.plan(q[2], q[3]), Cs.reference("hole"), "hole after the tick")
    assert gp.plan(q[2], q[3]).path.tolist() == before_plan.path.tolist()
    after = lp.tick(name, sc.tick)
    upto = K.RolloutResult.device_ms.offset                                    # everything but the two timings
    assert bytes(after)[:upto] == bytes(before)[:upto]
