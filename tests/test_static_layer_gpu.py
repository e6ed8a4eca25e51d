"""GPU tests of the static layer and the no-entry layer on the device (dddmr_rollout_static_layer_*): sGraph's CSR rows,
both dGraphs and the stack binding, bit for bit against tests/helpers/static_layer_ref.py (UNPINNED, see there), and
the refusals.  tests/test_static_layer_cpu.py holds the conditions on the cases that these tests rely on."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, scenes, stack, static_layer
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import static_layer_ref as R  # noqa: E402
import static_layer_cases as Cs  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:      # (the C2 scene's cloud, for the pending tick)
        yield p


@pytest.fixture(scope="module")
def lp2():
    with LocalPlanner([configs.bench_theory("C2")], max_points=1000) as p:
        yield p


def layer(lp, cfg, **kw):
    d = dict(max_ground_points=4096, max_map_points=8192, max_edges=400_000)
    d.update(cfg)
    d.update(kw)
    return static_layer.StaticLayer(lp, static_layer.shipped_config(**d))


def refused(code, fn, *a):
    with pytest.raises(RolloutError) as e:
        fn(*a)
    assert e.value.code == code, (e.value.code, str(e.value))


def same_bits(got, ref, name=""):
    """row_start and neighbour as integers, weight as uint32 patterns, the dGraph as uint64 patterns"""
    g = got["graph"]
    np.testing.assert_array_equal(g["row_start"], ref["row_start"], err_msg=name)
    np.testing.assert_array_equal(g["neighbour"], ref["neighbour"], err_msg=name)
    np.testing.assert_array_equal(g["weight"].view(np.uint32), ref["weight"].view(np.uint32), err_msg=name)
    np.testing.assert_array_equal(got["dgraph"].view(np.uint64), ref["dgraph"].view(np.uint64), err_msg=name)


def run(lp, name, **kw):
    c = Cs.all_cases()[name]
    sl = layer(lp, c["cfg"], **kw)
    st = sl.build(c["ground"], c["map"])
    return sl, st, dict(graph=sl.graph(), dgraph=sl.dgraph())


@pytest.mark.parametrize("name", ("floor", "floor_adaptive", "floor_shifted", "long_row", "n_ground_1", "empty_map", "graph_off", "edge_off"))
def test_build_matches_the_restatement(lp, name):
    """The floor in fixed and adaptive mode, the floor shifted by (4000, -3000, 100) m, the clump whose rows exceed the LDS
    row budget and the four small cases: every array bit for bit, and the counters."""
    ref = Cs.reference(name)
    sl, st, got = run(lp, name)
    c = Cs.all_cases()[name]
    deg = np.diff(ref["row_start"].astype(np.int64))
    print(f"{name}: {st.n_ground} nodes, {st.n_map} map points, {st.n_edges} edges, max degree {st.max_degree}, long rows {st.n_long_rows}, "
          f"overhang {st.n_overhang}, near {st.n_near_obstacle}, launches {st.launches}, waits {st.host_waits}")
    assert (st.n_ground, st.n_map, st.n_edges) == (len(c["ground"]), len(c["map"]), len(ref["neighbour"]))
    assert st.max_degree == int(deg.max()) and st.n_long_rows == int((deg > Cs.row_lds()).sum())
    assert st.n_overhang == int(ref["overhang"].sum()) and st.n_near_obstacle == int(ref["near"].sum())
    assert st.host_waits == 2
    same_bits(got, ref, name)
    if name == "long_row":
        assert st.n_long_rows >= 1
    if name == "graph_off":
        assert st.n_edges == 0 and (got["graph"]["row_start"] == 0).all()
    assert got["dgraph"][-1] == c["cfg"]["max_obstacle_distance"]           # entry n_ground is never written


def test_a_build_beyond_max_edges_leaves_the_previous_one(lp):
    ref = Cs.reference("edge_off")
    sl, st, got = run(lp, "edge_off", max_edges=len(ref["neighbour"]))       # exactly enough
    same_bits(got, ref)
    big = Cs.all_cases()["empty_map"]                                        # the same ground: as many edges
    sl2 = layer(lp, big["cfg"], max_edges=len(ref["neighbour"]) - 1)
    m = Cs.mini()
    first = sl2.build(m["ground"][:100], m["map"])
    keep = dict(graph=sl2.graph(), dgraph=sl2.dgraph())
    refused(K.ERR_CAPACITY, sl2.build, big["ground"], big["map"])
    assert sl2.last.n_edges == len(ref["neighbour"])                         # the true count
    sl2.n_ground = int(first.n_ground)
    after = dict(graph=sl2.graph(), dgraph=sl2.dgraph())
    for k in ("row_start", "neighbour", "weight"):
        assert keep["graph"][k].tobytes() == after["graph"][k].tobytes()
    assert keep["dgraph"].tobytes() == after["dgraph"].tobytes()
    # more points than created for, an empty ground, a coordinate that is not finite, a cloud too wide
    refused(K.ERR_CAPACITY, sl2.build, np.zeros((5000, 3), F), m["map"])
    refused(K.ERR_BAD_ARG, sl2.build, np.zeros((0, 3), F), m["map"])
    bad = m["ground"][:50].copy()
    bad[3, 2] = np.nan
    refused(K.ERR_BAD_ARG, sl2.build, bad, m["map"])
    wide = m["ground"][:50].copy()
    wide[0, 0] += 5000.0
    refused(K.ERR_BAD_ARG, sl2.build, wide, m["map"])
    assert keep["dgraph"].tobytes() == sl2.dgraph().tobytes()
    for n in (0, 33):
        refused(K.ERR_BAD_ARG, layer, lp, R.config(use_adaptive_connection=1, adaptive_connection_number=n))


def test_zones(lp):
    """Both zones, then one, then none; a zone point farther than the inflation distance from every node changes nothing."""
    c = Cs.floor()
    sl = layer(lp, c["cfg"])
    a, b = Cs.zone_sets()
    refused(K.ERR_STATE, sl.set_zones, a, Cs.INFLATION)                      # before any build
    sl.build(c["ground"], c["map"])
    refused(K.ERR_STATE, sl.zone_dgraph)
    mod = c["cfg"]["max_obstacle_distance"]
    for pts in (np.concatenate([a, b]), a, b[-1:], np.zeros((0, 3), F)):
        want = R.zones(c["ground"], pts, Cs.INFLATION, mod)
        st = sl.set_zones(pts, Cs.INFLATION)
        got = sl.zone_dgraph()
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        assert st.n_zone_points == len(pts) and st.n_zone_nodes == int((want[:-1] < mod).sum())
        if len(pts) <= 1:
            assert (got == mod).all()
    assert (R.zones(c["ground"], a, Cs.INFLATION, mod) < mod).sum() > 50
    # a new build drops the zones' dGraph
    sl.build(c["ground"], c["map"])
    refused(K.ERR_STATE, sl.zone_dgraph)
    refused(K.ERR_STATE, sl.bind, 1, 0)


def test_bind_equals_set_host_layer(lp, lp2):
    c = Cs.floor()
    n = len(c["ground"])
    a, b = Cs.zone_sets()
    sl = layer(lp, c["cfg"])
    refused(K.ERR_STATE, sl.bind, 0, 0)                                      # no build yet (and this context may have no stack)
    sl.build(c["ground"], c["map"])
    sl.set_zones(np.concatenate([a, b]), Cs.INFLATION)
    st1 = stack.PerceptionStack(lp, host_layers=(None, None), n_ground=n, max_changes=n + 1)
    sl.bind(0, 0)
    sl.bind(1, 1)
    st1.update()
    st2 = stack.PerceptionStack(lp2, host_layers=(sl.dgraph(), sl.zone_dgraph()), n_ground=n, max_changes=n + 1)
    st2.update()
    assert st1.min_dgraph().tobytes() == st2.min_dgraph().tobytes()
    want = np.minimum(np.minimum(sl.dgraph(), sl.zone_dgraph()), K.STACK_START)
    assert st1.min_dgraph().tobytes() == want.tobytes()
    c1, c2 = st1.changes(), st2.changes()
    as_set = lambda ch: set(zip(ch[0].tolist(), ch[1].view(np.uint64).tolist(), ch[2].tolist()))
    assert as_set(c1) == as_set(c2) and len(c1[0]) == n + 1
    refused(K.ERR_BAD_ARG, sl.bind, 0, 2)
    refused(K.ERR_BAD_ARG, sl.bind, 0, -1)
    refused(K.ERR_BAD_ARG, sl.bind, 2, 0)
    # a stack of another n_ground: refused, the slot as it was
    st3 = stack.PerceptionStack(lp, host_layers=(np.full(n + 3, 7.0), None), n_ground=n + 2, max_changes=n + 3)
    st3.update()
    keep = st3.min_dgraph()
    refused(K.ERR_BAD_ARG, sl.bind, 0, 0)
    refused(K.ERR_BAD_ARG, sl.bind, 1, 1)
    st3.update()
    assert st3.min_dgraph().tobytes() == keep.tobytes() and st3.last.n_changed == 0 and (keep == 7.0).all()


def test_every_entry_is_refused_beside_a_pending_tick(lp):
    c = Cs.mini()
    sl = layer(lp, c["cfg"])
    sl.build(c["ground"], c["map"])
    a, _ = Cs.zone_sets()
    sl.set_zones(a, Cs.INFLATION)
    keep = dict(graph=sl.graph(), dgraph=sl.dgraph())
    zkeep = sl.zone_dgraph()
    stack.PerceptionStack(lp, host_layers=(None,), n_ground=len(c["ground"]))
    sc = scenes.bench_scene("C2")
    lp.set_cloud(sc.cloud)
    lp.setPlan(sc.plan)
    name = sc.theory.name.decode()
    before = lp.tick(name, sc.tick)
    lp.tick_begin(name, sc.tick)
    try:
        for call in (lambda: sl.build(c["ground"], c["map"]), sl.graph, sl.dgraph, lambda: sl.set_zones(a, Cs.INFLATION), sl.zone_dgraph,
                     lambda: sl.bind(0, 0), lambda: layer(lp, c["cfg"])):
            refused(K.ERR_STATE, call)
    finally:
        lp.tick_end()
    after_graph = dict(graph=sl.graph(), dgraph=sl.dgraph())
    same_bits(after_graph, dict(row_start=keep["graph"]["row_start"], neighbour=keep["graph"]["neighbour"], weight=keep["graph"]["weight"], dgraph=keep["dgraph"]))
    assert sl.zone_dgraph().tobytes() == zkeep.tobytes()
    # a tick after a build gives what it gave before
    sl.build(c["ground"], c["map"])
    after = lp.tick(name, sc.tick)
    upto = K.RolloutResult.device_ms.offset                                  # everything but the two timings
    assert bytes(after)[:upto] == bytes(before)[:upto]
