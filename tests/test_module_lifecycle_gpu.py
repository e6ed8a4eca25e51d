"""Module states that are created again and again during a context's life: the lidar marking layer, the depth camera's
selfMark, the depth layer, the perception stack over them, the particle measure and its prepared observation.  Every
create tears the old state down (the states own their memory and free it when they die) and builds the next; what a
later create must drop -- the stack over a layer that is made again, the map of a particle measure that is made again,
the prepared observation of one that is configured again -- must be gone.  One context runs the whole sequence twice and
is then closed; after every step its products must be those of a context that saw only that step's configuration.

How that is compared.  The perception products (voxels, dGraph, lethal set, cluster lists, stacked arrays, change list)
depend on the order of the observation's points, and the feeds append their points in the order their waves finish: two
contexts fed alike may hold them in another order.  So, as in the modules' own GPU tests whose helpers this file uses,
the fresh state each step is compared with is the module's restatement, made anew for that step and fed the observation
the device holds: stats and sets equal, floats bit for bit.  The particle measure reads only what the host hands it:
there each step is compared bit for bit with a fresh context that ran that step alone.

The cases are the smallest of tests/helpers/*_cases.py with a lidar beside two depth cameras that leave no product
empty: the first updates of stack_cases' sequence, depth_mark_cases' lidar_beside, 8 particles of the room."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, localization, marking
from dddmr_navigation_amd.stack import PerceptionStack
from conftest import ROOT
import oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_clear_cases as dcases  # noqa: E402
import depth_frustum_ref as R  # noqa: E402
import depth_layer_cases as lcases  # noqa: E402
import depth_mark_cases as mcases  # noqa: E402
import mcl_measure_cases as MC  # noqa: E402
import mcl_observation_cases as OC  # noqa: E402
import stack_cases as sc  # noqa: E402
import stack_ref as S  # noqa: E402
import test_depth_layer_gpu as TL  # noqa: E402  (planner, configure, feed, make_layer, assert_state)
import test_depth_mark_gpu as TM  # noqa: E402  (configure, feed, create, assert_equal)
import test_mcl_observation_gpu as TO  # noqa: E402  (mcl_config, obs_config)
import test_stack_gpu as TS  # noqa: E402  (assert_full, assert_changes, refused, LIDAR_FIELDS)

pytestmark = pytest.mark.gpu

NO_MAP = TS.NO_MAP
N_PARTICLES = 8


# ---- the perception modules: steps 1 to 4 ---------------------------------------------------------------------------------
def lidar_layer(lp, ground):
    """a new lidar layer (the context's old one dies) with a restatement as new as it is"""
    return marking.MarkingLayer(lp, sc.marking_config(), ground, NO_MAP), oracle.MarkingOracle(sc.marking_config(), ground, NO_MAP)


def assert_lidar(ml, mo, st, so, what):
    assert tuple(int(getattr(st, f)) for f in TS.LIDAR_FIELDS) == tuple(int(getattr(so, f)) for f in TS.LIDAR_FIELDS), what
    assert set(map(tuple, ml.voxels().tolist())) == set(map(tuple, mo.voxels().tolist())), what
    np.testing.assert_array_equal(TS.bits(ml.dgraph()), TS.bits(mo.dgraph()), err_msg=what)
    np.testing.assert_array_equal(ml.lethal(), mo.lethal(), err_msg=what)


def lidar_update(lp, ml, mo, u, what):
    """feeds the update's scan and runs the layer on the aggregate, as marking_update does"""
    TL.feed(lp, u["feeds"][0])
    st = ml.update(mcases.TBS_LIDAR, u["t_gb"])
    so = mo.update(lp.get_cloud()[:, :3], mcases.TBS_LIDAR, u["t_gb"])
    assert_lidar(ml, mo, st, so, what)
    assert st.n_marked > 0 and len(ml.voxels()) > 0 and ml.lethal().any(), what


def lidar_stack(lp, ml, mo, n_nodes, what):
    stack = PerceptionStack(lp, ml, order=(K.STACK_LIDAR,))
    tr = S.Tracker(n_nodes)
    tr.publish([(mo.dgraph(), mo.lethal())])
    TS.assert_full(stack, tr, what)
    assert tr.mask.any(), what
    return stack


def assert_no_stack(stack, what):
    for fn in (stack.min_dgraph, stack.lethal_mask, stack.update):
        with pytest.raises(TS.RolloutError, match="before stack_create") as e:
            fn()
        assert e.value.code == K.ERR_STATE, what


def depth_mark_twice(lp, what):
    case, steps, _, frs, _, ground, smap, _ = mcases.built("lidar_beside")
    TM.configure(lp, case)
    n_lidar = sum(TM.feed(lp, st) or 0 for st in steps)
    obs = lp.get_cloud()[n_lidar:, :3]
    ref = mcases.restate(case, frs, obs, ground, smap)
    assert ref["stats"]["n_accepted"] > 0
    for max_obs in (1 << 16, 1 << 15):
        TM.create(lp, case, ground, smap, max_obs=max_obs)
        TM.assert_equal(lp.depth_mark_clusters(case.t_gb), ref, f"{what}, max_observation_points {max_obs}")


def perception_steps(lp, what):
    b = sc.built()
    case, ups, ground = b["case"], b["ups"], b["ground"]
    n_nodes = len(ground) + 1
    TL.configure(lp, case)
    # 1. the lidar layer, updated once, and a stack over it
    ml, mo = lidar_layer(lp, ground)
    lidar_update(lp, ml, mo, ups[0], f"{what}, step 1")
    stack = lidar_stack(lp, ml, mo, n_nodes, f"{what}, step 1: stack")
    # 2. the lidar layer a second time: the stack is gone; a new layer, updated, takes a new stack
    ml, mo = lidar_layer(lp, ground)
    assert_no_stack(stack, f"{what}, step 2")
    lidar_update(lp, ml, mo, ups[1], f"{what}, step 2")
    stack = lidar_stack(lp, ml, mo, n_nodes, f"{what}, step 2: stack")
    # 3. the depth camera's selfMark, created twice
    depth_mark_twice(lp, f"{what}, step 3")
    # 4. the depth layer twice, the second with other capacities: the stack is gone again; then a stack over both layers
    TL.configure(lp, case)
    TL.make_layer(lp, case, ground)
    assert_no_stack(stack, f"{what}, step 4")
    dl = TL.make_layer(lp, case, ground, max_markings=2 * case.max_markings, max_cluster_points=2 * case.max_cluster_points)
    dref = lcases.layer_ref(case, ground)
    stack = PerceptionStack(lp, ml, dl, order=(K.STACK_LIDAR, K.STACK_DEPTH))
    tr = S.Tracker(n_nodes)
    layers = lambda: [(mo.dgraph(), mo.lethal()), (dref.dgraph, dref.lethal)]
    tr.publish(layers())
    TS.assert_full(stack, tr, f"{what}, step 4: stack")
    u, frs, n_lidar = ups[0], {}, 0
    for st in u["feeds"]:
        n_lidar += TL.feed(lp, st)
        if st["kind"] != "lidar":
            frs[st["sid"]] = R.Frustum(dcases.FOV_W, dcases.FOV_V, dcases.D_MIN, dcases.D_MAX, st["m2s"])
    cloud = lp.get_cloud()                                 # the aggregate is in source order: lidar first
    st = stack.update(mcases.TBS_LIDAR, u["t_gb"])
    assert st.lidar_rc == st.depth_rc == K.OK and st.depth_skipped == 0
    so = mo.update(cloud[:n_lidar, :3], mcases.TBS_LIDAR, u["t_gb"])
    res = dref.update([frs[s] for s in sorted(frs)], cloud[n_lidar:, :3], u["t_gb"])
    assert_lidar(ml, mo, st.lidar, so, f"{what}, step 4: lidar layer")
    TL.assert_state(dl, st.depth, dref, res, f"{what}, step 4: depth layer")
    want = tr.step(layers())
    TS.assert_changes(stack, tr, want, f"{what}, step 4: changes")
    TS.assert_full(stack, tr, f"{what}, step 4: stacked")
    assert st.depth.n_accepted > 0 and dref.lethal.any() and len(want) > 0, what


# ---- the particle measure: steps 5 to 7 -----------------------------------------------------------------------------------
def mcl_inputs():
    room = MC.room_case(4242, N_PARTICLES, 40, 200)
    return room, OC.flat_case(100)[0], OC.case("islands")[0]


def step_measure(pm):
    room = mcl_inputs()[0]
    pm.set_map(room["map"], room["ground"], room["normals"])
    like, qual = pm.measure(room["flat"], room["ls"], room["states"])
    assert qual.max() > 0.0
    return dict(likelihood=like, quality=qual, stats=np.frombuffer(bytes(pm.last), np.uint8), **pm.terms(N_PARTICLES))


def step_prepared(pm):
    room, flat, ls = mcl_inputs()
    pm.configure_observation(TO.obs_config())
    st = pm.prepare(flat, ls, OC.T_B2S)
    f, l, nrm = pm.observation()
    like, qual = pm.measure_prepared(room["states"])
    assert len(f) > 0 and len(l) > 0 and len(nrm) > 0 and qual.max() > 0.0
    return dict(flat=f, less_sharp=l, normals=nrm, prepare_stats=np.frombuffer(bytes(st), np.uint8), likelihood=like, quality=qual,
                stats=np.frombuffer(bytes(pm.last), np.uint8))


_FRESH = {}


def fresh_mcl():
    """each step's products from a context that ran that step alone, computed once"""
    if not _FRESH:
        with TL.planner() as lp:
            _FRESH["measure"] = step_measure(localization.ParticleMeasure(lp, TO.mcl_config()))
        with TL.planner() as lp:
            pm = localization.ParticleMeasure(lp, TO.mcl_config())
            pm.set_map(*(mcl_inputs()[0][k] for k in ("map", "ground", "normals")))
            _FRESH["prepared"] = step_prepared(pm)
    return _FRESH


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), f"{what}: {key}"


def mcl_steps(lp, what):
    fresh = fresh_mcl()
    states = mcl_inputs()[0]["states"]
    # 5. create, set_map, measure
    pm = localization.ParticleMeasure(lp, TO.mcl_config())
    assert_same(step_measure(pm), fresh["measure"], f"{what}, step 5")
    # 6. the observation on, prepared and measured; off: measure_prepared refuses; on again
    assert_same(step_prepared(pm), fresh["prepared"], f"{what}, step 6")
    pm.configure_observation(None)
    with pytest.raises(TS.RolloutError, match="before mcl_set_observation_config") as e:
        pm.measure_prepared(states)
    assert e.value.code == K.ERR_STATE
    assert_same(step_prepared(pm), fresh["prepared"], f"{what}, step 6, on again")
    assert_same(step_measure(pm), fresh["measure"], f"{what}, step 6: measure beside the observation")
    # 7. a second create forgets the map
    pm = localization.ParticleMeasure(lp, TO.mcl_config())
    room = mcl_inputs()[0]
    with pytest.raises(TS.RolloutError, match="before mcl_set_map") as e:
        pm.measure(room["flat"], room["ls"], states)
    assert e.value.code == K.ERR_STATE


def test_modules_created_again_deliver_what_fresh_ones_deliver():
    with TL.planner() as lp:
        for round_ in range(2):
            perception_steps(lp, f"round {round_}")
            mcl_steps(lp, f"round {round_}")
    # 8. close: the context's exit above released every module with the device current
