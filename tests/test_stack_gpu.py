"""GPU parity of the perception stack (dddmr_rollout_stack_*).  Every array comparison is EQUALITY OF BIT PATTERNS.

Expected values come from the restatements alone: oracle.MarkingOracle fed the lidar part of get_cloud(),
tests/helpers/depth_layer_ref.py fed the depth part, tests/helpers/stack_ref.py for the minimum, the masks and the changed
set.  The sequence is tests/helpers/stack_cases.py's; tests/test_stack_cpu.py asserts on the CPU that it is adequate."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, depth_layer, marking, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from dddmr_navigation_amd.stack import PerceptionStack
from conftest import ROOT
import oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_clear_cases as dcases  # noqa: E402
import depth_frustum_ref as R  # noqa: E402
import depth_layer_cases as cases  # noqa: E402
import depth_mark_cases as mc  # noqa: E402
import stack_cases as sc  # noqa: E402
import stack_ref as S  # noqa: E402
import test_depth_layer_gpu as T  # noqa: E402  (configure, feed, make_layer, assert_state: the depth layer's own assertions)

pytestmark = pytest.mark.gpu

NO_MAP = np.zeros((0, 3), np.float32)
LIDAR_FIELDS = ("n_observation", "n_clusters", "n_marked", "n_in_window", "n_cleared", "n_alive")
SPECIALS = (np.nan, np.inf, -np.inf, 123456.0, S.START, np.nextafter(S.START, 0.0), 0.0, -0.0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def refused(code, fn, *a):
    with pytest.raises(RolloutError) as e:
        fn(*a)
    assert e.value.code == code, e.value


def assert_full(stack, tr, what):
    np.testing.assert_array_equal(bits(stack.min_dgraph()), bits(tr.values), err_msg=what)
    np.testing.assert_array_equal(stack.lethal_mask(), tr.mask, err_msg=what)


def assert_changes(stack, tr, want, what):
    """the list against the expected set: each node once, values and masks equal to the full arrays at those nodes"""
    assert stack.last.n_changed == stack.n_changes() == len(want), what
    if len(want) > stack.cfg.max_changes:
        refused(K.ERR_CAPACITY, stack.changes)
        return None
    node, value, mask = stack.changes()
    assert len(node) == len(set(node.tolist())) == len(want) and set(node.tolist()) == set(want.tolist()), what
    np.testing.assert_array_equal(bits(value), bits(tr.values[node]), err_msg=what)
    np.testing.assert_array_equal(mask, tr.mask[node], err_msg=what)
    return node, value, mask


# ---- 1. the kernel's shapes, host layers only -------------------------------------------------------------------------
def host_values(rng, n, with_neg_inf):
    v = rng.uniform(0.0, 200000.0, n)                              # about half above the start value
    sp = [s for s in SPECIALS if with_neg_inf or not (np.isinf(s) and s < 0)]
    at = rng.integers(0, n, size=min(n, len(sp)))
    for i, s in zip(at, sp):
        v[i] = s
    return v


def kernel_sequence(lp, n_nodes, n_layers, max_changes, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    what = f"{n_nodes} nodes, {n_layers} host layers, max_changes {max_changes}"
    stack = PerceptionStack(lp, host_layers=[None] * n_layers, n_ground=n_nodes - 1, max_changes=max_changes)
    tr = S.Tracker(n_nodes)
    layers = [(None, None)] * n_layers
    tr.publish(layers)
    assert stack.n_changes() == 0 and len(stack.changes()[0]) == 0, what
    assert_full(stack, tr, what + " after create")
    assert (tr.values == S.START).all()

    def step(slot, values, expect, tag):
        layers[slot] = (values, None)
        stack.set_host_layer(slot, values)
        stack.update()
        want = tr.step(layers)
        if expect is not None:
            assert len(want) == expect, (what, tag)                # (the case really is what it is named)
        got = assert_changes(stack, tr, want, f"{what}: {tag}")
        assert_full(stack, tr, f"{what}: {tag}")
        return got

    # only slot 0 ever holds -inf, so that replacing it can change every node
    for slot in range(n_layers):
        step(slot, host_values(rng, n_nodes, slot == 0), None, f"slot {slot} set")
    step(0, layers[0][0].copy(), 0, "(a) replaced by itself")
    others = S.stacked(layers[1:])[0] if n_layers > 1 else np.full(n_nodes, S.START)
    v = layers[0][0].copy()
    i = int(rng.integers(0, n_nodes))
    v[i] = (min(tr.values[i], 0.0) - 1.0) if np.isfinite(tr.values[i]) else -5.0      # (-inf there is slot 0's own)
    step(0, v, 1, "(b) one node")
    v = others - 1.0 - rng.uniform(0.0, 1.0, n_nodes)
    step(0, v, n_nodes, "(c) every node")                           # max_changes = n_nodes: fits; one below: ERR_CAPACITY, n exact
    v = v.copy()
    v[i] -= 1.0
    step(0, v, 1, "one node after (c)")                             # the list is right again after an overflow
    assert stack.last.lidar_rc == stack.last.depth_rc == K.OK and stack.last.depth_skipped == 0


@pytest.mark.parametrize("n_nodes", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_kernel_shapes_with_host_layers_only(n_nodes):
    with LocalPlanner([configs.bench_theory("C2")], max_points=1024) as lp:
        for n_layers in (1, 2, 3, 4):
            for max_changes in (n_nodes, n_nodes - 1):
                kernel_sequence(lp, n_nodes, n_layers, max_changes, 1000 * n_nodes + 10 * n_layers)


# ---- 2. the whole stack after every update ----------------------------------------------------------------------------
class Rig:
    """one context with the sequence's sources, both layers (or one) and their restatements"""

    def __init__(self, lp, lidar=True, depth=True, host=True, max_changes=4096):
        b = sc.built()
        self.lp, self.case, self.ups, self.ground = lp, b["case"], b["ups"], b["ground"]
        self.n = len(self.ground)
        T.configure(lp, self.case)
        self.ml = marking.MarkingLayer(lp, sc.marking_config(), self.ground, NO_MAP) if lidar else None
        self.dl = T.make_layer(lp, self.case, self.ground) if depth else None
        self.mo = oracle.MarkingOracle(sc.marking_config(), self.ground, NO_MAP)
        self.dref = cases.layer_ref(self.case, self.ground)
        self.order = tuple(o for o in sc.ORDER if (o == K.STACK_LIDAR and lidar) or (o == K.STACK_DEPTH and depth) or (o == K.STACK_HOST0 and host))
        self.stack = PerceptionStack(lp, self.ml, self.dl, [None] if host else [], order=self.order, max_changes=max_changes)
        self.static = b["static"] if host else None
        self.tr = S.Tracker(self.n + 1)
        self.tr.publish(self.layers(host_set=False))
        if host:
            self.stack.set_host_layer(0, self.static)
        self.frs, self.n_lidar = {}, 0

    def layers(self, host_set=True):
        by = {K.STACK_HOST0: (self.static if host_set else None, None),
              K.STACK_LIDAR: (self.mo.dgraph(), self.mo.lethal()),
              K.STACK_DEPTH: (self.dref.dgraph, self.dref.lethal)}
        return [by[o] for o in self.order]

    def feed(self, u, frustum=True, kinds=("lidar", "frame", "image")):
        for st in u["feeds"]:
            if st["kind"] not in kinds:
                continue
            n = T.feed(self.lp, st, frustum=frustum)
            if st["kind"] == "lidar":
                self.n_lidar = n
            elif frustum:
                self.frs[st["sid"]] = R.Frustum(dcases.FOV_W, dcases.FOV_V, dcases.D_MIN, dcases.D_MAX, st["m2s"])

    def observations(self):
        cloud = self.lp.get_cloud()                                  # the aggregate is in source order: lidar first
        return cloud[: self.n_lidar, :3], cloud[self.n_lidar:, :3]

    def assert_lidar(self, sm, so, what):
        assert tuple(int(getattr(sm, f)) for f in LIDAR_FIELDS) == tuple(int(getattr(so, f)) for f in LIDAR_FIELDS), what
        assert set(map(tuple, self.ml.voxels().tolist())) == set(map(tuple, self.mo.voxels().tolist())), what
        np.testing.assert_array_equal(bits(self.ml.dgraph()), bits(self.mo.dgraph()), err_msg=what)
        np.testing.assert_array_equal(self.ml.lethal(), self.mo.lethal(), err_msg=what)

    def assert_stack(self, what, mirror=None):
        want = self.tr.step(self.layers())
        got = assert_changes(self.stack, self.tr, want, what)
        assert_full(self.stack, self.tr, what)
        dev_pos = [p for p, o in enumerate(self.order) if o < K.STACK_HOST0]
        np.testing.assert_array_equal(self.stack.lethal_nodes(), S.lethal_nodes(self.tr.mask, dev_pos, self.n), err_msg=what)
        if mirror is not None:
            S.apply_changes(mirror[0], mirror[1], *got)
            np.testing.assert_array_equal(bits(mirror[0]), bits(self.stack.min_dgraph()), err_msg=what + ": mirror")
            np.testing.assert_array_equal(mirror[1], self.stack.lethal_mask(), err_msg=what + ": mirror")
        return want


def test_the_whole_stack_after_every_update():
    with T.planner() as lp:
        rig = Rig(lp)
        assert_full(rig.stack, rig.tr, "after create")
        mirror = (rig.stack.min_dgraph(), rig.stack.lethal_mask())
        for k, u in enumerate(rig.ups):
            what = f"update {k}"
            rig.feed(u)
            lidar_obs, depth_obs = rig.observations()
            st = rig.stack.update(mc.TBS_LIDAR, u["t_gb"])
            assert st.lidar_rc == st.depth_rc == K.OK and st.depth_skipped == 0
            so = rig.mo.update(lidar_obs, mc.TBS_LIDAR, u["t_gb"])
            res = rig.dref.update([rig.frs[s] for s in sorted(rig.frs)], depth_obs, u["t_gb"])
            rig.assert_lidar(st.lidar, so, what)
            T.assert_state(rig.dl, st.depth, rig.dref, res, what)
            want = rig.assert_stack(what, mirror)
            print(f"{what}: {len(lidar_obs)} lidar + {len(depth_obs)} depth points, {len(want)} of {rig.n + 1} nodes changed, "
                  f"{st.launches} launches, {st.host_waits} host waits")
            assert st.launches > 0 and st.host_waits >= 3


def test_marking_update_in_the_same_context_still_takes_the_whole_aggregate():
    """the entry the stack does not replace: in a context with depth sources it marks their points too, as before"""
    with T.planner() as lp:
        rig = Rig(lp)
        u = rig.ups[0]
        rig.feed(u)
        whole = lp.get_cloud()[:, :3]
        sm = rig.ml.update(mc.TBS_LIDAR, u["t_gb"])
        so = rig.mo.update(whole, mc.TBS_LIDAR, u["t_gb"])
        assert sm.n_observation == len(whole) > rig.n_lidar
        rig.assert_lidar(sm, so, "marking_update beside a stack")


# ---- 3. stack against the stand-alone entries, device against device --------------------------------------------------
def device_state(layer, with_clusters):
    out = [set(map(tuple, layer.voxels().tolist())), bits(layer.dgraph()).tobytes(), np.asarray(layer.lethal()).tobytes()]
    if with_clusters:
        out.append(T.device_store(layer))
    return out


# The feeds compact their survivors with one counter add per wave (and the lidar feed emits its voxels in the order they
# were claimed), so two contexts fed the same scan hold the same points in an order that can differ from run to run, and
# both layers sum floats in observation order.  "The same scans" therefore has to mean the same observation, point for
# point: the second lidar context is handed the first one's observation (marking_update reads any aggregate), and the
# depth contexts are fed frames of at most 64 points, which one wave compacts in lane order.
def store_points(layer):
    """the store's generator points with their voxels, as a sorted list of bit patterns (slot order is the hash table's)"""
    pts, vox = layer.points(with_voxels=True)
    return sorted(zip(map(tuple, vox.tolist()), map(tuple, pts.view(np.uint32).tolist())))


def test_a_lidar_only_stack_equals_marking_update():
    with T.planner() as a, T.planner() as b:
        ra, rb = Rig(a, depth=False, host=False), Rig(b, depth=False, host=False)
        for k, u in enumerate(ra.ups):
            ra.feed(u, kinds=("lidar",))
            obs = a.get_cloud()
            assert len(obs) == ra.n_lidar > 5
            b.set_cloud(obs)
            assert b.get_cloud().tobytes() == obs.tobytes()
            sa = ra.stack.update(mc.TBS_LIDAR, u["t_gb"]).lidar
            sb = rb.ml.update(mc.TBS_LIDAR, u["t_gb"])
            assert tuple(int(getattr(sa, f)) for f in LIDAR_FIELDS) == tuple(int(getattr(sb, f)) for f in LIDAR_FIELDS), k
            assert device_state(ra.ml, False) == device_state(rb.ml, False), k
            assert store_points(ra.ml) == store_points(rb.ml), k
            np.testing.assert_array_equal(bits(ra.stack.min_dgraph()), bits(rb.ml.dgraph()))       # (all below the start value)
        assert sa.n_marked > 0
        ca, cb = ra.ml.route_counts(), rb.ml.route_counts()
        assert (ca["fused"], ca["general"]) == (cb["fused"], cb["general"]) and ca["fused"] + ca["general"] == len(ra.ups)


def one_wave_frame(k, cam):
    """63 points in the camera's frame (x ahead): three blobs out of five places, which three depends on the update, so
    that blobs of the update before are gone (cleared) and new ones stand (marked)"""
    rng = np.random.Generator(np.random.PCG64(900 + 10 * k + cam))
    places = np.array([[1.6, -0.5, 0.1], [2.0, 0.0, 0.15], [2.4, 0.5, 0.2], [2.8, -0.3, 0.1], [1.8, 0.4, 0.25]])
    pick = [(k + j + cam) % 5 for j in (0, 2, 3)]
    pts = np.concatenate([places[p] + rng.uniform(-0.04, 0.04, (21, 3)) for p in pick], axis=0)
    return pts.astype(np.float32)


def test_a_depth_only_stack_equals_depth_layer_update():
    with T.planner() as a, T.planner() as b:
        ra, rb = Rig(a, lidar=False, host=False), Rig(b, lidar=False, host=False)
        accepted = cleared = 0
        for k, u in enumerate(ra.ups):
            for st in u["feeds"]:
                if st["kind"] == "lidar":
                    continue
                small = dict(st, kind="frame", data=one_wave_frame(k, st["sid"]))
                T.feed(a, small)
                T.feed(b, small)
            obs = a.get_cloud()
            assert obs.tobytes() == b.get_cloud().tobytes() and len(obs) > 5, k
            sa = ra.stack.update(None, u["t_gb"]).depth
            sb = rb.dl.update(u["t_gb"])
            assert {f: int(getattr(sa, f)) for f in T.STAT_FIELDS} == {f: int(getattr(sb, f)) for f in T.STAT_FIELDS}, k
            assert device_state(ra.dl, True) == device_state(rb.dl, True), k
            accepted += int(sa.n_accepted)
            cleared += int(sa.n_cleared)
        assert accepted > 0 and cleared > 0            # both halves of the pass were compared


# ---- 4. a camera without a frustum yet --------------------------------------------------------------------------------
def test_a_camera_without_a_frustum_skips_the_depth_layer_only():
    with T.planner() as lp:
        rig = Rig(lp)
        u = rig.ups[0]
        rig.feed(u, frustum=False)
        lidar_obs, _ = rig.observations()
        before = device_state(rig.dl, True)
        st = rig.stack.update(mc.TBS_LIDAR, u["t_gb"])                # returns DDDMR_OK (no exception)
        assert st.depth_skipped == 1 and st.depth_rc == K.OK and st.lidar_rc == K.OK
        assert device_state(rig.dl, True) == before and len(before[0]) == 0
        so = rig.mo.update(lidar_obs, mc.TBS_LIDAR, u["t_gb"])
        assert so.n_marked > 0
        rig.assert_lidar(st.lidar, so, "lidar beside a skipped depth layer")
        rig.assert_stack("depth layer skipped")
        refused(K.ERR_STATE, rig.dl.update, u["t_gb"])                # the stand-alone entry still refuses
        # once the frustums are there the depth layer joins in
        rig.feed(rig.ups[1])
        lidar_obs, depth_obs = rig.observations()
        st = rig.stack.update(mc.TBS_LIDAR, rig.ups[1]["t_gb"])
        so = rig.mo.update(lidar_obs, mc.TBS_LIDAR, rig.ups[1]["t_gb"])
        res = rig.dref.update([rig.frs[s] for s in sorted(rig.frs)], depth_obs, rig.ups[1]["t_gb"])
        assert st.depth_skipped == 0 and st.depth.n_accepted > 0
        T.assert_state(rig.dl, st.depth, rig.dref, res, "after the frustums arrived")
        rig.assert_stack("after the frustums arrived")


# ---- 5. reset and errors ----------------------------------------------------------------------------------------------
def test_reset_in_mid_sequence():
    with T.planner() as lp:
        rig = Rig(lp)
        for k, u in enumerate(rig.ups):
            what = f"update {k}"
            rig.feed(u)
            lidar_obs, depth_obs = rig.observations()
            if k == sc.RESET_AT:
                rig.stack.reset()
                rig.mo.reset()
                rig.dref.reset()
                rig.tr.publish(rig.layers())
                assert rig.stack.n_changes() == 0 and len(rig.stack.changes()[0]) == 0
                assert_full(rig.stack, rig.tr, "after reset")
                assert len(rig.ml.voxels()) == 0 and len(rig.dl.voxels()) == 0
            st = rig.stack.update(mc.TBS_LIDAR, u["t_gb"])
            so = rig.mo.update(lidar_obs, mc.TBS_LIDAR, u["t_gb"])
            res = rig.dref.update([rig.frs[s] for s in sorted(rig.frs)], depth_obs, u["t_gb"])
            rig.assert_lidar(st.lidar, so, what)
            T.assert_state(rig.dl, st.depth, rig.dref, res, what)
            rig.assert_stack(what)


def test_error_paths_leave_the_context_usable():
    b = sc.built()
    ground, u0 = b["ground"], b["ups"][0]
    sc2 = scenes.bench_scene("C2")
    with T.planner() as lp:
        # stack calls before create
        st = K.StackStats()
        tf = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
        n = C.c_size_t(0)
        buf = np.zeros(len(ground) + 1, np.float64)
        lib, ctx = lp._lib, lp._ctx
        assert lib.dddmr_rollout_stack_update(ctx, tf, tf, C.byref(st)) == K.ERR_STATE
        assert lib.dddmr_rollout_stack_get_changes(ctx, None, None, None, 0, C.byref(n)) == K.ERR_STATE
        assert lib.dddmr_rollout_stack_get_min_dgraph(ctx, buf.ctypes.data_as(C.c_void_p), buf.size) == K.ERR_STATE
        assert lib.dddmr_rollout_stack_get_lethal_mask(ctx, buf.ctypes.data_as(C.c_void_p), buf.size) == K.ERR_STATE
        assert lib.dddmr_rollout_stack_get_lethal_nodes(ctx, None, 0, C.byref(n)) == K.ERR_STATE
        assert lib.dddmr_rollout_stack_set_host_layer(ctx, 0, buf.ctypes.data_as(C.c_void_p)) == K.ERR_STATE
        assert lib.dddmr_rollout_stack_reset(ctx) == K.ERR_STATE
        # a device layer that is asked for must exist, with the stack's n_ground
        refused(K.ERR_STATE, lambda: PerceptionStack(lp, marking_layer=type("L", (), {"n_ground": len(ground)})()))
        refused(K.ERR_STATE, lambda: PerceptionStack(lp, depth_layer=type("L", (), {"n_ground": len(ground)})()))
        rig = Rig(lp)
        refused(K.ERR_BAD_ARG, lambda: PerceptionStack(lp, rig.ml, rig.dl, n_ground=len(ground) - 1))
        refused(K.ERR_BAD_ARG, lambda: PerceptionStack(lp, rig.ml, rig.dl, order=(K.STACK_LIDAR, K.STACK_LIDAR)))
        refused(K.ERR_BAD_ARG, lambda: PerceptionStack(lp, rig.ml, rig.dl, host_layers=[None] * 5))
        refused(K.ERR_BAD_ARG, rig.stack.set_host_layer, 1, buf)
        # ... and the refused creates left the earlier stack in place
        rig.feed(u0)

        def one_good_update(u, what):
            lidar_obs, depth_obs = rig.observations()
            st = rig.stack.update(mc.TBS_LIDAR, u["t_gb"])
            so = rig.mo.update(lidar_obs, mc.TBS_LIDAR, u["t_gb"])
            res = rig.dref.update([rig.frs[s] for s in sorted(rig.frs)], depth_obs, u["t_gb"])
            rig.assert_lidar(st.lidar, so, what)
            T.assert_state(rig.dl, st.depth, rig.dref, res, what)
            rig.assert_stack(what)

        one_good_update(u0, "after the refused creates")
        # between tick_begin and tick_end
        lp.setPlan(sc2.plan)
        lp.tick_begin(sc2.theory.name.decode(), sc2.tick)
        refused(K.ERR_STATE, rig.stack.update, mc.TBS_LIDAR, u0["t_gb"])
        lp.tick_end()
        assert_full(rig.stack, rig.tr, "after the refused update")
        # after set_cloud the aggregate is not the sources': the lidar layer fails, the depth layer and the stack go on
        u1 = b["ups"][1]
        rig.feed(u1)
        _, depth_obs = rig.observations()
        lp.set_cloud(np.zeros((10, 4), np.float32))
        refused(K.ERR_STATE, rig.stack.update, mc.TBS_LIDAR, u1["t_gb"])
        st = rig.stack.last
        assert st.lidar_rc == K.ERR_STATE and st.depth_rc == K.OK and st.depth_skipped == 0
        res = rig.dref.update([rig.frs[s] for s in sorted(rig.frs)], depth_obs, u1["t_gb"])
        T.assert_state(rig.dl, st.depth, rig.dref, res, "depth layer beside a refused lidar pass")
        rig.assert_stack("stacked arrays after a refused lidar pass")
        # the next feed makes the aggregate the sources' again
        u2 = b["ups"][2]
        rig.feed(u2)
        one_good_update(u2, "after set_cloud and a new feed")
        # a later marking_create drops the stack
        rig.ml = marking.MarkingLayer(lp, sc.marking_config(), ground, NO_MAP)
        refused(K.ERR_STATE, rig.stack.update, mc.TBS_LIDAR, u2["t_gb"])
        refused(K.ERR_STATE, rig.stack.min_dgraph)
        refused(K.ERR_STATE, rig.stack.reset)
        # ... and a new stack over the new layer works
        rig.mo = oracle.MarkingOracle(sc.marking_config(), ground, NO_MAP)
        rig.stack = PerceptionStack(lp, rig.ml, rig.dl, [rig.static], order=rig.order)
        rig.tr.publish(rig.layers(host_set=False))                   # (the slot was set after create: it shows in the next update)
        assert_full(rig.stack, rig.tr, "a new stack over layers that hold state")
        u3 = b["ups"][3]
        rig.feed(u3)
        one_good_update(u3, "a new stack after marking_create")
