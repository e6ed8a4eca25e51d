"""The deals of the load-feedback assignment against each other and against the CPU oracle.

From a context's second tick of one shard on, k_bin_count's assignment block sorts the trajectories by the load the tick
before filed and deals them to k_score's workgroups (csrc/rollout_kernels.hip.h, deal_slot()): in snake order, every
workgroup equally heavy (mode 0; shards of one round of resident workgroups), sorted, workgroup b the b-th heaviest
(mode 1; shards of several rounds), or with the lightest in the workgroups of the last, partial round (mode 2, behind
the knob).  DDDMR_DEAL = 0 / 1 / 2 at create forces one wherever there is an assignment.  Any deal gives the same bits,
so every case runs four ticks (feedback starts at the second) in a context per mode and asserts
  * result, costs, steps, samples and best poses bit-equal between the modes on every tick,
  * against the oracle: steps and samples exact, reject codes exact and |cost difference| <= 1e-4 where the oracle's own
    verdict margin is at least that,
  * dddmr_rollout_deal names the expected path: 0 on the first tick (no assignment), the forced mode from then on,
  * the assignment read back is a permutation of [0, n_local),
  * in mode 1, with the load classes of assign_block recomputed here from the loads read back after the tick before, no
    class in workgroup b + G is heavier than the lightest class in workgroup b.
Shapes: the shipped 275-trajectory omni theory on the 5 000-point C1 cloud in tiles of 4 (69 workgroups of 4 and 3); a
17 x 16 x 16 grid of 20 steps in tiles of 6 (two assignment groups, n_local no multiple of G x tile); a 33 x 16 x 16 grid of
10 steps with the knob left alone (8 448 trajectories in 528 workgroups of 16: more than the 512 resident, so the
automatic choice is the sorted deal); and two theories in one context, where a tick after a changed shard falls back to the
strided deal.  Every per-trajectory output is poisoned before each tick (DDDMR_POISON)."""
import contextlib
import functools
import os

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, local_planner, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner
import oracle

pytestmark = pytest.mark.gpu
os.environ["DDDMR_POISON"] = "1"
TOL = 1e-4
TICKS = 4
LOAD_CLASSES = 1024          # kLoadClasses
ASSIGN_PER_GROUP = 4096      # kAssignPer * kBinThreads


@contextlib.contextmanager
def forced(env):
    """The knobs are read when a context is created: set, create, restore."""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def snapshot(lp, res):
    costs, steps, smp = (a.copy() for a in lp.debug())
    assign, load, assigned = local_planner.deal_arrays(lp)
    return dict(index=res.best_index, cost=res.best_cost, cmd=(res.vx, res.vy, res.wz), key=res.key, state=res.planner_state,
                costs=costs, steps=steps, samples=smp, best_poses=lp.best_poses().copy(), deal=local_planner.deal(lp),
                assign=assign.copy(), load=load.copy(), assigned=assigned)


def run(theories, names, cloud, plan, tick, env):
    """one tick per entry of `names` in a context created under `env` -> a snapshot per tick"""
    with forced(env):
        lp = LocalPlanner(theories, max_points=max(len(cloud), 16), max_plan_poses=max(len(plan), 16))
    try:
        assert local_planner.deal(lp) == -1
        lp.set_cloud(cloud)
        lp.setPlan(plan)
        return [snapshot(lp, lp.tick(n, tick)) for n in names]
    finally:
        lp.close()


def assert_same(a, b, what=""):
    assert (b["index"], b["cost"], b["key"], b["state"]) == (a["index"], a["cost"], a["key"], a["state"]), what
    assert tuple(b["cmd"]) == tuple(a["cmd"]), what
    for name in ("costs", "steps", "samples", "best_poses"):
        assert a[name].shape == b[name].shape, f"{what} {name}"
        np.testing.assert_array_equal(b[name].view(np.uint8), a[name].view(np.uint8), err_msg=f"{what} {name}")   # bit for bit


def assert_oracle(got, o):
    np.testing.assert_array_equal(got["steps"], o.steps)
    np.testing.assert_array_equal(got["samples"], o.samples)
    assert not np.isnan(got["costs"]).any()                            # nothing left poisoned
    firm = np.abs(o.min_margin) >= TOL                                 # the oracle's own verdict is not within TOL of flipping
    neg = ((got["costs"] < 0) | (o.costs < 0)) & firm
    np.testing.assert_array_equal(got["costs"][neg], o.costs[neg])     # reject codes bit-exact
    pos = (got["costs"] >= 0) & (o.costs >= 0)
    if pos.any():
        assert np.max(np.abs(got["costs"][pos] - o.costs[pos])) <= TOL


def load_classes(load, n, groups):
    """assign_block's class of every trajectory (0 = heaviest), or None for a group whose loads are all equal"""
    cls = np.zeros(n, np.int64)
    flat = []
    for grp in range(groups):
        v = load[grp::groups].astype(np.uint32)
        mx, mn = max(1, int(v.max())), int(v.min())
        if mx <= mn:
            flat.append(grp)
            continue
        scale = np.float32(LOAD_CLASSES - 1) / np.float32(mx)
        c = (v.astype(np.float32) * scale).astype(np.int64)
        cls[grp::groups] = LOAD_CLASSES - 1 - np.minimum(LOAD_CLASSES - 1, c)
    return cls, flat


def assert_sorted_deal(assign, load_before, tile):
    """workgroup b reads the slots b, b + n_tiles, ...: its classes against those of workgroup b + G"""
    n = len(assign)
    groups = max(1, (n + ASSIGN_PER_GROUP - 1) // ASSIGN_PER_GROUP)
    n_tiles = ((n + tile - 1) // tile + groups - 1) // groups * groups
    cls, flat = load_classes(load_before, n, groups)
    lo = np.full(n_tiles, -1, np.int64)      # heaviest (smallest) class of the workgroup
    hi = np.full(n_tiles, -1, np.int64)      # lightest
    sizes = np.zeros(n_tiles, np.int64)
    for b in range(n_tiles):
        slots = np.arange(b, n, n_tiles)[:tile]
        assert np.all(assign[slots] % groups == b % groups)             # a group deals its own trajectories to its own workgroups
        sizes[b] = len(slots)
        if len(slots):
            c = cls[assign[slots]]
            lo[b], hi[b] = c.min(), c.max()
    checked = 0
    for b in range(n_tiles - groups):
        if b % groups in flat or sizes[b] == 0 or sizes[b + groups] == 0:
            continue
        assert lo[b + groups] >= hi[b], f"workgroup {b + groups} holds class {lo[b + groups]}, workgroup {b} class {hi[b]}"
        checked += 1
    return checked, sizes


def check_modes(theory, cloud, plan, tick, o, env, tile, modes=("0", "1", "2")):
    name = theory.name.decode()
    outs = {m: run([theory], [name] * TICKS, cloud, plan, tick, {**env, "DDDMR_DEAL": m}) for m in modes}
    n = len(o.costs)
    for m, snaps in outs.items():
        assert [s["deal"] for s in snaps] == [0] + [int(m)] * (TICKS - 1), m
        assert [s["assigned"] for s in snaps] == [False] + [True] * (TICKS - 1), m
        for i, s in enumerate(snaps):
            assert_same(outs[modes[0]][i], s, f"DDDMR_DEAL={m} tick {i + 1}")
            assert_oracle(s, o)
            np.testing.assert_array_equal(np.sort(s["assign"]), np.arange(n, dtype=np.uint32))     # a permutation
    return outs


@functools.lru_cache(maxsize=None)
def c1_cloud():
    return scenes.bench_scene("C1").cloud


def grid_theory(name, nx, ny, nth, steps):
    return configs.theory(name, K.THEORY_OMNI_SIMPLE, configs.shipped_dd_critics(),
                          controller_frequency=10.0, sim_time=2.0, sim_granularity=0.05, angular_sim_granularity=0.025,
                          bench_fixed_steps=steps, bench_no_zero_insert=1, max_vel_theta=0.6, min_vel_theta=0.0, acc_lim_theta=100.0,
                          min_vel_x=-1.0, max_vel_x=1.0, min_vel_y=-1.0, max_vel_y=1.0, min_vel_trans=0.0, max_vel_trans=2.0,
                          acc_lim_x=100.0, acc_lim_y=100.0, deceleration_ratio=1.0,
                          linear_x_sample=float(nx), linear_y_sample=float(ny), angular_z_sample=float(nth))


@functools.lru_cache(maxsize=None)
def scene(kind):
    """-> (theory, cloud, plan, tick, oracle tick), computed once and shared"""
    if kind == "omni275":
        th = configs.omni_simple_shipped()
    elif kind == "grid4352":
        th = grid_theory("deal_4352", 17, 16, 16, 20)
    elif kind == "grid8448":
        th = grid_theory("deal_8448", 33, 16, 16, 10)
    else:
        raise KeyError(kind)
    plan = scenes.s_curve_plan(80)
    tick = scenes.tick_input()
    o = oracle.tick(th, c1_cloud(), plan, tick, n_threads=8, want_margin=True)
    return th, c1_cloud(), plan, tick, o


def test_shipped_omni_theory_in_tiles_of_four():
    th, cloud, plan, tick, o = scene("omni275")
    assert len(o.costs) == 275
    outs = check_modes(th, cloud, plan, tick, o, {"DDDMR_TILE": "4", "DDDMR_THREADS": "512"}, 4)
    for i in range(1, TICKS):
        checked, sizes = assert_sorted_deal(outs["1"][i]["assign"], outs["1"][i - 1]["load"], 4)
        assert len(sizes) == 69 and sorted(set(sizes.tolist())) == [3, 4] and checked >= 60
        assert list(sizes) == [4] * 68 + [3]                 # 275 - 3 * 69 = 68 workgroups of 4, then one of 3


def test_two_assignment_groups_and_a_ragged_last_round():
    th, cloud, plan, tick, o = scene("grid4352")
    n = len(o.costs)
    assert n == 4352 and n > ASSIGN_PER_GROUP and n % (2 * 6) != 0
    outs = check_modes(th, cloud, plan, tick, o, {"DDDMR_TILE": "6", "DDDMR_THREADS": "512"}, 6)
    for i in range(1, TICKS):
        checked, sizes = assert_sorted_deal(outs["1"][i]["assign"], outs["1"][i - 1]["load"], 6)
        assert len(sizes) == 726 and sorted(set(sizes.tolist())) == [5, 6] and checked >= 700


def test_the_automatic_choice_on_a_shard_of_more_than_one_round():
    """528 workgroups of 16 on 512 resident slots: sorted without the knob; DDDMR_DEAL=0 is the snake it is compared with"""
    th, cloud, plan, tick, o = scene("grid8448")
    n = len(o.costs)
    assert n == 8448
    name = th.name.decode()
    auto = run([th], [name] * TICKS, cloud, plan, tick, {})
    snake = run([th], [name] * TICKS, cloud, plan, tick, {"DDDMR_DEAL": "0"})
    assert [s["deal"] for s in auto] == [0] + [1] * (TICKS - 1)
    assert [s["deal"] for s in snake] == [0] * TICKS
    for i, (a, b) in enumerate(zip(auto, snake)):
        assert_same(b, a, f"tick {i + 1}")
        assert_oracle(a, o)
        np.testing.assert_array_equal(np.sort(a["assign"]), np.arange(n, dtype=np.uint32))
        np.testing.assert_array_equal(np.sort(b["assign"]), np.arange(n, dtype=np.uint32))
    for i in range(1, TICKS):
        checked, sizes = assert_sorted_deal(auto[i]["assign"], auto[i - 1]["load"], 16)
        assert len(sizes) == 528 and int(sizes.sum()) == n and checked >= 500
    # a sorted tick files the candidate item counts: the same loads whoever shared the tile, tick after tick
    np.testing.assert_array_equal(auto[2]["load"], auto[3]["load"])


def test_a_tick_after_a_changed_shard_deals_strided():
    th_a, cloud, plan, tick, _ = scene("omni275")
    th_b = configs.dd_simple_shipped()
    names = [th_a.name.decode(), th_a.name.decode(), th_b.name.decode(), th_b.name.decode(), th_a.name.decode()]
    outs = {m: run([th_a, th_b], names, cloud, plan, tick, {"DDDMR_TILE": "4", "DDDMR_THREADS": "512", "DDDMR_DEAL": m}) for m in ("0", "1")}
    for m, snaps in outs.items():
        assert [s["assigned"] for s in snaps] == [False, True, False, True, False], m
        assert [s["deal"] for s in snaps] == [0, int(m), 0, int(m), 0], m
        for i, s in enumerate(snaps):
            assert_same(outs["0"][i], s, f"DDDMR_DEAL={m} tick {i + 1}")
            if not s["assigned"]:
                np.testing.assert_array_equal(s["assign"], np.arange(len(s["assign"]), dtype=np.uint32))
    assert len(outs["1"][2]["costs"]) != len(outs["1"][1]["costs"])        # the shard did change
