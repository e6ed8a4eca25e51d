"""The two tails of the scoring launch against each other and against the CPU oracle.

A single-round shard scores its critic stacks in k_score and reduces the workgroups' slots in the last workgroup; a
multi-round shard (DevTick::final_kernel, forced here with DDDMR_FINAL=1) leaves a 32-byte record per trajectory and
k_finalize scores the whole shard one lane per trajectory, 256 to a workgroup, and takes the exact argmin.  Both call
the same score_stack(); every case below runs both and asserts
  * costs, steps, samples, winner, cost, command and key bit-equal between the two paths, and
  * against the oracle: reject codes bit-exact, |cost difference| <= 1e-4, winner = the last exact minimum of the
    engine's own costs (local_planner.cpp:452-463).  No trajectory is excluded: the oracle has no decision closer
    than 1e-4 to its threshold in any of these scenes (asserted).
Every per-trajectory output is poisoned before each tick (DDDMR_POISON), so a trajectory that got no record or no
score cannot pass for scored.  The scenes are small: one partly filled k_finalize workgroup, two workgroups with the
winner in the second, equal costs across the workgroup boundary, no winner at all."""
import contextlib
import functools
import os

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, scenes, sharding
from dddmr_navigation_amd.local_planner import LocalPlanner
import oracle

pytestmark = pytest.mark.gpu
os.environ["DDDMR_POISON"] = "1"
TOL = 1e-4
FINAL = {"DDDMR_FINAL": "1"}


def last_argmin(costs):
    """The reference's scan (local_planner.cpp:452-463) over an array of costs."""
    best, m = -1, 9999999.0
    for i, c in enumerate(costs):
        if c >= 0 and c <= m:
            best, m = i, c
    return best


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


def planner(theory, cloud, plan, env, **kw):
    with forced(env):
        lp = LocalPlanner([theory], max_points=max(len(cloud), 16), **kw)
    lp.set_cloud(cloud)
    lp.setPlan(plan)
    return lp


def snapshot(lp, res):
    costs, steps, smp = (a.copy() for a in lp.debug())
    return dict(index=res.best_index, cost=res.best_cost, cmd=(res.vx, res.vy, res.wz), key=res.key, state=res.planner_state,
                costs=costs, steps=steps, samples=smp)


def run(theory, cloud, plan, tick, env, ticks=1, **kw):
    lp = planner(theory, cloud, plan, env, **kw)
    try:
        return [snapshot(lp, lp.tick(theory.name.decode(), tick)) for _ in range(ticks)]
    finally:
        lp.close()


def assert_same(a, b, what=""):
    assert (b["index"], b["cost"], b["key"], b["state"]) == (a["index"], a["cost"], a["key"], a["state"]), what
    assert tuple(b["cmd"]) == tuple(a["cmd"]), what
    for name in ("costs", "steps", "samples"):
        np.testing.assert_array_equal(b[name].view(np.uint8), a[name].view(np.uint8), err_msg=f"{what} {name}")   # bit for bit


def both_paths(theory, cloud, plan, tick, env=None, ticks=1, **kw):
    """default path and k_finalize path, tick by tick bit-equal -> the default path's snapshots"""
    env = dict(env or {})
    base = run(theory, cloud, plan, tick, env, ticks, **kw)
    fin = run(theory, cloud, plan, tick, {**env, **FINAL}, ticks, **kw)
    for i, (a, b) in enumerate(zip(base, fin)):
        assert_same(a, b, f"tick {i + 1} {env}")
    return base


def assert_oracle(got, o, begin=0):
    n = len(got["costs"])
    oc = o.costs[begin:begin + n]
    assert int((np.abs(o.min_margin) < TOL).sum()) == 0                # nothing fragile: nobody is excluded below
    np.testing.assert_array_equal(got["steps"], o.steps[begin:begin + n])
    np.testing.assert_array_equal(got["samples"], o.samples[begin:begin + n])
    assert not np.isnan(got["costs"]).any()                            # nothing left poisoned
    neg = (got["costs"] < 0) | (oc < 0)
    np.testing.assert_array_equal(got["costs"][neg], oc[neg])          # reject codes bit-exact: -1 / -4 / -100
    if (~neg).any():
        assert np.max(np.abs(got["costs"][~neg] - oc[~neg])) <= TOL
    la = last_argmin(got["costs"])
    assert got["index"] == (begin + la if la >= 0 else -1)
    if la >= 0:
        assert got["cost"] == got["costs"][la] and got["key"] == sharding.pack_key(got["costs"][la], begin + la)
        assert got["cmd"] == tuple(float(v) for v in got["samples"][la])


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (theory, cloud, plan, tick, oracle tick), computed once and shared"""
    c1 = scenes.bench_scene("C1")
    if name == "playground_c1":
        pg = scenes.playground_scene()
        th, cloud, plan, tick = pg.theory, c1.cloud, pg.plan, pg.tick
    elif name in ("omni_c1", "omni_c1_collision_only", "omni_blocked"):
        th = configs.omni_simple_shipped()
        cloud, plan, tick = c1.cloud, c1.plan, scenes.tick_input(twist=(0.3, 0.0, 0.0))
        if name == "omni_c1_collision_only":
            assert th.critics[0].kind == K.CRITIC_COLLISION
            th.n_critics = 1
        if name == "omni_blocked":          # a dense blob at the robot: every cuboid of every trajectory holds points
            rng = np.random.default_rng(19)
            cloud = np.concatenate([rng.uniform(-0.6, 0.6, (4000, 2)), rng.uniform(0.05, 0.6, (4000, 1)), np.zeros((4000, 1))],
                                   axis=1).astype(np.float32)
    elif name == "omni_corridor":
        c2 = scenes.bench_scene("C2", "r01")
        th = configs.omni_simple_shipped(linear_x_sample=6.0, linear_y_sample=6.0, angular_z_sample=8.0, sim_time=4.0)
        cloud, plan, tick = c2.cloud, c2.plan, scenes.tick_input(twist=(0.4, 0.3, 0.0))
    elif name == "near_tie":
        # cost = {1.0 | 2.0} + |w| * 1e-10: hundreds of costs share a packed key's 40 cost bits but differ as doubles
        th = configs.dd_simple_shipped(name="near", linear_x_sample=8.0, angular_z_sample=33.0, acc_lim_theta=100.0,
                                       critics=[configs.critic(K.CRITIC_SHORTEST_ANGLE, weight=1.0),
                                                configs.critic(K.CRITIC_TWIRLING, weight=1e-10)])
        cloud, plan = np.zeros((0, 4), np.float32), scenes.s_curve_plan()
        tick = scenes.tick_input(twist=(0.4, 0.0, 0.0), heading_deviation=0.5)
    else:
        raise KeyError(name)
    return th, cloud, plan, tick, oracle.tick(th, cloud, plan, tick, n_threads=8, want_margin=True)


@pytest.mark.parametrize("env", [{}, {"DDDMR_TILE": "3"}, {"DDDMR_THREADS": "256"}], ids=["default", "tile3", "threads256"])
def test_one_partly_filled_workgroup(env):
    th, cloud, plan, tick, o = scene("playground_c1")
    assert (len(o.costs), int((o.costs == -1.0).sum()), o.result.best_index) == (55, 23, 19)
    got = both_paths(th, cloud, plan, tick, env)[0]
    assert_oracle(got, o)
    assert got["index"] == 19


def test_two_workgroups_winner_in_the_second():
    th, cloud, plan, tick, o = scene("omni_c1")
    assert (len(o.costs), o.result.best_index) == (275, 258)
    got = both_paths(th, cloud, plan, tick)[0]
    assert_oracle(got, o)
    assert got["index"] == 258


def test_equal_costs_the_last_free_index_wins_across_the_workgroup_boundary():
    th, cloud, plan, tick, o = scene("omni_c1_collision_only")
    free = np.flatnonzero(o.costs == 0.0)
    assert len(o.costs) == 275 and set(np.unique(o.costs)) == {-1.0, 0.0} and free[-1] >= 256 and (free < 256).any()
    got = both_paths(th, cloud, plan, tick)[0]
    assert_oracle(got, o)
    assert (got["index"], got["cost"]) == (int(free[-1]), 0.0)


@pytest.mark.parametrize("world", [2, 3])
def test_equal_costs_across_ranks(world):
    th, cloud, plan, tick, o = scene("omni_c1_collision_only")
    name = th.name.decode()
    expect = last_argmin(o.costs)
    for env in ({}, FINAL):
        lps, words = [], []
        try:
            for r in range(world):
                lp = planner(th, cloud, plan, env, rank=r, world_size=world)
                lps.append(lp)
                got = snapshot(lp, lp.tick(name, tick))
                b, e = sharding.shard_range(r, world, len(o.costs))
                assert len(got["costs"]) == e - b
                assert_oracle(got, o, begin=b)
                words.append(lp.winner_words())
            for lp in lps:
                w = lp.resolve_words([v for pair in words for v in pair])
                assert (w.best_index, w.best_cost) == (expect, 0.0)
                assert (w.vx, w.vy, w.wz) == (o.result.vx, o.result.vy, o.result.wz)
            # the same through the device side of the exchange (slot vector -> k_resolve), rehearsed on one GPU
            for r, lp in enumerate(lps):
                lp.comm_loopback()
                for p in range(world):
                    if p != r:
                        lp.comm_loopback_set_peer(p, words[p])
                res = lp.tick(name, tick)
                assert (res.best_index, res.best_cost) == (expect, 0.0), (env, r)
                assert (res.vx, res.vy, res.wz) == (o.result.vx, o.result.vy, o.result.wz)
                lp.comm_destroy()
        finally:
            for lp in lps:
                lp.close()


def test_rotate_in_place_on_an_empty_cloud():
    """2 trajectories, no binning launch (k_bin_reset + k_rollout): equal costs -> index 1; above the cap -> nobody."""
    cloud, plan, tick = np.zeros((0, 4), np.float32), scenes.s_curve_plan(), scenes.tick_input()
    th = configs.rotate_inplace_shipped("r", critics=[configs.critic(K.CRITIC_TWIRLING)])
    got = both_paths(th, cloud, plan, tick)[0]
    assert list(got["costs"]) == [0.5, 0.5] and (got["index"], got["cost"], got["cmd"][2]) == (1, 0.5, -0.5)
    assert_oracle(got, oracle.tick(th, cloud, plan, tick, want_margin=True))
    th = configs.rotate_inplace_shipped("r", critics=[configs.critic(K.CRITIC_TWIRLING, weight=4e7)])
    got = both_paths(th, cloud, plan, tick)[0]
    assert list(got["costs"]) == [2e7, 2e7]
    assert (got["state"], got["index"], got["cost"], got["cmd"], got["key"]) == (K.ALL_TRAJECTORIES_FAIL, -1, -1.0, (0.0, 0.0, 0.0), K.KEY_NONE)


@pytest.mark.parametrize("world", [1, 2])
def test_near_ties_below_a_packed_keys_resolution(world):
    th, cloud, plan, tick, o = scene("near_tie")
    n = len(o.costs)
    assert n == 264 and o.result.best_index == last_argmin(o.costs) == 247
    keys = [sharding.pack_key(c, i) for i, c in enumerate(o.costs)]
    assert sharding.key_index(min(keys)) != o.result.best_index        # the packed key alone picks another index
    for env in ({}, FINAL):
        lps, words = [], []
        try:
            for r in range(world):
                lp = planner(th, cloud, plan, env, rank=r, world_size=world)
                lps.append(lp)
                got = snapshot(lp, lp.tick("near", tick))
                b, e = sharding.shard_range(r, world, n)
                np.testing.assert_array_equal(got["costs"], o.costs[b:e])      # no libm in these critics: bit-equal
                assert_oracle(got, o, begin=b)
                words += list(lp.winner_words())
            for lp in lps:
                w = lp.resolve_words(words)
                assert (w.best_index, w.best_cost) == (o.result.best_index, o.result.best_cost), env
                assert (w.vx, w.wz) == (o.result.vx, o.result.wz)
        finally:
            for lp in lps:
                lp.close()


def test_corridor_where_most_trajectories_collide():
    th, cloud, plan, tick, o = scene("omni_corridor")
    assert (len(o.costs), int((o.costs == -1.0).sum())) == (324, 289)
    assert_oracle(both_paths(th, cloud, plan, tick)[0], o)


def test_a_cloud_that_blocks_every_trajectory():
    th, cloud, plan, tick, o = scene("omni_blocked")
    assert len(o.costs) == 275 and (o.costs == -1.0).all() and o.result.best_index == -1
    got = both_paths(th, cloud, plan, tick)[0]
    assert_oracle(got, o)
    assert (got["costs"] == -1.0).all()
    assert (got["state"], got["index"], got["cost"], got["key"]) == (K.ALL_TRAJECTORIES_FAIL, -1, -1.0, K.KEY_NONE)


def test_three_consecutive_ticks_on_one_context():
    """Tick 1 runs without load feedback and with the probe on; ticks 2 and 3 deal the tiles by the loads k_finalize
    filed and take the probe decision from its collided count."""
    th, cloud, plan, tick, o = scene("omni_corridor")
    outs = both_paths(th, cloud, plan, tick, ticks=3)
    for got in outs:
        assert_oracle(got, o)
    for got in outs[1:]:
        assert_same(outs[0], got, "a later tick against the first")
