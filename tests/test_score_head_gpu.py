"""The head of a k_score workgroup: pure pursuit filed by the rollout, phase A's batched loads, the walk's prefix.

PurePursuitModel's (distance, folded yaw) depends on a trajectory's last pose alone, so the rollout computes it
(pure_pursuit_last_pose(), csrc/rollout_kernels.hip.h) into a per-trajectory array and k_score's phase A loads it beside
the trajectory's header; phase A issues the row-run index copy as a bounded, unrolled batch of 16-byte loads with one
wait; a collision walk of one round reads the item prefix D2 left instead of scanning it again.  None of it may change
a bit, so every case here is compared
  * with the CPU oracle per trajectory, by tests/test_score_tail_gpu.py's rule: steps, samples and reject codes exact,
    |cost difference| <= 1e-4, the winner = the last exact minimum of the engine's own costs (nothing fragile: asserted);
  * bit for bit across the knob pairs that are legal for it: DDDMR_HEADING_ROWS 0 / 1 (both rollout routes),
    DDDMR_FINAL 0 / 1 (k_finalize and phase E read the array), DDDMR_THREADS 256 / 512, DDDMR_NO_TAB 0 / 1,
    DDDMR_PROBE 0 / 1.
Every per-trajectory output and the new array are poisoned before each tick (DDDMR_POISON): a value the rollout did not
rewrite would come out as NaN.  Shapes are C1-sized: at most 64 trajectories, clouds of a few thousand points."""
import contextlib
import functools
import math
import os
import re

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, scenes, sharding
from dddmr_navigation_amd.local_planner import LocalPlanner
import oracle

pytestmark = pytest.mark.gpu
os.environ["DDDMR_POISON"] = "1"
TOL = 1e-4


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


def snapshot(lp, res):
    costs, steps, smp = (a.copy() for a in lp.debug())
    return dict(index=res.best_index, cost=res.best_cost, cmd=(res.vx, res.vy, res.wz), key=res.key, state=res.planner_state,
                costs=costs, steps=steps, samples=smp, best_poses=lp.best_poses().copy())


def run(theory, cloud, plan, tick, env=None, ticks=1, **kw):
    """`ticks` ticks of one scene in a context created under `env` -> a snapshot per tick"""
    with forced(env or {}):
        lp = LocalPlanner([theory], max_points=max(len(cloud), 16), max_plan_poses=max(len(plan), 16), **kw)
    try:
        lp.set_cloud(cloud)
        lp.setPlan(plan)
        return [snapshot(lp, lp.tick(theory.name.decode(), tick)) for _ in range(ticks)]
    finally:
        lp.close()


def assert_same(a, b, what=""):
    assert (b["index"], b["cost"], b["key"], b["state"]) == (a["index"], a["cost"], a["key"], a["state"]), what
    assert tuple(b["cmd"]) == tuple(a["cmd"]), what
    for name in ("costs", "steps", "samples", "best_poses"):
        assert a[name].shape == b[name].shape, f"{what} {name}"
        np.testing.assert_array_equal(b[name].view(np.uint8), a[name].view(np.uint8), err_msg=f"{what} {name}")   # bit for bit


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
        assert len(got["best_poses"]) == got["steps"][la]


def omni_grid(name, nx, ny, nth, steps, **kw):
    """An omni theory whose window is the grid [-1, 1]^2 x [-0.6, 0.6] for twist (0.5, 0, 0), like configs.bench_theory()"""
    base = dict(controller_frequency=10.0, sim_time=2.0, sim_granularity=0.05, angular_sim_granularity=0.025,
                bench_fixed_steps=steps, bench_no_zero_insert=1, max_vel_theta=0.6, min_vel_theta=0.0, acc_lim_theta=100.0,
                min_vel_x=-1.0, max_vel_x=1.0, min_vel_y=-1.0, max_vel_y=1.0, min_vel_trans=0.0, max_vel_trans=2.0,
                acc_lim_x=100.0, acc_lim_y=100.0, deceleration_ratio=1.0,
                linear_x_sample=float(nx), linear_y_sample=float(ny), angular_z_sample=float(nth))
    base.update(kw)
    return configs.theory(name, K.THEORY_OMNI_SIMPLE, configs.shipped_dd_critics(), **base)


def c1_theory(name, **kw):
    """The C1 theory (DD, 8 x 1 x 8, 20 steps) with some fields replaced"""
    th = configs.bench_theory("C1")
    th.name = name.encode()
    for k, v in kw.items():
        assert hasattr(th, k), k
        setattr(th, k, v)
    return th


def lattice(x0, x1, y0, y1, z0, z1, step):
    ax = [np.arange(a, b + 1e-9, step) for a, b in ((x0, x1), (y0, y1), (z0, z1))]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    # off the lattice by a fixed irrational pattern, so that no point sits on a cuboid face
    g = g + 0.013 * np.stack([np.sin(7.0 * g[:, 1] + 3.0 * g[:, 2]), np.sin(5.0 * g[:, 0] + 1.0), np.zeros(len(g))], axis=-1)
    return np.concatenate([g, np.zeros((len(g), 1))], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (theory, cloud, plan, tick, oracle tick), computed once and shared"""
    c1 = scenes.bench_scene("C1")
    th, cloud, plan, tick = c1.theory, c1.cloud, c1.plan, c1.tick
    if name == "c1":
        pass
    elif name == "omni_3x11":         # three x samples (a window of 3 x 2 x 2) of eleven steps: the omni increments' quarter-ahead pair
        th = omni_grid("omni_3x11", 3, 1, 1, 11, sim_time=1.0)
    elif name == "rotate":            # the shipped rotate-in-place list: two samples +-w of 126 steps, a dt each; under the
        th = configs.rotate_inplace_shipped("rot", critics=configs.shipped_dd_critics())   # DD stack, so pure pursuit counts
    elif name == "playground":        # the reference's own step rule: a step count and a dt per trajectory
        pg = scenes.playground_scene()
        th, cloud, plan, tick = pg.theory, pg.cloud, pg.plan, pg.tick
    elif name == "omni_gated":        # |v| = 1.41 > max_vel_trans at the window's corners: steps 0, never generated
        th = omni_grid("omni_gated", 4, 4, 4, 10, max_vel_trans=1.2, sim_time=1.0)
    elif name == "c1_one_step":       # steps < 2: the critic's -4
        th = c1_theory("one_step", bench_fixed_steps=1)
    elif name == "c1_no_plan":        # m == 0: the critic's -4, nothing of the plan pose is read
        plan = np.zeros((0, 7))
    elif name == "c1_pitched":        # C3P's pose: the robot on a 10 degree ramp
        tick = scenes.tick_input(pose=(0.0, 0.0, 0.0) + tuple(scenes.quat_from_rpy(0.0, math.radians(10.0), 0.0)))
    elif name in ("c1_far_3s", "c1_far_6s"):   # C1's 64 x 20 with a horizon of 3 s / 6 s on a 15 / 10 degree ramp: a wider, oblong tile
        far = name == "c1_far_6s"
        th = c1_theory(name, sim_time=6.0 if far else 3.0)
        tick = scenes.tick_input(pose=(0.0, 0.0, 0.0) + tuple(scenes.quat_from_rpy(0.0, math.radians(10.0 if far else 15.0), 0.0)))
    elif name == "wall":              # a dense wall in front of the robot: more collision items than a workgroup has lanes
        th = omni_grid("wall", 4, 3, 3, 40)
        cloud = lattice(0.5, 0.9, -1.2, 1.2, 0.05, 0.55, 0.03)
    elif name == "slab":              # under every pose, below the cuboid: items for every pair and nobody collides
        th = omni_grid("slab", 4, 3, 3, 40)
        cloud = lattice(-2.6, 2.6, -2.6, 2.6, -0.25, -0.25, 0.08)
    elif name == "far":               # beyond the local grid: no item at all
        th = omni_grid("far", 4, 3, 3, 40)
        cloud = lattice(40.0, 40.2, 40.0, 40.1, 0.3, 0.3, 0.1)
    elif name == "slab_short":        # a 4-step horizon: 16 trajectories fit one workgroup
        th = omni_grid("slab_short", 4, 3, 3, 4, sim_time=0.4)
        cloud = lattice(-2.6, 2.6, -2.6, 2.6, -0.25, -0.25, 0.08)
    else:
        raise KeyError(name)
    return th, cloud, plan, tick, oracle.tick(th, cloud, plan, tick, n_threads=8, want_margin=True)


# ---- pure pursuit through every rollout route ----

KNOB_PAIRS = [{"DDDMR_HEADING_ROWS": "0"}, {"DDDMR_FINAL": "1"}, {"DDDMR_FINAL": "0"}, {"DDDMR_THREADS": "256"},
              {"DDDMR_THREADS": "512"}, {"DDDMR_THREADS": "512", "DDDMR_FINAL": "1", "DDDMR_HEADING_ROWS": "0"}]


def check_routes(name, expect=None, **kw):
    th, cloud, plan, tick, o = scene(name)
    if expect:
        expect(o)
    base = run(th, cloud, plan, tick, **kw)[0]
    begin = kw and sharding.shard_range(kw["rank"], kw["world_size"], len(o.costs))[0] or 0
    assert_oracle(base, o, begin)
    for env in KNOB_PAIRS:
        assert_same(base, run(th, cloud, plan, tick, env, **kw)[0], f"{name} {env}")
    return base, o


def test_c1():
    _, o = check_routes("c1")
    assert len(o.costs) == 64 and (o.steps == 20).all() and (o.costs >= 0).any()


def test_omni_three_by_eleven():
    _, o = check_routes("omni_3x11")
    assert len(o.costs) == 12 and (o.steps == 11).all() and len(np.unique(o.samples[:, 0])) == 3


def test_shipped_rotate_in_place_list():
    _, o = check_routes("rotate")
    assert len(o.costs) == 2 and (o.steps == 126).all()


def test_playground_under_the_reference_step_rule():
    _, o = check_routes("playground")
    assert len(o.costs) == 55 and len(np.unique(o.steps[o.steps > 0])) > 3     # a step count (and a dt) per trajectory


def test_window_with_samples_that_are_not_generated():
    _, o = check_routes("omni_gated")
    assert set(np.unique(o.steps)) == {0, 10} and (o.steps == 0).sum() == 16


def test_one_step_horizon_is_the_critics_guard():
    got, o = check_routes("c1_one_step")
    assert (o.steps == 1).all() and set(np.unique(o.costs)) <= {-1.0, -4.0} and (got["costs"] == -4.0).any()


def test_no_plan():
    got, o = check_routes("c1_no_plan")
    assert (got["costs"] < 0).all() and (got["costs"] == -4.0).any()


def test_pitched_pose():
    check_routes("c1_pitched")


@pytest.mark.parametrize("rank", [1, 2])
def test_shards_that_begin_inside_the_window(rank):
    th, cloud, plan, tick, o = scene("c1")
    b, e = sharding.shard_range(rank, 3, 64)
    assert b > 0
    got, _ = check_routes("c1", rank=rank, world_size=3)
    assert len(got["costs"]) == e - b


def test_poisoned_array_is_rewritten_on_every_tick():
    """three ticks with load feedback (ticks 2 and 3 deal the tiles by the loads of the tick before); the array and every
    per-trajectory output are filled with 0xFF before each, a third of the window is never generated"""
    th, cloud, plan, tick, o = scene("omni_gated")
    for env in ({"DDDMR_TILE": "4"}, {"DDDMR_TILE": "4", "DDDMR_FINAL": "1"}, {"DDDMR_TILE": "4", "DDDMR_HEADING_ROWS": "0"}):
        outs = run(th, cloud, plan, tick, env, ticks=3)
        for got in outs:
            assert_oracle(got, o)
        for got in outs[1:]:
            assert_same(outs[0], got, f"a later tick against the first {env}")


# ---- phase A's index copy ----

# (scene, DDDMR_CELL) -> (gnx + 1) * gny entries of the row-run index (the context prints its grid under DDDMR_DEBUG_GRID;
# the test asserts the size it meant to hit).  The grid of a level robot is square, n x n cells with n <= 26 on C1 (the
# cell has a floor of a sixth of the cuboid's diameter), and n (n + 1) is a multiple of 512 for no n below 511: the
# sizes 1024 and 4096 need gnx = gny - 1, which a pitched robot (its tile is shorter along x) and a longer horizon give.
INDEX_CASES = [
    pytest.param("c1", "0.26", 420, id="below-512"),
    pytest.param("c1", "0.24", 506, id="not-a-multiple-of-4"),
    pytest.param("c1", "0.2", 702, id="largest-of-the-C1-grid"),
    pytest.param("c1_far_3s", "0.23", 1024, id="multiple-of-512"),
    pytest.param("c1_far_6s", "0.2085", 4096, id="largest-that-fits"),
    pytest.param("c1_far_6s", "0.2065", 0, id="does-not-fit"),
]


def grid_line(capfd):
    m = re.search(r"\[dddmr\] grid: (\d+) x (\d+) x (\d+) cells, row-run index of (\d+) entries", capfd.readouterr().err)
    assert m, "the context did not print its grid"
    gnx, gny, _, entries = (int(v) for v in m.groups())
    return gnx, gny, entries


@pytest.mark.parametrize("threads", ["256", "512"])
@pytest.mark.parametrize("name,cell,entries", INDEX_CASES)
def test_index_copy(name, cell, entries, threads, capfd):
    th, cloud, plan, tick, o = scene(name)
    env = {"DDDMR_CELL": cell, "DDDMR_THREADS": threads, "DDDMR_DEBUG_GRID": "1"}
    capfd.readouterr()
    got = run(th, cloud, plan, tick, env)[0]
    gnx, gny, staged = grid_line(capfd)
    assert staged == entries and (entries == 0) == ((gnx + 1) * gny > 4096), (gnx, gny, staged)
    assert_oracle(got, o)
    off = run(th, cloud, plan, tick, {**env, "DDDMR_NO_TAB": "1"})[0]
    assert grid_line(capfd)[2] == 0
    assert_same(got, off, f"cell {cell}, {threads} lanes, against DDDMR_NO_TAB=1")


# ---- the walk's prefix ----

def probe_pair(name, env, ticks=1):
    """DDDMR_PROBE 0 / 1 (one round: the prefix D2 left; two rounds: the scan per round) bit-equal, and the oracle"""
    th, cloud, plan, tick, o = scene(name)
    a = run(th, cloud, plan, tick, {**env, "DDDMR_PROBE": "0"}, ticks)
    b = run(th, cloud, plan, tick, {**env, "DDDMR_PROBE": "1"}, ticks)
    for i, (x, y) in enumerate(zip(a, b)):
        assert_oracle(x, o)
        assert_same(x, y, f"{name} {env} tick {i + 1}")
    return o


@pytest.mark.parametrize("threads", ["256", "512"])
def test_walk_with_more_items_than_lanes(threads):
    o = probe_pair("wall", {"DDDMR_TILE": "6", "DDDMR_THREADS": threads})
    assert (o.costs == -1.0).any() and (o.costs >= 0).any()
    probe_pair("slab", {"DDDMR_TILE": "6", "DDDMR_THREADS": threads}, ticks=2)


def test_walk_without_an_item():
    o = probe_pair("far", {"DDDMR_TILE": "6", "DDDMR_THREADS": "512"})
    assert not (o.costs == -1.0).any()


def test_one_trajectory_and_sixteen_per_workgroup():
    probe_pair("slab", {"DDDMR_TILE": "1", "DDDMR_THREADS": "512"})
    o = probe_pair("slab_short", {"DDDMR_TILE": "16", "DDDMR_THREADS": "512"})
    assert len(o.costs) == 36 and (o.steps == 4).all()          # 16 + 16 + 4: two full workgroups and a partly filled one


def test_partly_filled_last_workgroup():
    probe_pair("slab", {"DDDMR_TILE": "5", "DDDMR_THREADS": "512"})      # 36 = 7 * 5 + 1
    probe_pair("wall", {"DDDMR_TILE": "5", "DDDMR_THREADS": "256"})
