"""One row of headings per angular sample against a heading chain per trajectory, and both against the CPU oracle.

On a grid tick with a fixed step count the rollout workgroups take the shard in class-major order and evaluate the
theta chain and its sin / cos once per (angular sample, step) (csrc/rollout_kernels.hip.h, heading_rows_shared());
DDDMR_HEADING_ROWS=0 keeps a chain per trajectory.  The shared path performs the same floating-point operations on the
same inputs, so every case below builds both contexts and asserts
  * result, costs, steps, samples, best_poses and the pose arrays (the rollout's own state rows, every generated
    trajectory) bit-equal between them, and
  * against the oracle, by tests/test_score_tail_gpu.py's rule: reject codes exact, |cost difference| <= 1e-4, winner =
    the last exact minimum of the engine's own costs.  No trajectory is excluded: the oracle has no decision closer than
    1e-4 to its threshold in any of these scenes (asserted).
Every per-trajectory output is poisoned before each tick (DDDMR_POISON).  dddmr_rollout_heading_rows tells which path
the default context took, so a case that means to compare the two paths cannot pass by falling back, and a case that
must fall back (list mode, thin shard) is known to.  The shapes are the smallest that can still go wrong: workgroups that
straddle two classes (DDDMR_RT that does not divide the class size), a partly filled last workgroup, shards that begin
inside the angular axis, one class, one step, gated members inside a shared row."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, scenes, sharding
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
import oracle

pytestmark = pytest.mark.gpu
os.environ["DDDMR_POISON"] = "1"
TOL = 1e-4
OFF = {"DDDMR_HEADING_ROWS": "0"}


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
                costs=costs, steps=steps, samples=smp, best_poses=lp.best_poses().copy(), poses=lp.pose_arrays().copy(),
                shared=lp.heading_rows())


def run(theory, cloud, plan, tick, env, ticks=1, **kw):
    lp = planner(theory, cloud, plan, env, **kw)
    try:
        return [snapshot(lp, lp.tick(theory.name.decode(), tick)) for _ in range(ticks)]
    finally:
        lp.close()


def assert_same(a, b, what=""):
    assert (b["index"], b["cost"], b["key"], b["state"]) == (a["index"], a["cost"], a["key"], a["state"]), what
    assert tuple(b["cmd"]) == tuple(a["cmd"]), what
    for name in ("costs", "steps", "samples", "best_poses", "poses"):
        assert a[name].shape == b[name].shape, f"{what} {name}"
        np.testing.assert_array_equal(b[name].view(np.uint8), a[name].view(np.uint8), err_msg=f"{what} {name}")   # bit for bit


def both_paths(theory, cloud, plan, tick, env=None, ticks=1, shared=1, **kw):
    """default context and DDDMR_HEADING_ROWS=0, tick by tick bit-equal -> the default context's snapshots.
    `shared`: what the default context must report for every tick (the other one always reports 0)."""
    env = dict(env or {})
    base = run(theory, cloud, plan, tick, env, ticks, **kw)
    off = run(theory, cloud, plan, tick, {**env, **OFF}, ticks, **kw)
    for i, (a, b) in enumerate(zip(base, off)):
        assert (a["shared"], b["shared"]) == (shared, 0), f"tick {i + 1} {env}"
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
    assert len(got["poses"]) == int(got["steps"].sum())                # a pose per generated (trajectory, step)
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


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (theory, cloud, plan, tick, oracle tick), computed once and shared"""
    c1 = scenes.bench_scene("C1")
    th, cloud, plan, tick = c1.theory, c1.cloud, c1.plan, c1.tick
    if name == "c1":
        pass
    elif name == "c1_empty":
        cloud = np.zeros((0, 4), np.float32)
    elif name == "c1_pitched":        # C3P's pose: the robot on a 10 degree ramp
        tick = scenes.tick_input(pose=(0.0, 0.0, 0.0) + tuple(scenes.quat_from_rpy(0.0, math.radians(10.0), 0.0)))
    elif name == "c1_one_step":
        th = c1_theory("one_step", bench_fixed_steps=1)
    elif name == "c1_one_class":      # acc_lim_theta 0: the angular window is the robot's own rate, one sample
        th = c1_theory("one_class", acc_lim_theta=0.0)
        tick = scenes.tick_input(twist=(0.5, 0.0, 0.2))
    elif name == "c1_list":           # the motor constraint filters the grid into an explicit list
        th = c1_theory("listed", use_motor_constraint=1, max_motor_shaft_rpm=3000.0, wheel_diameter=0.16, gear_ratio=1.0,
                       robot_radius=0.25)
    elif name == "rotate":            # two samples +-w, dt = 6.28 / |w| / steps: always an explicit list
        th = configs.rotate_inplace_shipped("rot", bench_fixed_steps=20)
    elif name == "omni_small":        # quarter-ahead rows
        th = omni_grid("omni_small", 4, 2, 4, 5, sim_time=1.0)
    elif name == "omni_gated":        # |v| = 1.41 > max_vel_trans at the window's corners: steps 0 inside every class
        th = omni_grid("omni_gated", 4, 4, 4, 10, max_vel_trans=1.2, sim_time=1.0)
    else:
        raise KeyError(name)
    return th, cloud, plan, tick, oracle.tick(th, cloud, plan, tick, n_threads=8, want_margin=True)


@pytest.mark.parametrize("rt", ["4", "3", "5"])
def test_c1_grid(rt):
    """8 members per class: 4 per workgroup is the shape of the tick plan (two whole workgroups per class); 3 and 5 make
    workgroups straddle two classes and leave the last one partly filled (64 = 21 * 3 + 1 = 12 * 5 + 4)."""
    th, cloud, plan, tick, o = scene("c1")
    assert len(o.costs) == 64 and (o.steps == 20).all()
    got = both_paths(th, cloud, plan, tick, {"DDDMR_RT": rt})[0]
    assert_oracle(got, o)


def test_omni_grid_with_quarter_ahead_rows():
    th, cloud, plan, tick, o = scene("omni_small")
    assert len(o.costs) == 32 and (o.steps == 5).all()
    assert_oracle(both_paths(th, cloud, plan, tick, {"DDDMR_RT": "3"})[0], o)


def test_rotate_in_place_with_fixed_steps_keeps_its_chains():
    """Its window is an explicit list of two samples with a dt each: never shared, still equal."""
    th, cloud, plan, tick, o = scene("rotate")
    assert len(o.costs) == 2 and (o.steps == 20).all()
    assert_oracle(both_paths(th, cloud, plan, tick, shared=0)[0], o)


def test_one_angular_sample():
    th, cloud, plan, tick, o = scene("c1_one_class")
    assert len(o.costs) == 8 and len(np.unique(o.samples[:, 2])) == 1
    assert_oracle(both_paths(th, cloud, plan, tick, {"DDDMR_RT": "3"})[0], o)


def test_one_step():
    th, cloud, plan, tick, o = scene("c1_one_step")
    assert len(o.costs) == 64 and (o.steps == 1).all()
    assert_oracle(both_paths(th, cloud, plan, tick, {"DDDMR_RT": "3"})[0], o)


def test_gated_members_inside_a_shared_row():
    th, cloud, plan, tick, o = scene("omni_gated")
    gated = o.steps.reshape(4, 4, 4) == 0
    assert len(o.costs) == 64 and gated.sum() == 16 and (gated.sum(axis=(0, 1)) == 4).all()     # 4 of the 16 members of every class
    assert set(np.unique(o.steps)) == {0, 10}
    assert_oracle(both_paths(th, cloud, plan, tick, {"DDDMR_RT": "3"})[0], o)


def test_more_steps_than_the_context_holds():
    """The capacity error is the plan's, before any launch: both contexts report it alike."""
    th, cloud, plan, tick, _ = scene("c1")
    msgs = []
    for env in ({}, OFF):
        lp = planner(th, cloud, plan, env, max_steps=16)
        try:
            with pytest.raises(RolloutError) as e:
                lp.tick(th.name.decode(), tick)
            assert e.value.code == K.ERR_CAPACITY
            msgs.append(str(e.value))
            assert lp.heading_rows() == -1
        finally:
            lp.close()
    assert msgs[0] == msgs[1] and "20 steps > max_steps 16" in msgs[0]


@pytest.mark.parametrize("rank", [1, 2])
def test_shards_that_begin_inside_the_angular_axis(rank):
    """Ranks 1 and 2 of three: 21 or 22 trajectories from begin % 8 != 0 on, 2 or 3 members per class.  Two positions
    per workgroup share the rows (and straddle classes); four make the shard thin, which keeps a chain per trajectory."""
    th, cloud, plan, tick, o = scene("c1")
    b, e = sharding.shard_range(rank, 3, 64)
    assert b % 8 != 0 and (e - b) // 8 == 2
    for rt, shared in (("2", 1), ("4", 0)):
        got = both_paths(th, cloud, plan, tick, {"DDDMR_RT": rt}, shared=shared, rank=rank, world_size=3)[0]
        assert len(got["costs"]) == e - b
        assert_oracle(got, o, begin=b)


def test_a_listed_window_keeps_its_chains():
    th, cloud, plan, tick, o = scene("c1_list")
    assert len(o.costs) == 64
    assert_oracle(both_paths(th, cloud, plan, tick, shared=0)[0], o)


def test_empty_cloud_through_the_stand_alone_rollout():
    """No binning launch: k_bin_reset + the 256-lane k_rollout."""
    th, cloud, plan, tick, o = scene("c1_empty")
    assert_oracle(both_paths(th, cloud, plan, tick, {"DDDMR_RT": "3"})[0], o)


def test_three_consecutive_ticks_with_load_feedback():
    """Ticks 2 and 3 deal the k_score tiles by the loads of the tick before; the assignment workgroups ride in the same
    launch as the rollout's."""
    th, cloud, plan, tick, o = scene("omni_gated")
    outs = both_paths(th, cloud, plan, tick, {"DDDMR_RT": "3", "DDDMR_TILE": "4"}, ticks=3)
    for got in outs:
        assert_oracle(got, o)
    for got in outs[1:]:
        assert_same(outs[0], got, "a later tick against the first")


def test_pitched_pose_through_the_general_k_score():
    th, cloud, plan, tick, o = scene("c1_pitched")
    assert_oracle(both_paths(th, cloud, plan, tick, {"DDDMR_RT": "3"})[0], o)
