"""Prune-plan length and critic-stack size against the oracle, HIP path.

k_score's phase P walks the prune plan in two ways: with more than 256 surviving (trajectory, step) pairs in a
workgroup every lane walks the whole plan through the scalar unit, one chunk of poses requested ahead of the one being
worked on, over a device copy of the plan that is padded with copies of its last pose to whole loop trips; with fewer
pairs several lanes share a pose and read slices of the plan from LDS.  Phase E reads the critic stack's kinds and
weights as one batch of kernel-argument loads.  These tests pin
  (a) every remainder of the chunked walk, the constant-return rule for plans under 3 poses and the 512-pose cap,
  (b) that the padding is rewritten when a shorter plan follows a longer one on the same context,
  (c) that both 1-NN routes give the same bits,
  (d) stacks of 1 ... 8 critics.
The C2 scene (4096 x 50 against 100 k points) runs the scalar route with its default 512-lane workgroups.
"""
import os

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner
import oracle
from test_argmin_stack_gpu import STACKS, _critic

pytestmark = pytest.mark.gpu
TOL = 1e-4

PREFIXES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 79, 80]
INTERPOLATED = [81, 257, 511, 512]


@pytest.fixture(scope="module")
def c2():
    return scenes.bench_scene("C2")


def plan_of(sc, m):
    """m poses: a prefix of the scene's 80, or its positions resampled (orientation of the nearest pose; the first
    and the last pose are the scene's own)."""
    if m <= len(sc.plan):
        return np.ascontiguousarray(sc.plan[:m])
    t = np.linspace(0.0, len(sc.plan) - 1.0, m)
    out = np.ascontiguousarray(sc.plan[np.rint(t).astype(int)])
    for c in range(3):
        out[:, c] = np.interp(t, np.arange(len(sc.plan)), sc.plan[:, c])
    return out


def gpu_ticks(sc, plans, **kw):
    """One context, one tick per plan in turn -> [(result, costs, steps, samples)]"""
    out = []
    with LocalPlanner([sc.theory], max_points=len(sc.cloud), max_plan_poses=512, **kw) as lp:
        lp.set_cloud(sc.cloud)
        for plan in plans:
            lp.setPlan(plan)
            res = lp.tick(sc.theory.name.decode(), sc.tick)
            out.append((res,) + tuple(a.copy() for a in lp.debug()))
    return out


def check_against_oracle(got, o):
    res, costs, steps, smp = got
    np.testing.assert_array_equal(steps, o.steps)
    np.testing.assert_array_equal(smp, o.samples)
    neg = (costs < 0) | (o.costs < 0)
    np.testing.assert_array_equal(costs[neg], o.costs[neg])            # -1 / -4 / -100: identical
    both = ~neg
    if both.any():
        assert np.max(np.abs(costs[both] - o.costs[both])) <= TOL
    r = o.result
    assert res.planner_state == r.planner_state
    assert res.best_index == r.best_index
    assert abs(res.vx - r.vx) <= TOL and abs(res.vy - r.vy) <= TOL and abs(res.wz - r.wz) <= TOL
    assert abs(res.best_cost - r.best_cost) <= TOL


def same_bits(a, b):
    (ra, ca, sa, ma), (rb, cb, sb, mb) = a, b
    np.testing.assert_array_equal(ca.view(np.int64), cb.view(np.int64))
    np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(ma, mb)
    assert (ra.best_index, ra.best_cost, ra.vx, ra.vy, ra.wz, ra.key) == (rb.best_index, rb.best_cost, rb.vx, rb.vy, rb.wz, rb.key)


@pytest.mark.parametrize("m", PREFIXES + INTERPOLATED)
def test_plan_length_against_oracle(c2, m):
    plan = plan_of(c2, m)
    assert len(plan) == m
    got = gpu_ticks(c2, [plan])[0]
    o = oracle.tick(c2.theory, c2.cloud, plan, c2.tick, n_threads=8)
    assert (o.costs == -1.0).any()
    check_against_oracle(got, o)


def test_shorter_plan_after_a_longer_one_is_padded_afresh(c2):
    long_plan, short_plan = plan_of(c2, 33), plan_of(c2, 5)
    second = gpu_ticks(c2, [long_plan, short_plan])[1]
    fresh = gpu_ticks(c2, [short_plan])[0]
    same_bits(second, fresh)


@pytest.mark.parametrize("m", [3, 5, 33, 80, 257])
def test_both_nearest_pose_routes_agree(c2, m):
    plan = plan_of(c2, m)
    o = oracle.tick(c2.theory, c2.cloud, plan, c2.tick, n_threads=8)
    default = gpu_ticks(c2, [plan])[0]
    saved = os.environ.get("DDDMR_TILE")
    os.environ["DDDMR_TILE"] = "1"           # 50 pairs per workgroup: several lanes per pose, plan slices from LDS
    try:
        shared = gpu_ticks(c2, [plan])[0]
    finally:
        if saved is None:
            os.environ.pop("DDDMR_TILE", None)
        else:
            os.environ["DDDMR_TILE"] = saved
    check_against_oracle(default, o)
    check_against_oracle(shared, o)
    np.testing.assert_array_equal(default[1].view(np.int64), shared[1].view(np.int64))


ONE = [[K.CRITIC_STICK_PATH]]
EIGHT = [[K.CRITIC_TWIRLING, K.CRITIC_STICK_PATH, K.CRITIC_TOWARD_GLOBAL_PLAN, K.CRITIC_PURE_PURSUIT,
          K.CRITIC_SHORTEST_ANGLE, K.CRITIC_COLLISION, K.CRITIC_COLLISION_MIN_MAX, K.CRITIC_TWIRLING]]


@pytest.mark.parametrize("stack", ONE + STACKS + EIGHT, ids=lambda s: "-".join(str(k) for k in s))
def test_critic_stack_sizes_against_oracle(stack):
    sc = scenes.bench_scene("C1")
    post = np.array([[1.05, 0.45, z, 0.0] for z in np.arange(0.05, 1.0, 0.05)], dtype=np.float32)
    cloud = np.concatenate([sc.cloud, post])
    th = configs.dd_simple_shipped(critics=[_critic(k) for k in stack])
    assert th.n_critics == len(stack)
    tick = scenes.tick_input(twist=(0.4, 0.0, 0.1))
    with LocalPlanner([th], max_points=len(cloud)) as lp:
        lp.set_cloud(cloud)
        lp.setPlan(sc.plan)
        res = lp.tick(th.name.decode(), tick)
        costs, steps, smp = (a.copy() for a in lp.debug())
    o = oracle.tick(th, cloud, sc.plan, tick, n_threads=8, want_margin=True)
    np.testing.assert_array_equal(steps, o.steps)
    np.testing.assert_array_equal(smp, o.samples)
    assert not np.isnan(costs).any()
    # a point within 1e-4 m of a cuboid face may fall either way (the suite's rule for collision verdicts)
    fragile = np.abs(o.min_margin) < TOL
    neg = (costs < 0) | (o.costs < 0)
    assert not (neg & (costs != o.costs) & ~fragile).any()
    both = (costs >= 0) & (o.costs >= 0)
    assert both.any() and np.max(np.abs(costs[both] - o.costs[both])) <= TOL
    if not (neg & (costs != o.costs)).any():
        assert res.planner_state == o.result.planner_state
        if res.best_index != o.result.best_index:                      # libm-level near-tie
            assert abs(costs[res.best_index] - o.costs[o.result.best_index]) <= 1e-6
