"""The Python binding end to end on the device, once: clouds of every accepted layout go in through set_cloud and come
back through get_cloud, and the per-trajectory getters of a tick return arrays of the documented rank and dtype whose
lengths are those of the result struct.  What is expected comes from the inputs and the result, never from a second call."""
import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner

pytestmark = pytest.mark.gpu

THEORY = "differential_drive_simple"


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner(configs.shipped_theories(), device=0, max_points=64) as planner:
        yield planner


@pytest.mark.parametrize("n", [0, 1, 5])
@pytest.mark.parametrize("cols,dtype", [(3, np.float32), (4, np.float32), (6, np.float64)])
def test_cloud_round_trip(lp, n, cols, dtype):
    rng = np.random.default_rng(100 * n + cols)
    cloud = rng.uniform(-2.0, 2.0, size=(n, cols)).astype(np.float32).astype(dtype)      # (exact in float32 either way)
    lp.set_cloud(cloud)
    got = lp.get_cloud()
    assert got.shape == (n, 4) and got.dtype == np.float32
    assert np.array_equal(got[:, :3], cloud[:, :3].astype(np.float32))
    if n and cols == 3:
        assert np.all(got[:, 3] == 0.0)
    elif n:
        assert np.array_equal(got[:, 3], cloud[:, 3].astype(np.float32))


def test_getters_after_a_tick(lp):
    lp.set_cloud(scenes.playground_scene().cloud)
    lp.setPlan(np.array([[0.5, 0.0, 0.0, 0, 0, 0, 1], [1.0, 0.0, 0.0, 0, 0, 0, 1]], dtype=np.float64))
    tick_in = scenes.tick_input(twist=(0.4, 0.0, 0.0))
    res = lp.tick(THEORY, tick_in)
    assert res is lp.last_result and res.n_samples > 0 and res.local_begin == 0 and res.n_local == res.n_samples   # one rank
    n = int(res.n_local)

    smp = lp.samples(THEORY, tick_in)
    assert smp.shape == (int(res.n_samples), 3) and smp.dtype == np.float32

    costs, steps, dbg_smp = lp.debug()
    assert costs.shape == (n,) and costs.dtype == np.float64
    assert steps.shape == (n,) and steps.dtype == np.int32
    assert dbg_smp.shape == (n, 3) and dbg_smp.dtype == np.float32
    assert res.planner_state != K.TRAJECTORY_FOUND or 0 <= res.best_index < n

    poses = lp.pose_arrays()
    accepted = lp.pose_arrays(accepted_only=True)
    assert poses.ndim == 2 and poses.shape[1] == 7 and poses.dtype == np.float64
    assert accepted.ndim == 2 and accepted.shape[1] == 7 and accepted.dtype == np.float64
    assert len(poses) == int(steps[steps > 0].sum()) and len(accepted) == int(steps[(steps > 0) & (costs >= 0)].sum())

    best, cub = lp.best_poses(), lp.best_cuboids()
    n_best = int(steps[res.best_index]) if res.best_index >= 0 else 0
    assert best.shape == (n_best, 7) and best.dtype == np.float64
    assert cub.shape == (n_best, 8, 3) and cub.dtype == np.float32
