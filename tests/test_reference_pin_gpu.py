"""The HIP tick against the recorded outputs of the reference's own rollout code (tests/golden/REF_*.npz, written by
tests/golden/make_ref_golden.py from the compiled reference).  Reads only tests/golden/: inputs and expected outputs
are both in the fixture.  Bar of test_parity_gpu.py: exact samples and step counts, equal reject codes apart from
points the fragile-point rule exempts, |cost difference| <= 1e-4 and the same winner."""
import glob
import importlib.util
import os

import numpy as np
import pytest

from dddmr_navigation_amd.local_planner import LocalPlanner

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4
FILES = sorted(f for f in glob.glob(os.path.join(GOLD, "REF_*.npz"))
               if not os.path.basename(f).startswith(("REF_MCL_", "REF_GP_")))      # (the particle-measure and planner pins', formats of their own)

_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(GOLD, "make_ref_golden.py"))
_mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mk)


def test_fixtures_present():
    assert len(FILES) >= 10


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_hip_matches_recorded_reference(path):
    th, ti, cloud, plan, g = _mk.load(path)
    with LocalPlanner([th], max_points=max(len(cloud), 16)) as lp:
        lp.set_cloud(cloud)
        lp.setPlan(plan)
        res = lp.tick(th.name.decode(), ti)
        costs, steps, smp = lp.debug()
    np.testing.assert_array_equal(smp, g["samples"])
    np.testing.assert_array_equal(steps, g["steps"])
    fragile = np.abs(g["min_margin"]) < TOL
    neg = (costs < 0) | (g["costs"] < 0)
    flips = neg & (costs != g["costs"])
    assert not (flips & ~fragile).any(), f"reject codes differ at {np.nonzero(flips & ~fragile)[0][:8]}"
    both = (costs >= 0) & (g["costs"] >= 0)
    if both.any():
        assert np.max(np.abs(costs[both] - g["costs"][both])) <= TOL
    if not flips.any():
        state, best, _, _ = g["summary"].tolist()
        best_cost, vx, vy, wz = g["best"].tolist()
        assert res.planner_state == state and res.best_index == best
        assert abs(res.best_cost - best_cost) <= TOL
        assert abs(res.vx - vx) <= TOL and abs(res.vy - vy) <= TOL and abs(res.wz - wz) <= TOL
