"""The planner pin on the device: dddmr_rollout_global_plan_* against tests/golden/REF_GP_cloud_*.npz, the answers of the
reference's own a_star_on_pre_graph.cpp (O2 build) on the four committed cloud cases -- every committed FOUND query and the
no-path queries on which the reference is defined (start_lone, start_in_pocket).  Reads only tests/golden/ and the case
generators, never oracle/_ref/ or a reference checkout.

The reference was handed the rows of static_layer_ref.build, so each case first asserts that the device's own rows are
those bytes (read the way tests/test_static_layer_gpu.py reads them) and that their digests are the golden's; then status,
path, n_expanded (the reference's closed count) and the goal's g equal the reference's on bits.  The pin's hand-built CSR
graphs (tests/helpers/global_plan_pin_cases.py) cannot reach the device: the static layer builds its own graph from a
cloud, so they hold the restatement alone (tests/test_global_plan_pin_cpu.py)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import configs, global_plan, stack, static_layer
from dddmr_navigation_amd.local_planner import LocalPlanner
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import global_plan_ref as G  # noqa: E402
import global_plan_cases as Cs  # noqa: E402
import global_plan_pin_golden as Gd  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MAX_NODES = 4096


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=1000) as p:
        yield p


@pytest.mark.parametrize("name", Gd.CLOUD_CASES)
def test_device_against_the_references_answers(lp, name):
    golden = Gd.load(f"REF_GP_cloud_{name}.npz")
    c, ref = Cs.case(name), Cs.static_ref(name)
    assert len(c["ground"]) <= 2615 and golden["answers"]
    sl = static_layer.StaticLayer(lp, static_layer.shipped_config(max_ground_points=MAX_NODES, max_map_points=8192, max_edges=400_000, **c["cfg"]))
    sl.build(c["ground"], c["map"])
    st = stack.PerceptionStack(lp, host_layers=(c["dgraph"],), n_ground=len(c["ground"]), max_changes=len(c["ground"]) + 1)
    st.update()
    rows = sl.graph()
    np.testing.assert_array_equal(rows["row_start"], ref["row_start"], err_msg=name)
    np.testing.assert_array_equal(rows["neighbour"], ref["neighbour"], err_msg=name)
    np.testing.assert_array_equal(np.asarray(rows["weight"], F).view(np.uint32), np.asarray(ref["weight"], F).view(np.uint32), err_msg=name)
    assert st.min_dgraph().tobytes() == np.asarray(c["dgraph"], np.float64).tobytes()
    queries = {q[0]: q for q in Cs.queries() if q[1] == name}
    for label, want in golden["answers"].items():
        q = queries[label]
        sha = json.loads(golden["sha256"][label])
        for k, t in (("row_start", np.uint32), ("neighbour", np.uint32), ("weight", np.float32)):
            assert hashlib.sha256(np.ascontiguousarray(rows[k], t).tobytes()).hexdigest() == sha[k], (label, k)
        assert hashlib.sha256(st.min_dgraph().tobytes()).hexdigest() == sha["dgraph"] and \
            hashlib.sha256(np.ascontiguousarray(c["ground"], F).tobytes()).hexdigest() == sha["ground"], label
        cfg = json.loads(golden["config"][label])
        assert (cfg["start"], cfg["goal"], cfg["turning_weight"]) == (q[2], q[3], q[4])
        gp = global_plan.GlobalPlan(lp, global_plan.shipped_config(max_open_entries=1 << 16, max_expansions=MAX_NODES, turning_weight=q[4],
                                                                   **c["plan_cfg"]), MAX_NODES)
        gp.set_node_weights(c["weights"] if q[5] else None)
        got = gp.plan(q[2], q[3])
        print(f"{label}: status {got.status}, {len(got.path)} nodes, expanded {got.n_expanded}, g {got.g_goal!r} | reference {want['status']}, "
              f"{len(want['path'])}, {want['n_closed']}, {want['g_goal']!r}")
        assert got.status == want["status"], label
        assert got.path.tolist() == want["path"].tolist(), label
        assert got.n_expanded == want["n_closed"], label
        assert F(got.g_goal).view(np.uint32) == F(want["g_goal"]).view(np.uint32), label
    # (tests/test_global_plan_pin_cpu.py asserts that every committed FOUND query is among the goldens)
    labels = set(golden["answers"])
    assert sum(a["status"] == G.FOUND for a in golden["answers"].values()) >= 2
    if name == "floor":
        assert {"start_lone", "start_in_pocket"} <= labels and all(golden["answers"][k]["status"] == G.NO_PATH for k in ("start_lone", "start_in_pocket"))
