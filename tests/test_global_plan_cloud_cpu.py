"""CPU side of the global planner's default A* on the device (A_Star_on_Graph::getPath, a_star_on_pc.cpp:200-329): what the
cases of tests/test_global_plan_cloud_gpu.py hold, the pure arithmetic header from a plain host build (also under the
sanitizers), the ROS-side bridge against a fake C-ABI, the struct the sizeof table does not know, and the restatement's
line of sight against a second brute-force count."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import global_plan_cloud_ref as R  # noqa: E402
import global_plan_cloud_cases as Cs  # noqa: E402

CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")
INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]
CXX = shutil.which("g++") or shutil.which("c++")
F = np.float32
D = np.float64


def test_struct_size_and_constants():
    """the struct the sizeof table does not know (global_plan_cloud.hip.h pins the same number with a static_assert)"""
    assert C.sizeof(K.GlobalPlanCloudResult) == 56 and K.GlobalPlanCloudResult.n_knn_fallbacks.offset == C.sizeof(K.GlobalPlanResult) == 32
    assert K.GLOBAL_PLAN_ROW_FULL == R.ROW_FULL == 4
    text = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    for name, value in (("ROW_FULL", K.GLOBAL_PLAN_ROW_FULL), ("CLOUD_MAX_SUCCESSORS", R.MAX_SUCCESSORS), ("LOS_MAX_SAMPLES", R.LOS_MAX_SAMPLES)):
        assert int(re.search(rf"#define\s+DDDMR_GLOBAL_PLAN_{name}\s+(\d+)", text).group(1)) == value, name
    assert (K.GLOBAL_PLAN_CLOUD_MAX_SUCCESSORS, K.GLOBAL_PLAN_LOS_MAX_SAMPLES) == (R.MAX_SUCCESSORS, R.LOS_MAX_SAMPLES)
    for name in ("global_plan_set_graph_node_weights", "global_plan_set_lethal_points", "global_plan_plan_on_cloud"):
        assert "dddmr_rollout_" + name in K.SIGNATURES and f"int dddmr_rollout_{name}(" in text


def test_cases_hold_what_the_gpu_tests_rely_on():
    found = Cs.check_cases()
    print(found)
    assert found["path_with_lethal"] > found["path_without"]
    labels = [q[0] for q in Cs.queries() + Cs.CAP_QUERIES]
    assert len(labels) == len(set(labels))
    for name in ("floor", "floor_shifted", "lattice", "cluster", "far_lone"):
        c = Cs.case(name)
        assert len(c["ground"]) <= 4096 and len(c["dgraph"]) == len(c["ground"]) + 1 and len(c["lethal"]) <= 4096
    # the jittered floor has no equal distances among a node's successors; the lattice has hardly anything else
    g = Cs.case("floor")["ground"]
    for n in (0, 100, 333, Cs.ISLAND, Cs.LONE):
        _, d2, _ = R.successors(g, n, 0.5)
        assert len(np.unique(d2)) == len(d2)
    _, d2, _ = R.successors(Cs.case("lattice")["ground"], Cs.node(10, 10), 0.5)
    assert len(np.unique(d2)) < len(d2)


def test_successors_of_the_restatement():
    """strictly inside the radius; fewer than 8: the 8 nearest whatever their distance; ascending (d2, index)"""
    g = np.array([[0.25 * i, 0, 0] for i in range(12)], F)
    ids, d2, fb = R.successors(g, 5, 0.5)                                      # 0.5 m itself is outside: 3 nodes, so the 8 nearest
    assert fb and ids.tolist() == [5, 4, 6, 3, 7, 2, 8, 1] and d2[0] == 0 and d2[-1] == F(1.0)
    g2 = np.concatenate([g, g[4:7] + F([0, 0.1, 0]), g[4:7] - F([0, 0.1, 0])])
    ids, d2, fb = R.successors(g2, 5, 0.5)
    assert not fb and len(ids) == 9 and ids[0] == 5 and (np.diff(d2) >= 0).all() and (d2 < F(0.25)).all()
    # squared in float (nanoflann_pcl.hpp:202), not in double as the static layer's sl_radius2: 0.4 tells the two apart
    assert R.radius2(0.4) == F(F(0.4) * F(0.4)) == F(0.16000001) and R.radius2(0.4) != F(D(0.4) * D(0.4))


def test_line_of_sight_against_a_second_brute_force_count():
    """random segments over a random lethal cloud: the restatement's verdict against the OR over a distance table of all the
    samples, whose t come from a float32 cumulative sum (written apart from los_ts)"""
    rng = np.random.default_rng(3)
    lethal = rng.uniform(0, 4, (150, 3)).astype(F) * F([1, 1, 0.1])
    lethal = np.concatenate([lethal, lethal[:10]])                             # ten points twice
    verdicts = {True: 0, False: 0}
    for _ in range(300):
        a = (rng.uniform(0, 4, 3) * [1, 1, 0.1]).astype(F)
        b = (a + rng.uniform(-1, 1, 3) * [1, 1, 0.05]).astype(F)
        ins = float(rng.choice([0.1, 0.15, 0.2]))
        if np.linalg.norm(b - a) < 2 * ins:
            continue
        clear, capped, n = R.line_of_sight(a, b, ins, lethal)
        dt = R.los_dt(a, b, ins)
        t = np.concatenate([[F(0)], np.cumsum(np.full(n + 2, dt, F), dtype=F)])   # (a float32 running sum: sequential additions)
        t = t[t.astype(D) <= 1.0 + D(dt)]
        assert len(t) == n and not capped
        r = np.where(t >= 1, F(1), t).astype(F)
        samples = (a[None, :] + ((b - a).astype(F)[None, :] * r[:, None]).astype(F)).astype(F)
        counts = R.lethal_count_brute(lethal, samples, ins)
        assert clear == (not (counts > 1).any())
        verdicts[clear] += 1
    print(verdicts)
    assert min(verdicts.values()) > 20
    # one lethal point alone never blocks; the same point twice does; no cloud at all: clear
    p = np.array([[1.0, 0.0, 0.0]], F)
    a, b = F([0, 0, 0]), F([2, 0, 0])
    assert R.line_of_sight(a, b, 0.15, p)[0] and not R.line_of_sight(a, b, 0.15, np.concatenate([p, p]))[0]
    assert R.line_of_sight(a, b, 0.15, np.zeros((0, 3), F))[0]
    assert R.line_of_sight(F([0, 0, 0]), F([700, 0, 0]), 0.15, p)[:2] == (False, True)     # the sample cap


def _build(tmp, src, *flags, inc=("-I", CSRC)):
    exe = os.path.join(tmp, "t")
    r = subprocess.run([CXX, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, *inc,
                        os.path.join(ROOT, "tests", "cpp", src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_arithmetic_header_against_hand_computed_values(flags):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([_build(tmp, "global_plan_cloud_plan_test.cpp", *flags)], capture_output=True, text=True)
        assert r.returncode == 0 and "global plan cloud arithmetic OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_bridge_against_a_fake_abi():
    with tempfile.TemporaryDirectory() as tmp:
        exe = _build(tmp, "global_plan_cloud_bridge_test.cpp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", inc=INC)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "global plan cloud bridge OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_bridge_syntax_with_the_stand_in_pcl_types():
    src = """
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "dddmr_rollout_adapter/global_plan_bridge.h"
int use(dddmr_rollout_ctx* ctx, const pcl::PointCloud<pcl::PointXYZI>& aggregate_lethal, const pcl::PointXYZ& start, const pcl::PointXYZ& goal) {
  dddmr_rollout_adapter::GlobalPlanBridge b;
  dddmr_global_plan_config cfg = {};
  cfg.inscribed_radius = 0.15; cfg.a_star_expanding_radius = 0.5; cfg.max_queries = 1; cfg.max_open_entries = 1 << 20; cfg.max_expansions = 1 << 17;
  int rc = b.create(ctx, cfg, 1 << 17);
  rc += b.setLethalCloud(aggregate_lethal);
  std::vector<float> w(10, 0.f);
  rc += b.setGraphNodeWeights(w);
  std::vector<uint32_t> ids;
  dddmr_global_plan_cloud_result res;
  rc += b.planOnCloud(start, goal, ids, &res);
  return rc + (int)res.n_los_blocked + (int)ids.size();
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.cpp")
        open(path, "w").write(src)
        r = subprocess.run([CXX, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), *INC, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
