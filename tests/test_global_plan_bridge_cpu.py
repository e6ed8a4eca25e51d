"""GlobalPlanBridge (global_plan_bridge.h: makePlanIds, dwaGoalPivot, pathPoses): compiled without ROS against a fake
C-ABI and run (tests/cpp/global_plan_bridge_test.cpp), and syntax-checked with the stand-in PCL headers of tests/stubs/."""
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_global_plan_bridge_against_a_fake_abi():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "global_plan_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *INC,
                            os.path.join(ROOT, "tests", "cpp", "global_plan_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "global plan bridge OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_global_plan_bridge_syntax_with_the_stand_in_pcl_types():
    src = """
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "dddmr_rollout_adapter/global_plan_bridge.h"
#include "dddmr_rollout.hpp"
typedef pcl::PointCloud<pcl::PointXYZI> CloudT;
double use(dddmr_rollout_ctx* ctx, const CloudT& pcl_ground, const pcl::PointCloud<pcl::PointXYZ>& pcl_global_path) {
  dddmr_rollout_adapter::GlobalPlanBridge b;
  dddmr_global_plan_config cfg = {};
  cfg.turning_weight = 0.1; cfg.a_star_expanding_radius = 0.5; cfg.max_queries = 1; cfg.max_open_entries = 1 << 20; cfg.max_expansions = 1 << 17;
  int rc = b.create(ctx, cfg, 1 << 17);
  std::vector<float> w;
  for (const auto& p : pcl_ground.points) w.push_back(p.intensity);
  rc += b.setNodeWeights(w);
  std::vector<uint32_t> ids;
  dddmr_global_plan_result res;
  rc += b.makePlanIds({{0.f, 0.f, 0.f}}, {{3.f, 4.f, 0.f}}, ids, &res);
  std::vector<dddmr_rollout_adapter::GlobalPlanBridge::Point> path;
  for (const auto& p : pcl_global_path.points) path.push_back({{p.x, p.y, p.z}});
  size_t pivot = 0;
  rc += b.dwaGoalPivot(path, 0, 2.0, &pivot);
  double sum = 0;
  for (const auto& row : dddmr_rollout_adapter::GlobalPlanBridge::pathPoses(ids, pcl_ground)) sum += row[0] + row[6];
  return sum + rc + pivot + res.g_goal;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.cpp")
        open(path, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), *INC, path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
