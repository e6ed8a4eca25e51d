"""StaticLayerBridge (static_layer_bridge.h: regenerate, edges, dGraphValue, setZones, bindToStack): compiled without ROS
against a fake C-ABI and run (tests/cpp/static_layer_bridge_test.cpp), and syntax-checked with the stand-in PCL headers
of tests/stubs/."""
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_static_layer_bridge_against_a_fake_abi():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "static_layer_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *INC,
                            os.path.join(ROOT, "tests", "cpp", "static_layer_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "static layer bridge OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_static_layer_bridge_syntax_with_the_stand_in_pcl_types():
    src = """
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "dddmr_rollout_adapter/static_layer_bridge.h"
typedef pcl::PointCloud<pcl::PointXYZI> CloudT;
double use(dddmr_rollout_ctx* ctx, const CloudT& pcl_ground, const CloudT& pcl_map, const std::vector<const CloudT*>& zones) {
  dddmr_rollout_adapter::StaticLayerBridge b;
  dddmr_static_layer_config cfg = {};
  cfg.max_ground_points = 1 << 17; cfg.max_map_points = 1 << 18; cfg.max_edges = 1 << 24;
  int rc = b.create(ctx, cfg);
  dddmr_static_layer_stats st;
  rc += b.regenerate(pcl_ground, pcl_map, &st);
  double sum = 0;
  for (const auto& e : b.edges(7)) sum += e.second + e.first;
  rc += b.setZones(zones, 0.5);
  rc += b.bindToStack(0, 0) + b.bindToStack(1, 1);
  return sum + b.dGraphValue(7) + b.zoneDGraphValue(7) + rc + (double)st.n_edges;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.cpp")
        open(path, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), *INC, path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
