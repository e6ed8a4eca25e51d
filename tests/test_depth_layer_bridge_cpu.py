"""DepthLayerBridge of perception_bridge.h: compiled without ROS against a fake C-ABI and run
(tests/cpp/depth_layer_bridge_test.cpp), and syntax-checked with the stand-in ROS / PCL headers of tests/stubs/."""
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_depth_layer_bridge_against_a_fake_abi():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "depth_layer_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *INC,
                            os.path.join(ROOT, "tests", "cpp", "depth_layer_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "depth layer bridge OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_depth_layer_bridge_syntax_with_the_stand_in_pcl_types():
    src = """
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <geometry_msgs/msg/transform_stamped.hpp>
#include "dddmr_rollout_adapter/perception_bridge.h"
int use(dddmr_rollout_ctx* ctx, const dddmr_depth_layer_config& cfg, const pcl::PointCloud<pcl::PointXYZ>& ground,
        const pcl::PointCloud<pcl::PointXYZI>& map, const geometry_msgs::msg::TransformStamped& gbl2b) {
  dddmr_rollout_adapter::DepthLayerBridge b;
  int rc = b.create(ctx, cfg, ground, ground.points.size(), map);
  dddmr_depth_layer_stats st;
  if (rc == DDDMR_OK && b.ready()) rc = b.clearThenMark(gbl2b, &st);
  pcl::PointCloud<pcl::PointXYZI> lethal, marks;
  b.lethalPointCloud(ground, lethal);
  rc += b.markingPointCloud(marks) + b.reset();
  return rc + (int)lethal.points.size() + (b.dGraphValue(0) > 1.0);
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.cpp")
        open(path, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), *INC, path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
