"""SubmapBridge (submap_bridge.h: create, addKeyframe, warmUp, swapIfReady): compiled without ROS against a fake C-ABI
and run (tests/cpp/submap_bridge_test.cpp), and syntax-checked with the stand-in PCL headers of tests/stubs/."""
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_submap_bridge_against_a_fake_abi():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "submap_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *INC,
                            os.path.join(ROOT, "tests", "cpp", "submap_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "submap bridge OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_submap_bridge_syntax_with_the_stand_in_pcl_types():
    src = """
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "dddmr_rollout_adapter/submap_bridge.h"
struct Affine3d { double m[16]; double operator()(int r, int c) const { return m[4 * c + r]; } };
struct Point { double x, y, z; };
int use(dddmr_rollout_ctx* ctx, const pcl::PointCloud<pcl::PointXYZI>& corner, const pcl::PointCloud<pcl::PointXYZI>& ground,
        const Affine3d& trans_m2b_af3, const Point& position, const pcl::PointXYZ& robot) {
  dddmr_rollout_adapter::SubmapBridge b;
  int rc = b.create(ctx, 1024, 1 << 22, 1 << 21);
  int32_t id = -1;
  rc += b.addKeyframe(corner, ground, trans_m2b_af3, position, &id);
  dddmr_submap_stats st;
  rc += b.warmUp(robot, 50.0, &st);
  bool swapped = false;
  if (b.warmed()) rc += b.swapIfReady(&swapped);
  return rc + id + (int)st.n_ground + (int)swapped;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.cpp")
        open(path, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), *INC, path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
