"""sweepAssociation() of perception_bridge.h: compiled without ROS against a fake C-ABI and run
(tests/cpp/sweep_association_bridge_test.cpp), and syntax-checked with the stand-in PCL headers of tests/stubs/."""
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sweep_association_bridge_against_a_fake_abi():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sweep_association_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *INC,
                            os.path.join(ROOT, "tests", "cpp", "sweep_association_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "sweep association bridge OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sweep_association_bridge_syntax_with_the_stand_in_pcl_types():
    src = """
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "dddmr_rollout_adapter/perception_bridge.h"
struct CloudInfo { float start_orientation, end_orientation, orientation_diff; };   // the fields of the feature node's cloud_info message
int use(dddmr_rollout_ctx* ctx, pcl::PointCloud<pcl::PointXYZI>& sharp, pcl::PointCloud<pcl::PointXYZI>& less_sharp,
        pcl::PointCloud<pcl::PointXYZI>& flat, pcl::PointCloud<pcl::PointXYZI>& less_flat, CloudInfo& info,
        pcl::PointCloud<pcl::PointXYZI>& outliers) {
  return dddmr_rollout_adapter::sweepAssociation(ctx, 0, 0, sharp, less_sharp, flat, less_flat, info, outliers) +
         dddmr_rollout_adapter::sweepAssociation(ctx, 0, 1, sharp, less_sharp, flat, less_flat, info, outliers);
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.cpp")
        open(path, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), *INC, path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
