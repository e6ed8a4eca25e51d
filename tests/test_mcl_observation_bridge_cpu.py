"""The observation calls of LocalizationBridge (localization_bridge.h: configureObservation, prepareObservation,
measurePrepared): compiled without ROS against a fake C-ABI and run (tests/cpp/mcl_observation_bridge_test.cpp), and
syntax-checked with the stand-in PCL headers of tests/stubs/."""
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_observation_bridge_against_a_fake_abi():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mcl_observation_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *INC,
                            os.path.join(ROOT, "tests", "cpp", "mcl_observation_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "mcl observation bridge OK" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_observation_bridge_syntax_with_the_stand_in_pcl_types():
    src = """
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "dddmr_rollout_adapter/localization_bridge.h"
struct Affine3d { double m[16]; double operator()(int r, int c) const { return m[4 * c + r]; } };
struct State { struct { float x_, y_, z_; } pos_; struct { float x_, y_, z_, w_; } rot_; };
int use(dddmr_rollout_ctx* ctx, const pcl::PointCloud<pcl::PointXYZI>& flat, const pcl::PointCloud<pcl::PointXYZI>& less_sharp,
        const Affine3d& trans_b2s_af3, const std::vector<State>& particles) {
  dddmr_rollout_adapter::LocalizationBridge b;
  int rc = b.create(ctx, 0.3, 0.05, 1.0, 6, 1 << 20, 1 << 20, 1 << 14) + b.configureObservation(0.8, 3, 400, 1600);
  dddmr_mcl_observation_stats st;
  rc += b.prepareObservation(flat, less_sharp, trans_b2s_af3, &st) + b.prepareObservation(0, trans_b2s_af3);
  std::vector<float> like, qual;
  float lo, hi;
  if (b.prepared()) rc += b.measurePrepared(particles, like, qual, &lo, &hi);
  return rc + (int)st.branch;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.cpp")
        open(path, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), *INC, path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
