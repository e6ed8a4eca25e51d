"""plan_tick() of csrc/tick_plan.hip.h -- the shard, the horizon, the local costmap grid, the k_score workgroup shape and
the rollout tile of one tick -- compiled into a stand-alone host program (tests/cpp/tick_plan_test.cpp) and replayed
over tests/golden/tick_plan_cases.bin: the planning inputs of recorded ticks and what the engine decided for them
before plan_tick was split off (recorded on an MI355X).  The program makes no HIP call, so it runs without a GPU."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")


def makefile_defines():
    """-DDDDMR_SCORE_WPE / -DDDDMR_ITEM as csrc/Makefile sets them: both reach the LDS sizes plan_tick works with"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    wpe = re.search(r"^SCORE_WPE \?= (\d+)$", text, re.M).group(1)
    item = re.search(r"^ITEM \?= (\d+)$", text, re.M).group(1)
    return [f"-DDDDMR_SCORE_WPE={wpe}", f"-DDDDMR_ITEM={item}"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_plan_tick_decides_what_the_recorded_ticks_decided():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "tick_plan_test")
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", *makefile_defines(), "-O3", "-std=c++17", "-Wall",
                            "-Wno-unused-function", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "tick_plan_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "tick_plan_cases.bin")], capture_output=True, text=True)
        assert r.returncode == 0 and "tick plan OK" in r.stdout, (r.stdout, r.stderr)
        assert int(re.search(r"tick plan OK: (\d+) records", r.stdout).group(1)) >= 1, r.stdout   # it replays every record or fails
