"""plan_tick()'s decision whether k_score walks the prune plan inside the collision walk (TickPlan::fused_walk of
csrc/tick_plan.hip.h), compiled into a stand-alone host program (tests/cpp/fused_walk_test.cpp): named ticks, one per
branch of the rule -- the knob, a lean launch (min-max critic, cuboid beyond the search ball), the collision critic, the
5-point cloud, the plan, the pairs of a workgroup against 256 and against the lane count (forced tiles, both kernels),
the derived share bound 1 - 256 / pairs on either side at C3's (6 x 80) and C2's (8 x 50) shapes and at 512 and 257
pairs, a context's first tick and an empty shard -- against values worked out by hand.  The program makes no HIP call,
so it runs without a GPU; it is built and run once plainly and once under the address and undefined-behaviour
sanitizers."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")


def makefile_defines():
    text = open(os.path.join(CSRC, "Makefile")).read()
    wpe = re.search(r"^SCORE_WPE \?= (\d+)$", text, re.M).group(1)
    item = re.search(r"^ITEM \?= (\d+)$", text, re.M).group(1)
    return [f"-DDDDMR_SCORE_WPE={wpe}", f"-DDDDMR_ITEM={item}"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("sanitize", [[], ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_plan_tick_decides_the_fused_walk_branch_by_branch(sanitize):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fused_walk_test")
        opt = "-O1" if sanitize else "-O3"
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", *makefile_defines(), opt, "-g", "-std=c++17", "-Wall",
                            "-Wno-unused-function", *sanitize, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "fused_walk_test.cpp"),
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "fused walk plan OK" in r.stdout, (r.stdout, r.stderr)
        m = re.search(r"fused walk plan OK: (\d+) cases", r.stdout)
        assert int(m.group(1)) >= 25, r.stdout
