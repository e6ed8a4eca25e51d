"""The class-major deal of the rollout workgroups -- class_major_position() and heading_rows_shared() of
csrc/rollout_kernels.hip.h -- compiled into a stand-alone host program (tests/cpp/heading_rows_test.cpp): for
begin % nth in {0, 1, nth - 1}, n_local a multiple of nth, not a multiple and smaller than nth, and nth in {1, 2, 8, 32}
the position -> li function is a permutation of [0, n_local) along which the classes ascend, and where the predicate
holds no window of rt positions spans more than two classes; the predicate is false for list mode, the reference's
step rule and thin shards.  The same program then plans named ticks through plan_tick() of csrc/tick_plan.hip.h, one per
branch of the rule that decides whether a tick shares heading rows (rows on within 72 KB of dynamic LDS, off where they
would push the rollout beyond it, on again where the rollout alone is beyond it, off beyond 150 KB, off for the knob,
list mode and an empty shard), against values worked out by hand.  The program makes no HIP call, so it runs without a
GPU; it is built and run once plainly and once under the address and undefined-behaviour sanitizers."""
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
def test_class_major_order_is_a_permutation_with_two_classes_per_window(sanitize):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "heading_rows_test")
        opt = "-O1" if sanitize else "-O3"
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", *makefile_defines(), opt, "-g", "-std=c++17", "-Wall",
                            "-Wno-unused-function", *sanitize, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "heading_rows_test.cpp"),
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "heading rows OK" in r.stdout, (r.stdout, r.stderr)
        m = re.search(r"heading rows OK: (\d+) shapes, (\d+) windows, (\d+) plan cases", r.stdout)
        assert int(m.group(1)) >= 100 and int(m.group(2)) >= 1000 and int(m.group(3)) >= 12, r.stdout
