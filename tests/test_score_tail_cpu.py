"""score_stack() of csrc/rollout_kernels.hip.h -- the one stacked-scoring function that k_score's single-round tail and
k_finalize both call -- with traj_load_of() and the slot-word pack / unpack helpers, compiled into a stand-alone host
program (tests/cpp/score_tail_test.cpp) that checks them against stacks worked out by hand: every critic kind, a path
critic ahead of a collision critic with a collided trajectory, short plans, pure pursuit's guard, a trajectory that
was not generated, the planner's cost cap, and workgroup counts of 0 .. 1024 in slot word 3.  The program makes no HIP
call, so it runs without a GPU; the second build runs the same checks under the address and undefined-behaviour
sanitizers of the host compiler."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_scoring_function_and_slot_words_against_hand_computed_cases(sanitize):
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "score_tail_test")
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1" if sanitize else "-O3", "-std=c++17", "-Wall",
                            "-Wno-unused-function"] + extra + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "score_tail_test.cpp"),
                                                               "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    m = re.search(r"score tail OK: (\d+) checks", r.stdout)
    assert m and int(m.group(1)) >= 200, (r.stdout, r.stderr)      # (235 when written: nothing compiled out)
