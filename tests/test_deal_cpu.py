"""The deal of the load-feedback assignment (deal_slot() of csrc/rollout_kernels.hip.h) and plan_tick()'s choice of it
(TickPlan::deal of csrc/tick_plan.hip.h), compiled into a stand-alone host program (tests/cpp/deal_test.cpp):
  * every mode (0 snake, 1 sorted, 2 light tail) is a bijection from an assignment group's ranks onto the slots k_score's
    workgroups read for that group, for n_local 1 .. 260 and around multiples of tile and of G * tile up to 4200, tiles
    2 .. 16, 1 .. 4 groups;
  * mode 0 equals the formula assign_block had before, restated in the program, rank for rank (tail-round layouts too);
  * in mode 1 the ranks of workgroup b precede those of workgroup b + G and the workgroup sizes are tile / tile - 1 as
    DESIGN.md section 4 states; in mode 2 the head workgroups hold the heaviest ranks;
  * plan_tick picks snake on the C2 tick (one round), sorted on the C3 tick, snake on a first tick and after a changed
    shard size (no assignment), what DDDMR_DEAL = 0 / 1 / 2 force, and the snake with the tail-round knob.
The program makes no HIP call, so it runs without a GPU; it is built and run once plainly and once under the address and
undefined-behaviour sanitizers.  The recorded plans of tests/golden/tick_plan_cases.bin replay byte for byte as before
(DevTick is unchanged): tests/cpp/tick_plan_test.cpp is run on them here once more."""
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


def build(tmp, source, opt, extra=()):
    exe = os.path.join(tmp, os.path.splitext(source)[0])
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", *makefile_defines(), opt, "-g", "-std=c++17", "-Wall",
                        "-Wno-unused-function", *extra, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", source), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("sanitize", [[], ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_every_deal_is_a_bijection_and_plan_tick_picks_it_as_specified(sanitize):
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, "deal_test.cpp", "-O1" if sanitize else "-O3", sanitize)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "deal OK" in r.stdout, (r.stdout, r.stderr)
        m = re.search(r"deal OK: (\d+) layouts, (\d+) decisions", r.stdout)
        assert int(m.group(1)) >= 4 * 15 * 260 and int(m.group(2)) >= 15, r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_recorded_plans_still_replay_byte_for_byte():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, "tick_plan_test.cpp", "-O3")
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "tick_plan_cases.bin")], capture_output=True, text=True)
        assert r.returncode == 0 and "tick plan OK" in r.stdout, (r.stdout, r.stderr)
