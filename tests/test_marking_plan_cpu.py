"""make_update_frame() and plan_fused_update() of csrc/marking_plan.hip.h -- the transforms and MarkParams of one marking
update and every number its fused launches get -- compiled into a stand-alone host program
(tests/cpp/marking_plan_test.cpp) and replayed over tests/golden/marking_plan_cases.bin: the inputs of recorded updates
and what the engine launched for them before the plan was split off (recorded on an MI355X over one run of
tests/test_marking_gpu.py).  The program also checks the n_part estimate by hand and the plan's invariants under every
non-default knob.  It makes no HIP call, so it runs without a GPU."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_tick_plan_cpu import CSRC, HIPCC, makefile_defines


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_marking_plan_launches_what_the_recorded_updates_launched():
    golden = os.path.join(ROOT, "tests", "golden", "marking_plan_cases.bin")
    data, n_golden, at = open(golden, "rb").read(), 0, 0
    while at < len(data):                                   # u32 magic, input bytes, output bytes, then both
        magic, n_in, n_out = struct.unpack_from("<III", data, at)
        assert magic == 0x4C504B4D
        at += 12 + n_in + n_out
        n_golden += 1
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "marking_plan_test")
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", *makefile_defines(), "-O3", "-std=c++17", "-Wall",
                            "-Wno-unused-function", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "marking_plan_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe, golden], capture_output=True, text=True)
        assert r.returncode == 0 and "marking plan OK" in r.stdout, (r.stdout, r.stderr)
        m = re.search(r"marking plan OK: (\d+) records \((\d+) fused, (\d+) knob variants\)", r.stdout)
        # it replays every record or fails: a few hundred updates, each fused one again under four knobs
        assert 100 <= int(m.group(1)) == n_golden and int(m.group(2)) >= 50 and int(m.group(3)) == 4 * int(m.group(2)), r.stdout
