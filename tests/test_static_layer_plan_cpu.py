"""csrc/static_layer_plan.hip.h (the static layer's pure host arithmetic) built with a plain host compiler and run
(tests/cpp/static_layer_plan_test.cpp): the adaptive radii against the bit-pattern table of test_static_layer_cpu.py, the
grid cell choice and the edge-capacity decision.  One stand-alone build runs under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import static_layer_ref as R  # noqa: E402
import static_layer_cases as Cs  # noqa: E402
from test_static_layer_cpu import R2_BITS  # noqa: E402

CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
F = np.float32
pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")


def build(tmp, *flags):
    exe = os.path.join(tmp, "static_layer_plan_test")
    r = subprocess.run([CXX, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "static_layer_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return r.stdout.splitlines()


LINES = ["R", "Q 1.5", "Q 0.6", "Q 1000", "C 0 1.5 0.5 0.6", "C 1 1.5 0.5 0.6", "C 0 0.01 0.01 0.01", "C 0 900 30 30",
         "E 0 0", "E 100 100", "E 101 100", "E 4294967296 4294967295", "E 1073741824 1073741824"]


def check(out):
    assert out[0].split() == ["R"] + ["%08x" % b for b in R2_BITS]
    assert out[1:4] == ["Q %08x" % int(R.radius2(r).view(np.uint32)) for r in (1.5, 0.6, 1000.0)]
    bits = lambda v: "%08x" % int(F(v).view(np.uint32))
    # fixed mode: half of radius + pad, so the ball is about four cells wide; adaptive: from r_1 = 0.7; the map's and the
    # zones' cells follow their radii between 0.25 m and 4 m
    fixed, adaptive = F(0.5) * (F(1.5) + F(1e-3)), F(0.5) * (F(R.adaptive_radius(1)) + F(1e-3))
    assert out[4] == f"C {bits(fixed)} {bits(0.5)} {bits(0.6)}"
    assert out[5] == f"C {bits(adaptive)} {bits(0.5)} {bits(0.6)}"
    assert out[6] == f"C {bits(0.05)} {bits(0.25)} {bits(0.25)}"
    assert out[7] == f"C {bits(64.0)} {bits(4.0)} {bits(4.0)}"
    assert fixed == Cs.ground_cell(R.config()) and adaptive == Cs.ground_cell(R.config(use_adaptive_connection=1))
    assert 3.9 < 2 * (1.5 + 1e-3) / float(fixed) < 4.1
    assert [l.split()[1] for l in out[8:13]] == ["1", "1", "0", "0", "1"]


def test_plan_header_against_the_tables():
    with tempfile.TemporaryDirectory() as tmp:
        check(run(build(tmp), LINES))


def test_plan_header_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        check(run(build(tmp, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), LINES))
