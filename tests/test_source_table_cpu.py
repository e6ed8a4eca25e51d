"""The sensor sources' bookkeeping of csrc/source_table.hip.h -- which calls a source's kind refuses, the scan sources'
rules, the fit of a candidate observation beside the others, the aggregate's layout and the depth sources' queries --
compiled into a stand-alone host program (tests/cpp/source_table_test.cpp).  The header makes no HIP call and uses no HIP
type, so a plain host compiler builds it and it runs without a GPU."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_source_table_rules_and_layout():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "source_table_test")
        r = subprocess.run([CXX, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                            os.path.join(ROOT, "tests", "cpp", "source_table_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "source table OK" in r.stdout, (r.stdout, r.stderr)
        assert int(re.search(r"source table OK: (\d+) checks", r.stdout).group(1)) >= 100, r.stdout   # every group ran
