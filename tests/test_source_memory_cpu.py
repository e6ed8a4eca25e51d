"""Who frees what in the sensor half of the library -- the owners of csrc/dev_memory.hip.h (DevAllocs, HostAllocs, Owned,
dev_realloc, host_mapped_reserve) and the module states built on them -- and in the building blocks of the marking
layers (csrc/marking_buffers.hip.h), compiled into a stand-alone host program
(tests/cpp/source_memory_test.cpp) in which the HIP allocation, memset and copy calls are counting stand-ins on malloc.
For PerceptionScratch, DepthSource (with and without its raw staging), DepthImage, DepthClear, LidarSweep (alone and with
its features on) and LidarFeatures, and for StoreBuf (without heads and with the fov flag, as the lidar layer allocates
it; with heads and without the flag, as the depth layer does), ClusterScratch (temp_bytes given) and GridBuf at table 8,
pool 4, n_ground 1, N = 2 -- the smallest shapes that reach every allocation: a clean alloc + free leaves
nothing live; with the failure placed at every call of the clean pass in turn the alloc reports failure and nothing
stays live, whether the state is freed by name or dies; nothing is freed twice, nothing unknown is freed, no memset or
copy leaves its allocation.  The two growing helpers the same way: grow, grow with every call failing in turn (the
owner no longer holds the old pointer), free.  The program never reaches the HIP runtime, so it runs without a GPU; it is
built and run once plainly and once under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("sanitize", [[], ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_every_state_frees_what_it_allocated_wherever_the_allocation_fails(sanitize):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "source_memory_test")
        opt = "-O1" if sanitize else "-O3"
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", opt, "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                            *sanitize, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "source_memory_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "source memory OK" in r.stdout, (r.stdout, r.stderr)
        m = re.search(r"source memory OK: (\d+) states, (\d+) calls in their clean passes, (\d+) failure placements", r.stdout)
        # 12 states (the stores 21 and 24 allocations, the scratch 19, the grid 2); every call of every clean pass is a
        # failure placement, plus the clean and failing grows of the two helpers
        assert int(m.group(1)) == 12 and int(m.group(2)) == 257 and int(m.group(3)) == 257 + 3 + 4, r.stdout
