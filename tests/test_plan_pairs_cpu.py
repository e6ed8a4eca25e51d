"""plan_pack_pairs() of csrc/rollout_kernels.hip.h -- the prune plan as pair records for k_score's phase P, x0 x1 y0 y1
z0 z1 for poses (2i, 2i+1), padded with copies of the last pose to whole loop trips plus one chunk of slack -- compiled
into a stand-alone host program (tests/cpp/plan_pairs_test.cpp) and compared with a plain numpy repack.  The program
makes no HIP call, so it runs without a GPU."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")


def header_constants():
    text = open(os.path.join(CSRC, "rollout_kernels.hip.h")).read()
    chunk = int(re.search(r"^constexpr int kPlanChunk = (\d+);", text, re.M).group(1))
    assert re.search(r"^constexpr int kPlanTrip = 2 \* kPlanChunk;", text, re.M)
    return chunk, 2 * chunk


def numpy_repack(xyzw, chunk, trip):
    """what the walk expects: ceil(m / trip) trips of poses, one chunk of slack, the last pose repeated behind the plan"""
    m = len(xyzw)
    n = -(-m // trip) * trip + chunk
    p = xyzw[np.minimum(np.arange(n), m - 1), :3] if m else np.zeros((n, 3), np.float32)
    return p.reshape(n // 2, 2, 3).transpose(0, 2, 1).reshape(-1)      # [pair][x y z][pose of the pair]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_pair_records_match_a_numpy_repack():
    chunk, trip = header_constants()
    lengths = list(range(0, 2 * trip + 2)) + [80]
    rng = np.random.default_rng(18)
    plans = [rng.uniform(-50.0, 50.0, (m, 4)).astype(np.float32) for m in lengths]     # w is noise: it must not travel
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, n) for n in ("plan_pairs_test", "in.bin", "out.bin"))
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function",
                            "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "plan_pairs_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        with open(fin, "wb") as f:
            for p in plans:
                f.write(struct.pack("<I", len(p)) + p.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0 and f"plan pairs OK: {len(plans)} cases" in r.stdout, (r.stdout, r.stderr)
        blob = open(fout, "rb").read()
    assert struct.unpack_from("<3I", blob, 0) == (chunk, trip, 3)
    ofs = 12
    for p in plans:
        m = len(p)
        (n,) = struct.unpack_from("<Q", blob, ofs)
        got = np.frombuffer(blob, np.float32, 3 * n, ofs + 8)
        ofs += 8 + 12 * n
        # the size: whole trips that cover the plan, then one chunk of slack for the last request ahead
        assert n == -(-m // trip) * trip + chunk and n - chunk >= m and n - chunk - m < trip and n % 2 == 0, (m, n)
        np.testing.assert_array_equal(got.view(np.uint32), numpy_repack(p, chunk, trip).view(np.uint32), err_msg=f"m = {m}")
        # the same, spelled out: pair order, and every pose behind the plan is the last one
        rec = got.reshape(n // 2, 3, 2)
        for i in range(m):
            assert rec[i // 2, :, i % 2].tobytes() == p[i, :3].tobytes(), (m, i)
        for i in range(m, n):
            want = p[m - 1, :3] if m else np.zeros(3, np.float32)
            assert rec[i // 2, :, i % 2].tobytes() == want.tobytes(), (m, i)
    assert ofs == len(blob)
