"""csrc/point_grid_plan.hip.h -- the host arithmetic around the point grid every spatial query goes through -- compiled into
a stand-alone host program (tests/cpp/point_grid_plan_test.cpp, built like the marking plan's: the header takes PointGrid
and float4 from HIP's headers) that holds every expectation itself:
  stage_cloud   n = 0, 1, 5 at strides 12, 16, 32 against a loop written out; a NaN or an infinity at the first, a middle and
                the last record, on each axis; a finite input the transform turns infinite; submap_transform_row as the
                transform, bit for bit; HostCloud as its thin owner, which keeps what is not finite for cloud_coords_ok
  grid_shape    3 x 2 x 1 m at 0.5 m under a cap of 1000 cells (kept) and of 50 (three powers of 1.3), the origin, a
                degenerate box
  host_cx/cy/cz clamping below, above and at the cell edges of a grid whose origin is at 4 km
  cloud_box_ok  1e6 m, the next float above, an extent of exactly the limit, a NaN bound
The program makes no HIP runtime call, so it runs without a GPU."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_tick_plan_cpu import CSRC, HIPCC


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_point_grid_plan_header_against_its_written_out_expectations():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "point_grid_plan_test")
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC,
                            os.path.join(ROOT, "tests", "cpp", "point_grid_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "point grid plan OK" in r.stdout, (r.stdout, r.stderr)
        # every check ran: 9 staging cases, 81 x 2 placements of a bad coordinate, and the rest
        assert int(re.search(r"point grid plan OK: (\d+) checks", r.stdout).group(1)) >= 300, r.stdout
