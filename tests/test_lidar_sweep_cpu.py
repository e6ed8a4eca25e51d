"""CPU tests of the lidar sweep yardsticks: hand-derivable known answers against the NumPy restatement of
ImageProjection::cloudHandler's front half (tests/helpers/lidar_sweep_ref.py), the condition every generated sweep has to
meet (no fragile decision, a non-trivial answer), and feedSweep() / sweepCloud() of perception_bridge.h compiled with the
address and undefined-behaviour sanitizers against a fake C-ABI (tests/cpp/lidar_sweep_bridge_test.cpp)."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lidar_sweep_ref as R  # noqa: E402
import lidar_sweep_cases as Cs  # noqa: E402

KNOWN = Cs.known_answers()


def answer(name):
    c, raw = KNOWN[name]
    ref = R.stage_one(raw, c)
    assert ref["n_fragile"] == 0, name
    return c, raw, ref


def filled(ref):
    return sorted(map(tuple, np.argwhere(ref["range"] != R.FLT_MAX).tolist()))


def test_two_points_in_one_pixel_the_later_one_wins():
    c, raw, ref = answer("two_points_one_pixel")
    assert filled(ref) == [(9, 10)] and ref["owner"][9, 10] == 1
    assert abs(float(ref["range"][9, 10]) - 6.0) < 1e-5
    np.testing.assert_array_equal(ref["full"][9, 10], R.pitch_removed(raw, c.mount)[1])
    first = R.stage_one(raw[::-1], c)                         # the other order: the 5 m return is the later one
    assert abs(float(first["range"][9, 10]) - 5.0) < 1e-5 and first["owner"][9, 10] == 1


def test_a_row_quotient_of_minus_a_half_lands_in_row_0():
    c, raw, ref = answer("row_quotient_minus_half")
    d = R.Derived(c)
    pts = R.pitch_removed(raw, c.mount)
    row, col, rng, ok, row_angle, _ = R.project(pts, c, d)
    assert abs(row_angle[0] / float(d.res_y) + 0.5) < 1e-3    # the quotient the case was built for
    assert ok[0] and row[0] == 0 and filled(ref) == [(0, 20)]


def test_a_column_on_the_wrap_becomes_column_0():
    c, raw, ref = answer("column_on_the_wrap")
    pts = R.pitch_removed(raw, c.mount)
    horizon = np.arctan2(pts[:, 0], pts[:, 1])
    assert horizon[0] > 3.1 and horizon[1] < -3.1             # columnIdn = 0 and columnIdn = H -> 0
    assert filled(ref) == [(9, 0), (10, 0)]


def test_a_segment_crosses_the_columns_h_minus_1_and_0():
    c, raw, ref = answer("segment_across_the_wrap")
    assert filled(ref) == [(r, col) for r in (9, 10, 11) for col in (0, 1, 62, 63)]
    assert ref["n_labels"] == 1 and (ref["label"][ref["range"] != R.FLT_MAX] == 1).all()
    assert len(ref["cloud"]) == 12 and (ref["cloud"][:, 3] == 1.0).all()
    # raster order: row 9 columns 0, 1, 62, 63, then row 10 ...
    np.testing.assert_array_equal(ref["cloud"][:4, :3], ref["full"][9, [0, 1, 62, 63]])


def test_a_row_of_29_is_invalid_beside_a_row_of_30():
    c, raw, ref = answer("row_of_29_beside_row_of_30")
    assert c.valid_line_num == 2
    assert (ref["label"][9, 0:29] == R.INVALID).all()         # 29 pixels on one line: fewer than 30, fewer than 2 lines
    assert (ref["label"][9, 32:62] == 1).all()                # 30 pixels are valid whatever the lines
    assert ref["n_labels"] == 1 and len(ref["cloud"]) == 30


def test_a_pole_of_5_pixels_in_5_rows_counts_4_lines():
    _, _, ref5 = answer("pole_of_5_needs_5_lines")
    _, _, ref4 = answer("pole_of_5_needs_4_lines")
    assert filled(ref5) == filled(ref4) == [(r, 30) for r in range(8, 13)]
    assert (ref5["label"][8:13, 30] == R.INVALID).all() and len(ref5["cloud"]) == 0      # the seed's row is not counted
    assert (ref4["label"][8:13, 30] == 1).all() and len(ref4["cloud"]) == 5


def test_a_pair_with_an_empty_lower_pixel_is_not_ground():
    c, raw, ref = answer("empty_lower_pixel")
    assert c.gsi >= 1 and filled(ref) == [(0, 6), (1, 5), (1, 6)]
    assert ref["ground"][0, 6] == 1 and ref["ground"][1, 6] == 1                          # the floor pair beside it is
    assert ref["ground"][1, 5] == 0 and ref["ground"][0, 5] == 0
    assert ref["label"][1, 5] == R.INVALID and ref["label"][0, 5] == -1 and ref["label"][1, 6] == -1


def test_labels_follow_the_raster_order_of_the_seeds():
    c, raw, ref = answer("labels_in_seed_order")
    lab = ref["label"]
    assert (lab[2:4, 40:42] == 1).all()                       # seed (2, 40)
    assert (lab[4, 10:12] == R.INVALID).all()                 # seed (4, 10): 2 pixels, invalid, takes no number
    assert (lab[5:7, 3:6] == 2).all()                         # seed (5, 3)
    assert ref["n_labels"] == 2
    assert ref["cloud"][:, 3].tolist() == [1.0] * 4 + [2.0] * 6


def test_derived_constants_are_the_nodes_floats():
    d = R.Derived(R.Config(16, 1000, -15.0, 15.0, 7))
    assert d.res_x == np.float32(2 * np.pi / 1000) and d.res_y == np.float32(np.deg2rad(2.0))
    assert abs(float(d.ang_bottom) - np.deg2rad(15.1)) < 1e-7 and d.ang_bottom.dtype == np.float32
    assert abs(float(d.tan_theta) - np.tan(np.deg2rad(60.0))) < 1e-6 and d.tan_theta.dtype == np.float32


@pytest.mark.parametrize("name", Cs.NAMES)
def test_every_generated_case_has_no_fragile_decision_and_a_non_trivial_answer(name):
    c, raw, ref = Cs.case(name)
    assert ref["n_fragile"] == 0 and ref["fragile_points"] == []
    lab = ref["label"]
    n_ground, n_empty, n_invalid = int(ref["ground"].sum()), int((ref["range"] == R.FLT_MAX).sum()), int((lab == R.INVALID).sum())
    print(f"{name}: {len(raw)} records, {n_ground} ground, {ref['n_labels']} valid segments, {n_invalid} pixels of invalid ones, {n_empty} empty")
    if c.gsi > 0:
        assert n_ground > 0
    else:
        assert n_ground == 0                                   # with ground_scan_index 0 the node marks no ground at all
    assert ref["n_labels"] >= 2 and n_invalid >= 1 and n_empty >= 1
    assert len(ref["cloud"]) == int(((lab > 0) & (lab != R.INVALID)).sum()) > 0
    assert sorted(set(ref["cloud"][:, 3].astype(int).tolist())) == list(range(1, ref["n_labels"] + 1))
    if not name.startswith("4x8"):                             # junk records and second returns are in the input
        assert not np.isfinite(raw).all() and len(raw) > (ref["range"] != R.FLT_MAX).sum()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lidar_sweep_bridge_against_a_fake_abi_under_sanitizers():
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "lidar_sweep_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *inc, os.path.join(ROOT, "tests", "cpp", "lidar_sweep_bridge_test.cpp"),
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "lidar sweep bridge OK" in r.stdout, (r.stdout, r.stderr)
