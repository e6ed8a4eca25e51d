"""CPU tests of the lidar feature yardsticks: the restatement of mcl_feature_node's feature half
(tests/helpers/lidar_features_ref.py) against answers derived by hand from the reference's code
(tests/helpers/lidar_features_cases.py says how), the conditions every parity case has to meet, the new struct and
symbols against the header, and sweepFeatures() of perception_bridge.h compiled with the address and undefined-behaviour
sanitizers against a fake C-ABI (tests/cpp/lidar_features_bridge_test.cpp).  The argument refusals of
set_lidar_sweep_features need a context, hence a device: they are in tests/test_lidar_features_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from dddmr_navigation_amd import _capi as K

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lidar_features_ref as FR  # noqa: E402
import lidar_features_cases as FC  # noqa: E402

HAND = FC.hand_cases()
REPORT = ("edge_breaks", "flat_breaks", "ep_picks", "slot4_pick", "n_occluded", "n_tie_sensitive")


def hand(name):
    h = HAND[name]
    c, raw, ref = FC.hand_sweep(name)
    assert ref["n_fragile"] == 0, name
    f = FR.features(ref, c, h["edge"], h["surf"])
    assert f["n_tie_sensitive"] == 0, name
    return h, c, ref, f


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_hand_derived_answer(name):
    h, c, ref, f = hand(name)
    assert len(f["seg"]["range"]) == h["n_seg"]
    for which, what in enumerate(("sharp", "less sharp", "flat")):
        assert f["lists"][which].tolist() == h["expect"][which], (name, what)


def test_segmented_cloud_and_ring_indices_of_the_wall():
    """8 full rings of 128 behind 8 empty ones: start = count_before - 1 + 5, end = count_after - 1 - 5"""
    h, c, ref, f = hand("candidate_at_slot_ep")
    seg = f["seg"]
    assert seg["start"].tolist() == [4] * 8 + [128 * k + 4 for k in range(8)]
    assert seg["end"].tolist() == [-6] * 8 + [128 * k + 122 for k in range(8)]
    assert (seg["start"][:8] > seg["end"][:8]).all()                                  # an empty row
    assert seg["col"].tolist() == list(range(128)) * 8 and seg["row"].tolist() == [r for r in range(8, 16) for _ in range(128)]
    assert not seg["ground"].any()
    np.testing.assert_array_equal(seg["xyz"], ref["full"][8:].reshape(-1, 3))
    np.testing.assert_array_equal(seg["range"], ref["range"][8:].reshape(-1))


def test_ground_points_are_thinned_and_flagged():
    h, c, ref, f = hand("slot_4_picks_index_0")
    seg = f["seg"]
    cols = list(range(6)) + list(range(10, 121, 5)) + list(range(123, 128))           # j % 5 == 0 or j <= 5 or j >= H - 5
    assert seg["col"].tolist() == cols * 6 and seg["ground"].all()
    assert f["slot4_pick"] and f["n_occluded"] > 0


def test_a_candidate_at_slot_ep_is_taken_before_a_larger_one():
    h, c, ref, f = hand("candidate_at_slot_ep")
    curv = f["curvature"]
    assert f["ep_picks"] == 8 and curv[41] > curv[42] > np.float32(h["edge"])
    assert abs(float(curv[41]) - 3.24) < 1e-3 and abs(float(curv[42]) - 1.44) < 1e-3    # 900 a^2 and 400 a^2 with a = 0.06


def test_curvatures_of_the_cross_sixth_case_are_the_derived_ones():
    h, c, ref, f = hand("next_sixth_best_removed")
    curv = f["curvature"]
    assert abs(float(curv[20]) - 2.2 ** 2) < 1e-3 and abs(float(curv[25]) - 1.2 ** 2) < 1e-3
    assert (np.delete(curv[23:43], 2) < 1.0).all()                                     # sixth 1 has no other candidate
    h, c, ref, f = hand("next_sixth_best_kept")
    assert abs(float(f["curvature"][26]) - 1.2 ** 2) < 1e-3


def test_ground_is_never_an_edge_and_a_wall_is_never_flat():
    h, c, ref, f = hand("slot_4_picks_index_0")
    rough = f["curvature"][34 * 4 + 5: 34 * 4 + 29]                                    # ring 4: not occlusion-marked there
    assert (rough > np.float32(h["edge"])).sum() >= 20 and not f["occluded"][34 * 4 + 5: 34 * 4 + 29].any()
    assert f["lists"][FR.SHARP].size == 0 and f["lists"][FR.LESS_SHARP].size == 0
    h, c, ref, f = hand("next_sixth_best_kept")
    assert (f["curvature"] < np.float32(h["surf"])).sum() > 500 and f["lists"][FR.FLAT].size == 0


def test_the_slot_4_pick_goes_when_point_0_is_occlusion_marked():
    _, _, _, with_pick = hand("slot_4_picks_index_0")
    _, _, _, without = hand("slot_4_not_when_marked")
    assert with_pick["lists"][FR.FLAT][0] == 0 and with_pick["occluded"][0] == 0
    assert without["occluded"][:6].all() and 0 not in without["lists"][FR.FLAT].tolist() and not without["slot4_pick"]


@pytest.mark.parametrize("name", FC.PARITY)
def test_every_parity_case_is_insensitive_to_ties_and_fragile_decisions(name):
    c, raw, ref, f = FC.case(name)
    print(name, len(f["seg"]["range"]), "segmented,", [len(l) for l in f["lists"]], {k: f[k] for k in REPORT})
    assert ref["n_fragile"] == 0 and f["n_tie_sensitive"] == 0
    assert len(f["lists"][FR.SHARP]) <= 12 * c.V and len(f["lists"][FR.LESS_SHARP]) <= 120 * c.V and len(f["lists"][FR.FLAT]) <= 24 * c.V


def test_the_parity_set_takes_every_path():
    fs = [FC.case(n)[3] for n in FC.PARITY]
    assert sum(f["edge_breaks"] for f in fs) >= 1 and sum(f["flat_breaks"] for f in fs) >= 1
    assert any(f["n_occluded"] > 0 for f in fs) and any(f["ep_picks"] > 0 for f in fs) and any(f["slot4_pick"] for f in fs)
    big = FC.case(FC.BIG)[3]
    assert big["edge_breaks"] >= 10 and big["flat_breaks"] >= 10


def test_output_axes_ring_and_transform():
    h, c, ref, f = hand("next_sixth_best_kept")
    idx = f["lists"][FR.SHARP]
    out = FR.output(f["seg"], idx, FR.identity_T())
    p = f["seg"]["xyz"][idx]
    np.testing.assert_array_equal(out[:, :3], np.stack([p[:, 1], p[:, 2], p[:, 0]], axis=1))       # (y, z, x)
    assert out[:, 3].tolist() == [float(r) for r in range(8, 16) for _ in range(2)]
    T = FR.node_T()
    assert np.allclose(T[:, :3] @ T[:, :3].T, np.eye(3), atol=1e-12) and np.allclose(T[:, 3], 0.0)
    moved = FR.output(f["seg"], idx, T)
    np.testing.assert_allclose(moved[:, :3], out[:, :3].astype(np.float64) @ T[:, :3].T, rtol=0, atol=1e-6)


def test_new_symbols_are_exported_and_laid_out_as_the_header_says():
    lib = K.load_library()
    for s in ("dddmr_rollout_set_lidar_sweep_features", "dddmr_rollout_get_lidar_sweep_segmented", "dddmr_rollout_get_lidar_sweep_features"):
        assert s in K.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(K.LidarFeaturesConfig) == lib.dddmr_rollout_sizeof(20) == 120
    # no context: refused, not crashed
    assert lib.dddmr_rollout_set_lidar_sweep_features(None, 0, None) == K.ERR_BAD_ARG
    assert lib.dddmr_rollout_get_lidar_sweep_features(None, 0, 0, None, None, 0, None) == K.ERR_BAD_ARG
    assert lib.dddmr_rollout_get_lidar_sweep_segmented(None, 0, None, None, None, None, None, None, 0, None) == K.ERR_BAD_ARG


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_struct_offsets_against_the_header():
    fields = [n for n, _ in K.LidarFeaturesConfig._fields_]
    src = "#include <cstddef>\n#include <cstdio>\n#include \"dddmr_rollout.h\"\nint main() { std::printf(\"" + " ".join(["%zu"] * (len(fields) + 1)) + \
          "\\n\", " + ", ".join(f"offsetof(dddmr_lidar_features_config, {n})" for n in fields) + ", sizeof(dddmr_lidar_features_config)); return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "offsets")
        r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-", "-o", exe], input=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [getattr(K.LidarFeaturesConfig, n).offset for n in fields] + [C.sizeof(K.LidarFeaturesConfig)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lidar_features_bridge_against_a_fake_abi_under_sanitizers():
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "lidar_features_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *inc, os.path.join(ROOT, "tests", "cpp", "lidar_features_bridge_test.cpp"),
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "lidar features bridge OK" in r.stdout, (r.stdout, r.stderr)
