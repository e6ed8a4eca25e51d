"""CPU tests of the particle-measure restatement (tests/helpers/mcl_measure_ref.py; what pins it to mcl_3dl's own
measure() compiled from the reference is tests/test_mcl_measure_pin_cpu.py), of the generated cases' input conditions, of the
library's exports and of the ROS-side bridge."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcl_measure_ref as R  # noqa: E402
import mcl_measure_cases as Cs  # noqa: E402

F = np.float32
KNOWN = {name: (cfg, parts, exp) for name, cfg, parts, exp in Cs.known_answers()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_hand_derived_answers(name):
    cfg, parts, exp = KNOWN[name]
    ref = Cs.answer(parts, cfg)
    assert int(ref["n_fragile"].sum()) == 0 and int(ref["n_tied"].sum()) == 0
    for k, v in exp.items():
        want = np.asarray(v, dtype=ref[k].dtype)
        if want.dtype == np.float32:
            np.testing.assert_array_equal(bits(ref[k]), bits(want), err_msg=f"{name}: {k}")
        else:
            np.testing.assert_array_equal(ref[k], want, err_msg=f"{name}: {k}")


def test_the_match_term_by_hand():
    """(0.3 - max(d, 0.05))^2 / intensity at d = 0, 0.04, 0.2 in plain numbers; the edge of the radius is strict"""
    for d, want in ((0.0, 0.25 ** 2 / 1.7), (0.04, 0.25 ** 2 / 1.7), (0.2, 0.1 ** 2 / 1.7)):
        cfg, parts, exp = KNOWN[f"one-point-d{float(F(d)):.9g}"]
        assert abs(float(exp["score"][0]) - want) < 1e-7
    below, at, above = (KNOWN[f"one-point-d{float(v):.9g}"][2] for v in (np.nextafter(F(0.3), F(0)), F(0.3), np.nextafter(F(0.3), F(1))))
    assert below["n_match"] == [1] and 0 <= float(below["score"][0]) < 1e-14 and at["n_match"] == [0] and above["n_match"] == [0]


def test_weight_at_the_edge_of_the_bounded_search():
    """sqrtf(1.0000001f) is 1.0f: the weight there is 0.0 and stays 0.0 (it is not < 0); farther it is 0.01"""
    assert np.sqrt(np.nextafter(F(1), F(2))) == F(1)
    assert np.sqrt(np.nextafter(np.nextafter(F(1), F(2)), F(2))) > F(1)
    assert F(1.0 - float(np.sqrt(R.NN_D2))) < 0                  # everything the bounded search cannot see is negative


def test_transform_is_bit_equal_to_a_second_formulation():
    """The same float32 operations written per scalar (np.float32 arithmetic, one state and one point at a time) instead
    of broadcast arrays, on random raw states"""
    rng = np.random.default_rng(5)
    n = 400
    pos = rng.uniform(-50, 50, (n, 3)).astype(F)
    rot = (rng.normal(size=(n, 4)) * rng.uniform(0.2, 3.0, (n, 1))).astype(F)
    pts = rng.uniform(-30, 30, (7, 3)).astype(F)
    got = R.transform(pos, rot, pts)

    def mul(a, b):
        return (F(F(F(a[3] * b[0]) + F(a[0] * b[3])) + F(a[1] * b[2])) - F(a[2] * b[1]),
                F(F(F(a[3] * b[1]) + F(a[1] * b[3])) + F(a[2] * b[0])) - F(a[0] * b[2]),
                F(F(F(a[3] * b[2]) + F(a[2] * b[3])) + F(a[0] * b[1])) - F(a[1] * b[0]),
                F(F(F(a[3] * b[3]) - F(a[0] * b[0])) - F(a[1] * b[1])) - F(a[2] * b[2]))

    want = np.zeros_like(got)
    for i in range(n):
        x, y, z, w = rot[i]
        norm = np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z)) + F(w * w))
        s = F(1.0 / float(norm))
        r = (F(x * s), F(y * s), F(z * s), F(w * s))
        for j in range(len(pts)):
            b = mul(mul(r, (pts[j, 0], pts[j, 1], pts[j, 2], F(0))), (-r[0], -r[1], -r[2], r[3]))
            want[i, j] = (F(b[0] + pos[i, 0]), F(b[1] + pos[i, 1]), F(b[2] + pos[i, 2]))
    np.testing.assert_array_equal(bits(got), bits(want))
    # and it is a rotation: lengths kept to float accuracy
    moved = got.astype(np.float64) - pos[:, None, :]
    assert np.abs(np.linalg.norm(moved, axis=2) - np.linalg.norm(pts, axis=1)[None, :]).max() < 1e-3


@pytest.mark.parametrize("name", Cs.NAMES)
def test_every_named_case_has_no_fragile_decision_and_no_tie(name):
    parts, ref, draws = Cs.case(name)
    print(f"{name}: {draws} draw(s), {len(parts['states'])} particles, {int(ref['healthy'].sum())} on trusted ground, "
          f"{len(parts['map'])} map / {len(parts['ground'])} ground points, ground neighbours up to {int(ref['n_ground'].max())}")
    assert int(ref["n_fragile"].sum()) == 0 and int(ref["n_tied"].sum()) == 0
    assert len(parts["map"]) <= 20000 and np.isfinite(ref["likelihood"]).all()


def test_the_cases_cover_what_the_device_tests_need():
    sizes = {(len(Cs.case(n)[0]["states"])) for n in Cs.NAMES}
    shapes = {(len(Cs.case(n)[0]["flat"]), len(Cs.case(n)[0]["ls"])) for n in Cs.NAMES}
    assert {1, 64, 65, 300} <= sizes and {(0, 1), (1, 0), (1, 1), (64, 65), (3, 130), (40, 200)} <= shapes
    ref = Cs.case("ground-counts")[1]
    assert ref["n_ground"].tolist() == list(Cs.GROUND_COUNTS)
    room = Cs.case("n300-o64x65")[1]
    w = room["pos_weight"][room["healthy"]]
    assert (~room["healthy"]).sum() >= 5 and (room["pos_weight"] == F(0.01)).sum() >= 3 and len(np.unique(w)) > 100
    assert (Cs.case("needles")[1]["n_match"] == 1).all()
    assert len(Cs.case("map-of-one")[0]["map"]) == 1 and len(Cs.case("map-empty")[0]["map"]) == 0
    # the shifted scene is the same scene: the same branches
    a, b = Cs.case("n65-o40x200")[1], Cs.case("n65-o40x200-shifted")[1]
    assert (a["healthy"] == b["healthy"]).mean() > 0.9


def test_needles_sit_in_every_cell_of_the_query_box():
    """The device's grid, recomputed here in float32: along each axis the needle is in the query's cell or the one next
    to it as its direction says, inside the 2-cell candidate range, and over the 26 particles it takes each of the
    8 cells of the box, the corner opposite the query's among them"""
    parts, ref, _ = Cs.case("needles")
    qc, c0, c1, nc = Cs.needle_cells(parts)
    dirs = np.array(Cs.NEEDLE_DIRS)
    np.testing.assert_array_equal(nc - qc, dirs)
    assert ((c1 - c0) == 1).all() and (c0 >= 0).all()                # 2 x 2 x 2 cells: grid_for_each's fast path
    assert ((nc >= c0) & (nc <= c1)).all() and ((qc >= c0) & (qc <= c1)).all()
    assert {tuple(v) for v in (nc == c1).astype(int).tolist()} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    corner = (np.abs(dirs).sum(axis=1) == 3)
    assert corner.sum() == 8 and ((nc[corner] == c0[corner]) == (qc[corner] == c1[corner])).all() and (nc[corner] != qc[corner]).all()
    assert (ref["n_match"] == 1).all() and (ref["score"] > 0).all()
    # and each match is that needle alone: without it the particle matches nothing
    for i in (0, 12, 25):
        lone = np.delete(parts["map"], parts["needle_of"][i], axis=0)
        assert R.measure(Cs.CFG, lone, parts["ground"], parts["normals"], parts["flat"], parts["ls"], parts["states"][i:i + 1])["n_match"][0] == 0


def test_new_symbols_are_exported_and_laid_out_as_the_header_says():
    lib = K.load_library()
    for s in ("dddmr_rollout_mcl_create", "dddmr_rollout_mcl_set_map", "dddmr_rollout_mcl_measure", "dddmr_rollout_mcl_get_terms"):
        assert s in K.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(K.MclConfig) == lib.dddmr_rollout_sizeof(18) and C.sizeof(K.MclStats) == lib.dddmr_rollout_sizeof(19)
    # no context: refused, not crashed
    assert lib.dddmr_rollout_mcl_create(None, None) == K.ERR_BAD_ARG
    assert lib.dddmr_rollout_mcl_measure(None, None, 0, None, 0, None, 0, None, None, None) == K.ERR_BAD_ARG


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_localization_bridge_against_a_fake_abi_under_sanitizers():
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "localization_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *inc, os.path.join(ROOT, "tests", "cpp", "localization_bridge_test.cpp"),
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "localization bridge OK" in r.stdout, (r.stdout, r.stderr)
