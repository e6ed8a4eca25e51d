"""CPU tests of the static layer's restatement (tests/helpers/static_layer_ref.py): the cKDTree version against the
all-pairs NumPy version on every case, a hand-computed case, the adaptive radius table as bit patterns, the conditions
the GPU tests' floor case has to hold, and the new structs' ctypes sizes against the sizes the header's static_assert
pins.  Needs no GPU; the tests that use the cKDTree version skip without SciPy."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import static_layer_ref as R  # noqa: E402
import static_layer_cases as Cs  # noqa: E402

F = np.float32
SQRT2 = 0x3FB504F3           # sqrtf(2.0f)

# float(r_k * r_k) for r_k = double(0.5f) + 0.2 * k, k = 1 .. 101
R2_BITS = (
    0x3EFAE148, 0x3F4F5C29, 0x3F9AE148, 0x3FD851EC, 0x40100000, 0x4038F5C3, 0x40670A3D, 0x408D1EB8, 0x40A947AE, 0x40C80000,
    0x40E947AE, 0x41068F5C, 0x4119C28F, 0x412E3D71, 0x41440000, 0x415B0A3D, 0x41735C29, 0x41867AE1, 0x4193EB85, 0x41A20000,
    0x41B0B852, 0x41C0147B, 0x41D0147B, 0x41E0B852, 0x41F20000, 0x4201F5C3, 0x420B3D71, 0x4214D70A, 0x421EC28F, 0x42290000,
    0x42338F5C, 0x423E70A4, 0x4249A3D7, 0x425528F6, 0x42610000, 0x426D28F6, 0x4279A3D7, 0x42833852, 0x4289C7AE, 0x42908000,
    0x42976148, 0x429E6B85, 0x42A59EB8, 0x42ACFAE1, 0x42B48000, 0x42BC2E14, 0x42C4051F, 0x42CC051F, 0x42D42E14, 0x42DC8000,
    0x42E4FAE1, 0x42ED9EB8, 0x42F66B85, 0x42FF6148, 0x43044000, 0x4308E3D7, 0x430D9C29, 0x431268F6, 0x43174A3D, 0x431C4000,
    0x43214A3D, 0x432668F6, 0x432B9C29, 0x4330E3D7, 0x43364000, 0x433BB0A4, 0x434135C3, 0x4346CF5C, 0x434C7D71, 0x43524000,
    0x4358170A, 0x435E028F, 0x4364028F, 0x436A170A, 0x43704000, 0x43767D71, 0x437CCF5C, 0x43819AE1, 0x4384D852, 0x43882000,
    0x438B71EC, 0x438ECE14, 0x4392347B, 0x4395A51F, 0x43992000, 0x439CA51F, 0x43A0347B, 0x43A3CE14, 0x43A771EC, 0x43AB2000,
    0x43AED852, 0x43B29AE1, 0x43B667AE, 0x43BA3EB8, 0x43BE2000, 0x43C20B85, 0x43C60148, 0x43CA0148, 0x43CE0B85, 0x43D22000,
    0x43D63EB8,
)


def same(a, b, what=""):
    for k in ("row_start", "neighbour", "kidx", "counts", "qualifying", "overhang", "near"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(a["weight"].view(np.uint32), b["weight"].view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(a["dgraph"].view(np.uint64), b["dgraph"].view(np.uint64), err_msg=what)


def test_adaptive_radius_table():
    tab = R.adaptive_r2_table()
    assert len(tab) == 102 and len(R2_BITS) == R.ADAPTIVE_STEPS == 101
    assert tab[1:].view(np.uint32).tolist() == list(R2_BITS)
    assert (np.diff(tab[1:]) > 0).all()                    # the device's search for the first k relies on it
    assert R.adaptive_radius(1) == 0.7 and abs(R.adaptive_radius(101) - 20.7) < 1e-12


# ---- the hand-computed case: 6 ground points on a unit lattice (radius 1.5: r2 = 2.25, so distance 1 and sqrt 2 connect and
# 2 does not), 11 map points half a metre above node 1 inside its 1 m x 1 m window (limits included), one 0.375 m from node 4
HAND_GROUND = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0], [10, 10, 0]], F)
HAND_MAP = np.array([[0.5, -0.5, 0.5], [0.75, -0.25, 0.5], [1, 0, 0.5], [1.25, 0.25, 0.5], [1.5, 0.5, 0.5], [0.5, 0.5, 0.5], [1.5, -0.5, 0.5],
                     [1, 0.5, 0.5], [1, -0.5, 0.5], [0.5, 0, 0.5], [1.5, 0, 0.5], [2.375, 0, 0]], F)
HAND_ROW_START = [0, 4, 9, 13, 18, 21, 22]
HAND_NEIGHBOUR = [0, 1, 2, 3, 0, 1, 2, 3, 4, 0, 1, 2, 3, 0, 1, 2, 3, 4, 1, 3, 4, 5]
ONE = 0x3F800000
HAND_WEIGHT = [0, ONE, ONE, SQRT2, ONE, 0, SQRT2, ONE, ONE, ONE, SQRT2, 0, ONE, SQRT2, ONE, ONE, 0, SQRT2, ONE, SQRT2, 0, 0]
# node 1: five neighbours and 11 points in its window -> 0.25; node 3 has five neighbours but 3 points; node 0's window holds
# 3 and it has four neighbours; node 1's nearest obstacle is exactly 0.5 away: not below inscribed_radius; node 4's is 0.375
HAND_DGRAPH = [9999.0, 0.25, 9999.0, 9999.0, 0.375, 9999.0, 9999.0]


def check_hand(r):
    assert r["row_start"].tolist() == HAND_ROW_START and r["neighbour"].tolist() == HAND_NEIGHBOUR
    assert r["weight"].view(np.uint32).tolist() == HAND_WEIGHT
    assert r["dgraph"].tolist() == HAND_DGRAPH
    assert r["overhang"].tolist() == [False, True, False, False, False, False]
    assert r["near"].tolist() == [False, False, False, False, True, False]
    assert r["qualifying"].tolist() == [3, 11, 1, 3, 3, 0] and r["counts"].tolist() == [4, 5, 4, 5, 3, 1]


def test_hand_computed_case_all_pairs():
    check_hand(R.build_all_pairs(HAND_GROUND, HAND_MAP, R.config()))
    off = R.build_all_pairs(HAND_GROUND, HAND_MAP, R.config(generate_static_graph=0))
    assert off["row_start"].tolist() == [0] * 7 and off["dgraph"].tolist() == [9999.0, 0.25] + [9999.0] * 5
    off = R.build_all_pairs(HAND_GROUND, HAND_MAP, R.config(enable_edge_detection=0))
    assert off["dgraph"].tolist() == [9999.0] * 4 + [0.375, 9999.0, 9999.0] and off["neighbour"].tolist() == HAND_NEIGHBOUR
    # adaptive, number 4: node 1 reaches four points at r_3 = 1.1 (1.21 > 1); nodes 0, 2 and 3 need the diagonal, r_5 = 1.5
    # (2.25 > 2); node 4 needs node 0 at distance 2, r_8 = 2.1; node 5 has itself, node 3
    # (d2 162) and node 4 (164); nodes 1 and 2 (181, 13.45 m) come together at r_65 = 13.5 and make five
    ad = R.build_all_pairs(HAND_GROUND, HAND_MAP, R.config(use_adaptive_connection=1, adaptive_connection_number=4))
    assert R.build_all_pairs(HAND_GROUND, HAND_MAP, R.config(use_adaptive_connection=1, adaptive_connection_number=7))["kidx"].tolist() == [101] * 6
    assert ad["kidx"].tolist() == [5, 3, 5, 5, 8, 65] and ad["counts"].tolist() == [4, 4, 4, 5, 4, 5]


def test_hand_computed_case_tree():
    pytest.importorskip("scipy")
    check_hand(R.build(HAND_GROUND, HAND_MAP, R.config()))


@pytest.mark.parametrize("name", ("floor", "floor_adaptive", "floor_shifted", "long_row", "n_ground_1", "empty_map", "graph_off", "edge_off"))
def test_restatement_equals_all_pairs(name):
    pytest.importorskip("scipy")
    c = Cs.all_cases()[name]
    same(Cs.reference(name), R.build_all_pairs(c["ground"], c["map"], c["cfg"]), name)


def test_floor_case_holds_what_the_gpu_tests_claim():
    pytest.importorskip("scipy")
    found = Cs.check_floor()
    assert found["k101"] == 3 and found["few_neighbours"] == 3 and found["coincident"] == 2
    # the long-row case: rows longer than the budget the header names
    deg = np.diff(Cs.reference("long_row")["row_start"].astype(np.int64))
    assert Cs.row_lds() == 512 and int((deg > Cs.row_lds()).sum()) >= 1
    # the shifted floor is the same floor: its graph differs from the unshifted one by a few edges at most (rounding)
    assert abs(len(Cs.reference("floor_shifted")["neighbour"]) - len(Cs.reference("floor")["neighbour"])) < 50


def test_zones_restatement_equals_all_pairs():
    pytest.importorskip("scipy")
    g = Cs.floor()["ground"]
    a, b = Cs.zone_sets()
    for pts in (np.concatenate([a, b]), a, b, b[-1:], np.zeros((0, 3), F)):
        x, y = R.zones(g, pts, Cs.INFLATION, 9999.0), R.zones_all_pairs(g, pts, Cs.INFLATION, 9999.0)
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
    far = R.zones(g, b[-1:], Cs.INFLATION, 9999.0)
    assert (far == 9999.0).all()                            # farther than the inflation distance from every node
    hand = R.zones_all_pairs(HAND_GROUND, np.array([[1, 0.5, 0], [2.25, 0, 0]], F), 0.6, 50.0)
    assert hand.tolist() == [50.0, 0.5, 50.0, 0.5, 0.25, 50.0, 50.0]


def test_struct_sizes_match_the_header_static_assert():
    text = open(os.path.join(ROOT, "dddmr_navigation_amd", "csrc", "static_layer.hip.h")).read()
    m = re.search(r"static_assert\(sizeof\(dddmr_static_layer_config\) == (\d+) && sizeof\(dddmr_static_layer_stats\) == (\d+)", text)
    assert m, "static_layer.hip.h no longer pins the two struct sizes"
    assert C.sizeof(K.StaticLayerConfig) == int(m.group(1)) and C.sizeof(K.StaticLayerStats) == int(m.group(2))
    assert len(K.SIZEOF_STRUCTS) == 23                      # dddmr_rollout_sizeof's table is not extended
    # the fields, in the header's order
    head = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    for cls, name in ((K.StaticLayerConfig, "dddmr_static_layer_config"), (K.StaticLayerStats, "dddmr_static_layer_stats")):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", head).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in cls._fields_], name

