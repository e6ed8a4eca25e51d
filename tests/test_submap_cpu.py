"""CPU tests of the sub-maps' restatement (tests/helpers/submap_ref.py, UNPINNED: PCL and FLANN cannot be built here), of
the conditions the GPU tests rely on, of the host-callable header csrc/mcl_submap_plan.hip.h against the restatement,
and of the ABI's new symbols."""
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
import capi_header  # noqa: E402
import submap_ref as S  # noqa: E402
import submap_cases as Cs  # noqa: E402

F = np.float32
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
ENTRIES = ("create", "add_keyframe", "select", "warm_up", "swap", "get")


# ---- known answers ---------------------------------------------------------------------------------------------------

def test_neighbours_of_a_lattice_point_by_hand():
    # 5 x 5 lattice, 1 m, index = 5 * ix + iy; the centre is 12.  d2 0: itself; 1: 7 11 13 17; 2: 6 8 16 18; 4: 2 10 14 22
    g = np.array([[ix, iy, 0.0] for ix in range(5) for iy in range(5)], F)
    nb = S.neighbours(g, 13)
    assert nb[12].tolist() == [12, 7, 11, 13, 17, 6, 8, 16, 18, 2, 10, 14, 22]
    # the corner 0: d2 0 | 1: 1 5 | 2: 6 | 4: 2 10 | 5: 7 11 | 8: 12 | 9: 3 15 | 10: 8 16
    assert nb[0].tolist() == [0, 1, 5, 6, 2, 10, 7, 11, 12, 3, 15, 8, 16]
    # fewer points than k: all of them, -1 padded; exact duplicates tie by index
    few = S.neighbours(np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], F), 5)
    assert few.tolist() == [[0, 2, 1, -1, -1], [1, 0, 2, -1, -1], [0, 2, 1, -1, -1]]


def test_normal_of_an_exact_plane():
    # z = 0.5 x + 0.25 y + 1 on dyadic coordinates: every product is exact in float; the normal is (-0.5, -0.25, 1) / |.|,
    # flipped toward the origin (the plane lies above it: the normal points down)
    g = np.array([[x, y, 0.5 * x + 0.25 * y + 1.0] for x in (0.0, 0.5, 1.0, 1.5) for y in (0.0, 0.5, 1.0, 1.5, 2.0)], F)
    nb = S.neighbours(g, 20)
    n32, n64 = S.normals(g, nb), S.normals_f64(g, nb)
    want = np.array([0.5, 0.25, -1.0]) / np.linalg.norm([0.5, 0.25, 1.0])
    assert S.defined(g, nb).all()
    assert np.abs(n32.astype(np.float64) - want).max() < 2e-6
    assert S.R.angle(n32, n64).max() < 2e-6
    # fewer than 3 neighbours: NaN; collinear points: not defined by the data
    two = np.array([[0, 0, 0], [1, 0, 0]], F)
    assert np.isnan(S.normals(two, S.neighbours(two, 20))).all()
    line = np.array([[i * 0.25, 0, 0] for i in range(8)], F)
    assert not S.defined(line, S.neighbours(line, 20)).any()


def test_select_on_hand_placed_keyframes():
    kf = np.array([[49.999, 0, 0], [50.001, 0, 0], [0, -49.999, 0], [0, 0, 50.001], [30, 40, 0.4], [30, 39.99, -0.3], [0, 0, 0], [-35.4, -35.3, 0.0]])
    ids, d2 = S.select(kf, (0, 0, 0), 50.0)
    assert ids.tolist() == [0, 2, 5, 6, 7]           # 30 40 0.4: 50.0016 m; 30 39.99 -0.3: 49.9929 m
    far = np.sqrt(d2.astype(np.float64))
    assert (np.abs(far - 50.0) >= 0.8e-3).all()
    ids, _ = S.select(kf + np.array([1000.0, -2000.0, 5.0]), (1000.0, -2000.0, 5.0), 50.0)
    assert ids.tolist()[:2] == [0, 2] and 1 not in ids.tolist() and 3 not in ids.tolist()
    assert S.select(np.zeros((0, 3)), (0, 0, 0), 50.0)[0].tolist() == []


def test_concatenation_is_in_list_order_with_the_transform():
    kfs, ids, ref = Cs.case("j")
    parts = [S.stored(kfs[i]) for i in ids]
    assert ref["map"].tobytes() == np.concatenate([p[0] for p in parts]).tobytes()
    assert ref["ground"].tobytes() == np.concatenate([p[1] for p in parts]).tobytes()
    k = kfs[ids[0]]
    x = k["ground"][5].astype(np.float64)
    want = [F(((k["T"][r, 0] * x[0] + k["T"][r, 1] * x[1]) + k["T"][r, 2] * x[2]) + k["T"][r, 3]) for r in range(3)]
    assert ref["ground"][5].tolist() == want


# ---- the cases' own conditions -----------------------------------------------------------------------------------------

def test_the_cases_are_what_their_names_say():
    for name in Cs.NAMES:
        kfs, ids, ref = Cs.case(name)
        g = ref["ground"]
        assert 2 <= len(kfs) <= 6 and sorted(ids) == list(range(len(kfs))), name
        if name.startswith("h-"):
            assert len(g) == int(name[2:]), name
            continue
        assert all(len(k["ground"]) == 0 or 50 <= len(k["ground"]) <= 800 for k in kfs), name
        assert 300 <= len(g) <= 2000, name
    # d: equal d2 across the k-th place, so that the index decides; e: exact duplicates
    g, nb = Cs.case("d")[2]["ground"], Cs.case("d")[2]["neighbours"]
    d2 = S.R.l2_matrix(g[:200])
    tied = sum(int((np.sort(d2[i])[19] == np.sort(d2[i])[20])) for i in range(200))
    assert tied > 100
    g, nb = Cs.case("e")[2]["ground"], Cs.case("e")[2]["neighbours"]
    dup = (g[nb[:, 0]] == g[nb[:, 1]]).all(axis=1)
    assert dup.sum() >= 2 * 18 * 18 and (nb[dup, 0] < nb[dup, 1]).all()
    # f: the two lone points are tens of metres from every other
    g = Cs.case("f")[2]["ground"]
    lone = np.nonzero(g[:, 0] > 30.0)[0]
    d = np.linalg.norm(g[:, None, :].astype(np.float64) - g[None, lone, :].astype(np.float64), axis=2)
    d[lone, np.arange(len(lone))] = np.inf
    assert len(lone) == 2 and d[:, 0].min() > 25.0 and d[:, 1].min() > 300.0
    # g: kilometres from the origin; i: an empty ground and an empty corner cloud; j: all three angles
    assert np.abs(Cs.case("g")[2]["ground"]).max() > 5000
    kfs = Cs.case("i")[0]
    assert any(len(k["ground"]) == 0 and len(k["corner"]) for k in kfs) and any(len(k["corner"]) == 0 and len(k["ground"]) for k in kfs)
    for k in Cs.case("j")[0]:
        Rm = k["T"][:, :3]
        assert abs(Rm[2, 0]) > 0.03 and abs(Rm[2, 1]) > 0.03 and abs(Rm[1, 0]) > 0.3          # pitch, roll, yaw


def test_the_restatement_stays_within_the_excluded_cap():
    """Prints the restatement's own error per case (what the GPU test doubles) and holds the excluded share of the smooth
    cases under the cap; GAP_FACTOR and RANK_FLOOR (submap_ref.py) say which points are not compared."""
    assert S.GAP_FACTOR == 4.0 and S.RANK_FLOOR == 1e-9
    compared = excluded = 0
    for name in Cs.NAMES:
        err, n_cmp, n_exc, n_nan = Cs.restatement_error(name)
        print(f"{name}: restatement to float64 at most {err:.3e} rad over {n_cmp} points; {n_exc} not defined, {n_nan} NaN")
        assert np.isfinite(err) and err < 0.05, name
        if name in Cs.SMOOTH:
            compared, excluded = compared + n_cmp, excluded + n_exc
    assert compared > 5000 and excluded <= Cs.EXCLUDED_CAP * (compared + excluded), (compared, excluded)
    # below 3 points every normal is NaN, from 3 on none is (the jittered points are never collinear to the last bit)
    for n in Cs.H_TOTALS:
        nan = np.isnan(Cs.case(f"h-{n}")[2]["normals"][:, 0])
        assert nan.all() if n < 3 else not nan.any(), n


def test_select_cases_keep_away_from_the_sphere():
    for seed in (1, 2, 3):
        k, q, r = Cs.select_case(seed)
        ids, d2 = S.select(k, q, r)
        assert 5 < len(ids) < len(k) - 5 and (np.diff(ids) > 0).all()
        assert (np.abs(np.sqrt(d2.astype(np.float64)) - r) >= 0.9e-3).all()


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_capi_exposes_the_new_entries():
    protos = capi_header.prototypes()
    for e in ENTRIES:
        name = "dddmr_rollout_submap_" + e
        assert name in K.SIGNATURES and name in K.EXPORTED_SYMBOLS and name in protos, name
        ret, params = protos[name]
        sig = K.SIGNATURES[name]
        assert capi_header.ctypes_kind(sig[0], True) == ret and len(sig[1]) == len(params), name
        for t, kind in zip(sig[1], params):
            got = capi_header.ctypes_kind(t)
            assert got == ("ptr" if kind in ("in", "out") else kind), (name, got, kind)
    import ctypes as C
    assert C.sizeof(K.SubmapConfig) == 24 and C.sizeof(K.SubmapStats) == 32
    # (the compiled side: static_asserts on the same two sizes in csrc/mcl_submap.hip.h)
    from dddmr_navigation_amd import submaps
    assert submaps.shipped_config().normal_k == 20
    assert [m for m in ("add_keyframe", "select", "warm_up", "swap", "get", "close") if not hasattr(submaps.SubMaps, m)] == []


# ---- the host-callable header against the restatement --------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan_exe():
    if CXX is None:
        pytest.skip("needs a host C++ compiler")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "submap_plan_test")
        r = subprocess.run([CXX, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                            os.path.join(ROOT, "tests", "cpp", "submap_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        yield exe


def ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def test_plan_header_selects_like_the_restatement(plan_exe):
    lines, want = [], []
    for seed in (1, 2, 3):
        k, q, r = Cs.select_case(seed)
        lines.append(f"S {r!r} " + " ".join(repr(float(v)) for v in q) + f" {len(k)} " + " ".join(repr(float(v)) for v in k.astype(F).ravel()))
        ids, _ = S.select(k, q, r)
        want.append(f"S {len(ids)}" + "".join(f" {i}" for i in ids))
    assert ask(plan_exe, lines) == want


def test_plan_header_transforms_like_the_restatement(plan_exe):
    kfs, _, _ = Cs.case("j")
    lines, want = [], []
    for k in kfs:
        g = k["ground"][:40]
        lines.append("T " + " ".join(repr(float(v)) for v in k["T"].ravel()) + f" {len(g)} " + " ".join(repr(float(v)) for v in g.ravel()))
        want.append("T" + "".join(f" {int(b):08x}" for b in S.R.transform(g, k["T"]).view(np.uint32).ravel()))
    assert ask(plan_exe, lines) == want
