"""CPU tests of the observation's restatement (tests/helpers/mcl_observation_ref.py, UNPINNED: PCL cannot be built here),
of the conditions the GPU tests rely on, of the host-callable header csrc/mcl_observation_plan.hip.h against the
restatement, and of the ABI's new symbols."""
import ctypes as C
import math
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
import mcl_observation_ref as R  # noqa: E402
import mcl_observation_cases as Cs  # noqa: E402

F = np.float32
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


# ---- known answers ---------------------------------------------------------------------------------------------------

def test_voxel_grid_by_hand():
    # leaf (1, 1, 0.1): voxels by floor(x), floor(y), floor(z * 10f); min_b = (-1, 0, 0), dx = 3, dy = 2
    pts = np.array([[1.5, 0.5, 0.05],      # voxel (2, 0, 0) -> index 2
                    [-0.5, 0.5, 0.05],     # voxel (0, 0, 0) -> index 0
                    [-0.25, 0.25, 0.025],  # voxel (0, 0, 0) -> index 0
                    [0.5, 1.5, 0.05],      # voxel (1, 1, 0) -> index 4
                    [-0.5, 0.5, 0.15]],    # voxel (0, 0, 1) -> index 6
                   F)
    out = R.voxel_grid(pts)
    want = np.array([[-0.375, 0.375, F(F(0.05) + F(0.025)) / F(2)], [1.5, 0.5, 0.05], [0.5, 1.5, 0.05], [-0.5, 0.5, 0.15]], F)
    assert out.tobytes() == want.tobytes()
    assert len(R.voxel_grid(np.zeros((0, 3), F))) == 0


def test_normal_of_an_exact_plane():
    # z = 0.5 x on a lattice of exactly representable coordinates: the normal is (-1, 0, 2) / sqrt(5) up to the sign
    g = np.arange(-2.0, 2.01, 0.5)
    x, y = np.meshgrid(g, g)
    p = np.stack([x.ravel(), y.ravel() + 4.0, 0.5 * x.ravel() + 3.0], axis=1).astype(F)
    nrm = R.normals(p, R.neighbours(p))
    want = np.array([-1.0, 0.0, 2.0]) / math.sqrt(5.0)
    ang = R.angle(nrm, np.broadcast_to(want, nrm.shape))
    assert not np.isnan(nrm).any() and ang.max() < 1e-3, ang.max()
    # flipped toward the origin: the points are above the plane through the origin with this normal
    assert (np.sum(nrm.astype(np.float64) * -p, axis=1) >= 0).all()
    # fewer than three points: NaN normals, 0 / 0, the cluster branch, and nothing kept below the minimum of 3
    ref = R.prepare(np.zeros((0, 3), F), p[:2], IDENT)
    assert np.isnan(ref["normals"]).all() and ref["branch"] == R.CLUSTERS and len(ref["ls"]) == 0 and ref["n_nan_normals"] == 2
    assert R.prepare(np.zeros((0, 3), F), np.zeros((0, 3), F), IDENT)["branch"] == R.CLUSTERS


def hand_clusters():
    """groups of 1, 2, 3, 3, 4, 4 points 5 m apart, points of a group 0.5 m apart along z, in creation order
    a(1) b(2) c(3) d(3) e(4) f(4); on the plane x + y = 0, so that the sums tie and the cluster branch is taken"""
    sizes = (1, 2, 3, 3, 4, 4)
    pts = [[5.0 * g, -5.0 * g, 0.5 * k] for g, s in enumerate(sizes) for k in range(s)]
    return np.array(pts, F), sizes


def test_cluster_order_and_intensities_by_hand():
    p, sizes = hand_clusters()
    out, n_kept, n_small = R.clusters_output(p, 0.8, 3)
    # kept, creation order: c(3) d(3) e(4) f(4).  std::sort over the reverse iterators is an insertion sort of [f e d c]
    # ascending by size, which is stable: [d c f e]; read back through the reverse iterators: e f c d
    assert (n_kept, n_small) == (4, 2)
    first = {g: sum(sizes[:g]) for g in range(6)}
    want_groups = [4, 5, 2, 3]
    want_idx = [first[g] + k for g in want_groups for k in range(sizes[g])]
    assert out[:, :3].tobytes() == p[want_idx].tobytes()
    n = float(len(p))
    want_w = [F(4 / n)] * 8 + [F(3 / n / 2.0)] * 6           # size < min_size + 1: halved
    assert out[:, 3].tobytes() == np.array(want_w, F).tobytes()
    # the six intensities a group would get if it were kept, written out for N = 17
    assert [float(R.cluster_intensity(s, 17, 3)) for s in sizes] == [float(F(v)) for v in (1 / 34, 2 / 34, 3 / 34, 3 / 34, 4 / 17, 4 / 17)]
    # with min_size 1 all six are kept: [f e d c b a] sorted ascending and stable is [a b d c f e]; read back: e f c d b a
    out1, k1, s1 = R.clusters_output(p, 0.8, 1)
    assert (k1, s1) == (6, 1)
    idx1 = [first[g] + k for g in (4, 5, 2, 3, 1, 0) for k in range(sizes[g])]
    assert out1[:, :3].tobytes() == p[idx1].tobytes()
    # the whole function takes the cluster branch here: every point lies on the plane x + y = 0, so |normal_x| = |normal_y|
    ref = R.prepare(np.zeros((0, 3), F), p, IDENT, 0.8, 3)
    assert ref["branch"] == R.CLUSTERS and ref["ls"].tobytes() == out.tobytes()


def test_std_sort_replay_matches_sorted_on_distinct_keys():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 16, 17, 40, 300, 2000):
        keys = rng.permutation(n).tolist()
        order = R.cluster_order(keys)
        assert [keys[c] for c in order] == sorted(keys, reverse=True)
    # equal keys: still a permutation, descending
    keys = rng.integers(3, 6, 500).tolist()
    order = R.cluster_order(keys)
    assert sorted(order) == list(range(500)) and [keys[c] for c in order] == sorted(keys, reverse=True)


def test_dominance_rule():
    assert R.branch_of(1.6, 1.0) == R.X_DOMINANT and R.branch_of(1.0, 1.6) == R.Y_DOMINANT and R.branch_of(1.59, 1.0) == R.CLUSTERS
    assert R.branch_of(0.0, 0.0) == R.CLUSTERS                      # 0 / 0 is NaN: neither
    assert R.branch_of(1.0, 0.0) == R.X_DOMINANT and R.branch_of(0.0, 1.0) == R.Y_DOMINANT      # x / 0 is inf
    nrm = np.array([[0.8, 0.6, 0], [0.9, 0.1, 0], [np.nan, np.nan, np.nan], [-0.8, -0.6, 0], [0.8, -0.6, 0]], F)
    w = R.dominant_intensity(R.X_DOMINANT, nrm, 4.0, 1.0)
    low = F(0.05 * 1.0 / 4.0)
    assert w.tolist() == [low, 1.0, 1.0, low, 1.0]


# ---- the conditions the GPU tests rely on --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", Cs.NAMES)
def test_case_conditions(name):
    ls, ref, draws = Cs.case(name)
    assert Cs.condition(name, ref)
    if name in Cs.DOMINANT:
        q = Cs.ratio(ref)
        assert q >= 3.0 or q <= 1 / 3.0
        assert ref["branch"] == (R.Y_DOMINANT if name == "y-walls" else R.X_DOMINANT)
        assert (np.abs(ref["ratio"].astype(np.float64) - 0.5) < Cs.NEAR_HALF).mean() <= 0.02
        assert len(ref["ls"]) == len(ls)
    else:
        assert ref["branch"] == R.CLUSTERS
        if len(ls) >= 3:
            assert 0.8 <= Cs.ratio(ref) <= 1.25


def test_island_cases_have_the_ties():
    for name in ("islands", "islands-600", "islands-1900"):
        ls, ref, _ = Cs.case(name)
        sizes = [len(c) for c in R.euclidean_clusters(ref["pts"], Cs.TOL)]
        assert sizes.count(3) >= 20 and sizes.count(4) >= 10 and sizes.count(1) >= 5 and sizes.count(2) >= 5
        assert ref["n_small_clusters"] == sizes.count(3) and len(ref["ls"]) == len(ls) - sizes.count(1) - 2 * sizes.count(2)
        # the replayed order is not the stable one: the tie order decides the output
        kept = [s for s in sizes if s >= Cs.MIN_SIZE]
        stable = sorted(range(len(kept)), key=lambda c: -kept[c])
        assert R.cluster_order(kept) != stable


def test_normal_bound_a_ref():
    a = Cs.a_ref()
    print(f"a_ref = {a:.6g} rad")
    assert 0.0 < a < 0.1                                            # (DESIGN.md 4e records the figure)


def test_flat_cases_are_what_they_say():
    for n in Cs.FLAT_COUNTS:
        f, out = Cs.flat_case(n)
        assert len(f) == n and len(out) == (1 if n == 2 else len(out)) and len(out) <= n
    f, _ = Cs.flat_case(384)
    p = R.transform(f, Cs.T_B2S)
    assert (p[:, :2] < 0).any()
    assert np.isin(p[:, 2], np.array([-0.1, 0.0, 0.1, 0.2], F)).sum() >= 20        # z exactly on a voxel boundary, after the transform


# ---- the host-callable header against the restatement --------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan_exe():
    if CXX is None:
        pytest.skip("needs a host C++ compiler")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mcl_observation_plan_test")
        r = subprocess.run([CXX, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                            os.path.join(ROOT, "tests", "cpp", "mcl_observation_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        yield exe


def ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def test_plan_header_orders_and_weighs_like_the_restatement(plan_exe):
    lines, want = [], []
    rng = np.random.default_rng(11)
    sets = []
    for name in ("islands", "islands-600", "islands-1900"):
        _, ref, _ = Cs.case(name)
        n = len(ref["pts"])
        sets.append(([len(c) for c in R.euclidean_clusters(ref["pts"], Cs.TOL) if len(c) >= Cs.MIN_SIZE], n, Cs.MIN_SIZE))
    sets.append(([3, 3, 4, 4], 17, 3))
    sets.append((rng.integers(1, 4, 1000).tolist(), 2000, 1))      # many equal keys, past the insertion-sort threshold
    sets.append(([], 5, 3))
    for sizes, n, mn in sets:
        lines.append(f"C {mn} {n} {len(sizes)} " + " ".join(map(str, sizes)))
        order = R.cluster_order(sizes)
        want.append("C" + "".join(f" {c}" for c in order) + " |" + "".join(f" {int(np.array(R.cluster_intensity(sizes[c], n, mn), F).view(np.uint32)):08x}" for c in order))
    got = ask(plan_exe, lines)
    assert got == want


def test_plan_header_dominance_like_the_restatement(plan_exe):
    rows = [(4.0, 1.0, 0.8, 0.6), (4.0, 1.0, 0.9, 0.1), (4.0, 1.0, float("nan"), 0.3), (1.0, 4.0, 0.6, 0.8), (1.0, 4.0, 0.1, 0.9),
            (1.0, 1.0, 0.5, 0.5), (0.0, 0.0, 0.5, 0.5), (2.0, 0.0, 1.0, 0.0), (0.0, 2.0, 0.0, 1.0), (1.6, 1.0, 0.6, 0.3), (1.0, 1.6, 0.3, 0.6),
            (37.25, 4.125, -0.8, -0.6)]
    lines = [f"D {float(sx).hex()} {float(sy).hex()} {nx!r} {ny!r}" for sx, sy, nx, ny in rows]
    got = ask(plan_exe, lines)
    for (sx, sy, nx, ny), line in zip(rows, got):
        br = R.branch_of(sx, sy)
        w = 0 if br == R.CLUSTERS else int(R.dominant_intensity(br, np.array([[nx, ny, 0]], F), sx, sy).view(np.uint32)[0])
        assert line == f"D {br} {w:08x}", (sx, sy, nx, ny, line)


# ---- the ABI ----------------------------------------------------------------------------------------------------------

def test_capi_exposes_the_observation_entries():
    lib = K.load_library()
    for s in ("dddmr_rollout_mcl_set_observation_config", "dddmr_rollout_mcl_prepare", "dddmr_rollout_mcl_prepare_from_sweep",
              "dddmr_rollout_mcl_get_observation", "dddmr_rollout_mcl_measure_prepared"):
        assert s in K.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(K.MclObservationConfig) == lib.dddmr_rollout_sizeof(21) == 32
    assert C.sizeof(K.MclObservationStats) == lib.dddmr_rollout_sizeof(22) == 56
    assert lib.dddmr_rollout_mcl_prepare(None, None, 0, 0, None, 0, 0, None, None) == K.ERR_BAD_ARG
