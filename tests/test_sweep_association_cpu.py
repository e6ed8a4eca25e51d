"""CPU tests of the lidar sweep association's restatement (tests/helpers/sweep_association_ref.py) and of the conditions its
cases (tests/helpers/sweep_association_cases.py) must meet; needs no GPU.

  1. the restatement against a plain serial transcription of the reference's loops (adjustDistortion's halfPassed walk,
     extractFeatures with the cloudLabel writes and the less-flat loop where the reference has them, the outlier branch of
     cloudSegmentation) on every case;
  2. hand-computed answers: one sweep's orientation and point times, one ring's candidates and voxels;
  3. the VoxelGrid part against mcl_observation_ref's on the same points;
  4. the margins and shapes the GPU test relies on, for every committed case;
  5. the public surface: the header's entries, the Python class."""
import inspect
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lidar_features_ref as FR  # noqa: E402
import lidar_sweep_ref as R  # noqa: E402
import mcl_observation_ref as OR  # noqa: E402
import sweep_association_cases as AC  # noqa: E402
import sweep_association_ref as AR  # noqa: E402

f32, f64 = np.float32, np.float64
PI = math.pi


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- 1. the reference's loops, transcribed ---------------------------------------------------------------------------------
def serial_times(seg, start, end, diff, scan_period):
    """featureAssociation.cpp:281-314, line for line"""
    half_passed = False
    out, i0 = [], len(seg["range"])
    base = AR.atan2f(seg["xyz"][:, 1], seg["xyz"][:, 0])
    for i in range(len(base)):
        ori = f32(-base[i])
        if not half_passed:
            if f64(ori) < f64(start) - PI / 2:
                ori = f32(f64(ori) + 2 * PI)
            elif f64(ori) > f64(start) + PI * 3 / 2:
                ori = f32(f64(ori) - 2 * PI)
            if f64(f32(ori - start)) > PI:
                half_passed = True
                i0 = i
        else:
            ori = f32(f64(ori) + 2 * PI)
            if f64(ori) < f64(end) - PI * 3 / 2:
                ori = f32(f64(ori) + 2 * PI)
            elif f64(ori) > f64(end) + PI / 2:
                ori = f32(f64(ori) - 2 * PI)
        rel = f32(f32(ori - start) / diff)
        out.append(f32(f64(int(seg["row"][i])) + f64(scan_period) * f64(rel)))
    return np.asarray(out, f32), i0


def serial_less_flat(seg, curv, picked0, edge_threshold, surf_threshold, V):
    """featureAssociation.cpp:381-491 with cloudLabel written where the reference writes it and the loop of :486-490 at the
    end of each sixth: per ring the candidates' segment indices"""
    edge, surf = float(f32(edge_threshold)), float(f32(surf_threshold))
    n = len(curv)
    col, ground = seg["col"].tolist(), seg["ground"].tolist()
    curvature = [float(v) for v in curv]
    picked = list(picked0)
    label = [0] * max(n, 5)
    sm = [(curvature[i], i) if 5 <= i < n - 5 else (0.0, 0) for i in range(max(n, 5))]

    def suppress(ind):
        picked[ind] = 1
        for l in range(1, 6):
            if abs(col[ind + l] - col[ind + l - 1]) > 10:
                break
            picked[ind + l] = 1
        for l in range(-1, -6, -1):
            if ind + l < 0:
                continue
            if abs(col[ind + l] - col[ind + l + 1]) > 10:
                break
            picked[ind + l] = 1

    rings = []
    for i in range(V):
        scan = []
        s, e = int(seg["start"][i]), int(seg["end"][i])
        for j in range(6):
            sp = FR._cdiv(s * (6 - j) + e * j, 6)
            ep = FR._cdiv(s * (5 - j) + e * (j + 1), 6) - 1
            if sp >= ep:
                continue
            sm[sp:ep] = sorted(sm[sp:ep])
            largest = 0
            for k in range(ep, sp - 1, -1):
                ind = sm[k][1]
                if picked[ind] == 0 and curvature[ind] > edge and not ground[ind]:
                    largest += 1
                    if largest <= 2:
                        label[ind] = 2
                    elif largest <= 20:
                        label[ind] = 1
                    else:
                        break
                    suppress(ind)
            smallest = 0
            for k in range(sp, ep + 1):
                ind = sm[k][1]
                if picked[ind] == 0 and curvature[ind] < surf and ground[ind]:
                    label[ind] = -1
                    smallest += 1
                    if smallest >= 4:
                        break
                    suppress(ind)
            for k in range(sp, ep + 1):
                if label[k] <= 0:
                    scan.append(k)
        rings.append(scan)
    return rings


def serial_outliers(ref, c):
    """imageProjection.cpp:544-558, the branch that pushes to _outlier_cloud"""
    out = []
    for i in range(c.V):
        for j in range(c.H):
            if ref["label"][i, j] > 0 or ref["ground"][i, j] == 1:
                if ref["label"][i, j] == 999999:
                    if i > c.gsi and j % 5 == 0:
                        p = ref["full"][i, j]
                        out.append([p[0], p[1], p[2], f32(f64(f32(i)) + f64(f32(j)) / 10000.0)])
                    continue
    return np.asarray(out, f32).reshape(-1, 4)


@pytest.mark.parametrize("name", AC.NAMES)
def test_restatement_equals_the_serial_transcription(name):
    k = AC.case(name)
    c, f = k["config"], k["f"]
    for period in AC.PERIODS:
        a = AC.expected(name, period)
        times, i0 = serial_times(f["seg"], a["start"], a["end"], a["diff"], period)
        assert i0 == a["i0"], (name, period)
        np.testing.assert_array_equal(bits(times), bits(a["times"]))
    picked = FR.occlusion(f["seg"])
    rings = serial_less_flat(f["seg"], f["curvature"], picked, k["edge"], k["surf"], c.V)
    want, _ = AR.candidates(f, c.V)
    assert [list(r) for r in rings] == [r.tolist() for r in want], name
    np.testing.assert_array_equal(bits(serial_outliers(k["ref"], c)), bits(AC.expected(name, 0.1)["outliers"]))


# ---- 2. hand-computed answers -------------------------------------------------------------------------------------------------
def test_hand_computed_orientation_and_times():
    """The sweep starts at (1, 0): start = -0.  It ends at (0, -1): -atan2f = pi / 2, + 2 pi = 5 pi / 2, which is between pi
    and 3 pi of the start, so diff = 5 pi / 2.  Points, all in ring 3, scan_period 0.1:
      (1, 0)        ori 0, rel 0                                    -> 3
      (0, -1)       ori pi / 2, rel 0.2                             -> 3.02
      (-1, -0.001)  ori pi - 0.001: no wrap, not past pi            -> 3 + 0.1 (pi - 0.001) / (5 pi / 2)
      (-1, 0.001)   ori -(pi - 0.001) < -pi / 2: + 2 pi = pi + 0.001, past pi: the flag flips HERE, this point keeps
                    the first branch                                 -> 3 + 0.1 (pi + 0.001) / (5 pi / 2)
      (0, 1)        second branch: -pi / 2 + 2 pi = 3 pi / 2, inside [end - 3 pi / 2, end + pi / 2], rel 0.6   -> 3.06
      (1, 0.001)    -0.001 + 2 pi, rel (2 pi - 0.001) / (5 pi / 2)  -> 3 + 0.1 of it"""
    c = R.Config(4, 64, -15.0, 15.0, 0)
    raw = np.array([[1, 0, 0], [0, -1, 0]], f32)
    start, end, diff, _ = AR.orientation(raw, c)
    assert start == 0 and abs(end - 2.5 * PI) < 1e-6 and abs(diff - 2.5 * PI) < 1e-6
    xy = [(1, 0), (0, -1), (-1, -0.001), (-1, 0.001), (0, 1), (1, 0.001)]
    seg = dict(xyz=np.array([[x, y, 0.3] for x, y in xy], f32), range=np.ones(6, f32), row=np.full(6, 3, np.int32))
    times, rel, i0, _ = AR.point_times(seg, start, end, diff, 0.1)
    assert i0 == 3
    want_rel = [0.0, 0.2, (PI - 0.001) / (2.5 * PI), (PI + 0.001) / (2.5 * PI), 0.6, (2 * PI - 0.001) / (2.5 * PI)]
    np.testing.assert_allclose(rel, want_rel, rtol=0, atol=2e-7)
    np.testing.assert_allclose(times, 3 + 0.1 * np.asarray(want_rel), rtol=0, atol=3e-7)
    assert (AR.point_times(seg, start, end, diff, 0.0)[0] == 3).all()
    # the two corrections of findStartEndAngle: an end a little behind the start comes out one turn later, not three
    s2, e2, d2, _ = AR.orientation(np.array([[0, -1, 0], [1, 0, 0]], f32), c)          # start pi / 2, end 0 + 2 pi: 3 pi / 2 apart
    assert abs(s2 - PI / 2) < 1e-6 and abs(d2 - 1.5 * PI) < 1e-6
    s3, e3, d3, _ = AR.orientation(np.array([[0, 1, 0], [-1, -0.001, 0]], f32), c)     # start -pi / 2, end 3 pi - 0.001: more than 3 pi
    assert abs(d3 - (1.5 * PI - 0.001)) < 2e-6                                         # apart, one turn comes off
    s4, e4, d4, _ = AR.orientation(np.array([[0, -1, 0], [-0.001, 1, 0]], f32), c)     # start pi / 2, end 3 pi / 2 - 0.001: less than pi
    assert abs(d4 - (3 * PI - 0.001)) < 2e-6                                           # apart, one turn is added
    assert AR.orientation(np.zeros((0, 3), f32), c)[:3] == (0, 0, 0)


def test_hand_computed_ring():
    """A ring of 23 points that is the whole cloud: start 4, end 17.  The sixths are [4, 5] [6, 7] [8, 9] [10, 11] [12, 13]
    [14, 16] (the last ep is 17 * 6 / 6 - 1): 13 slots, index 17 is in none.  Index 6 is a less-sharp pick and 12 a sharp
    one (labels 1 and 2: out), 9 a flat pick (label -1: in).  Then five of the candidates through the voxel grid, leaf 0.2,
    x only: 0.05 -> voxel 0, 0.25 -> 1, 0.15 -> 0, -0.05 -> -1 (floor, not truncation), 0.3 -> 1; min_b = -1, so the output
    order is the fourth point, (first + third) / 2, (second + fifth) / 2."""
    seg = dict(range=np.ones(23, f32), start=np.array([4], np.int32), end=np.array([17], np.int32))
    f = dict(seg=seg, lists=[np.array([12]), np.array([12, 6]), np.array([9])])
    rings, skipped = AR.candidates(f, 1)
    assert rings[0].tolist() == [4, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16] and skipped == [0]
    pts = np.array([[0.05, 0.05, 0.05, 1], [0.25, 0.05, 0.05, 2], [0.15, 0.05, 0.05, 3], [-0.05, 0.05, 0.05, 5], [0.3, 0.05, 0.05, 4]], f32)
    cen, members, over = AR.voxel_grid(pts)
    assert not over and members == [[3], [0, 2], [1, 4]]
    np.testing.assert_array_equal(bits(cen[0]), bits(pts[3]))
    np.testing.assert_array_equal(bits(cen[1]), bits((pts[0] + pts[2]) / f32(2)))
    np.testing.assert_array_equal(bits(cen[2]), bits((pts[1] + pts[4]) / f32(2)))
    np.testing.assert_allclose(cen[:, 0], [-0.05, 0.1, 0.275], atol=1e-7)
    np.testing.assert_allclose(cen[:, 3], [5, 2, 3], atol=0)
    # a ring of 21 points: end - start = 11, the first sixth is [4, 4]: skipped, and its slot 4 is no candidate
    seg = dict(range=np.ones(21, f32), start=np.array([4], np.int32), end=np.array([15], np.int32))
    rings, skipped = AR.candidates(dict(seg=seg, lists=[np.array([], np.int64)] * 3), 1)
    assert skipped == [1] and rings[0].tolist() == list(range(5, 15))
    # the leaf-size check: 3 points 40 km apart on every axis hand the input through, in input order
    far = np.array([[0, 0, 0, 1], [4e4, 4e4, 4e4, 2], [-4e4, 1, 1, 3]], f32)
    cen, members, over = AR.voxel_grid(far)
    assert over and members == [[0], [1], [2]]
    np.testing.assert_array_equal(bits(cen), bits(far))
    near = far.copy()
    near[:, :3] *= f32(1e-3)                               # 80 m x 40 m x 40 m: 401 * 201 * 201 voxels fit
    assert not AR.voxel_grid(near)[2]


# ---- 3. the voxel grid against the observation's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("counts", "wide", "16x440-g7-m0.0"))
def test_voxel_grid_equals_the_observations_on_the_same_points(name):
    k = AC.case(name)
    a = AC.expected(name, 0.1)
    rings, _ = AR.candidates(k["f"], k["config"].V)
    at = 0
    for ks, n_vox in zip(rings, a["ring_voxels"]):
        pts = AR.association_frame(k["f"]["seg"], ks, a["times"])
        other = OR.voxel_grid(pts[:, :3], (AR.LEAF, AR.LEAF, AR.LEAF))
        assert len(other) == n_vox
        np.testing.assert_array_equal(bits(a["clouds"][0][3][0][at: at + n_vox, :3]), bits(other))
        at += n_vox
    assert at == len(a["clouds"][0][3][0]) > 0


# ---- 4. the conditions the GPU test relies on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.NAMES)
def test_every_case_keeps_its_margins(name):
    k = AC.case(name)
    assert k["ref"]["n_fragile"] == 0 and k["f"]["n_tie_sensitive"] == 0
    for period in AC.PERIODS:
        a = AC.expected(name, period)
        assert a["min_margin"] >= AC.MARGIN, (name, period, a["min_margin"])
        assert len(a["times"]) == len(k["f"]["seg"]["range"]) and np.isfinite(a["times"]).all()
        if period == 0.0:
            np.testing.assert_array_equal(a["times"], k["f"]["seg"]["row"].astype(f32))


def test_the_cases_cover_the_shapes():
    A = {n: AC.expected(n, 0.1) for n in AC.NAMES}
    n_seg = {n: len(AC.case(n)["f"]["seg"]["range"]) for n in AC.NAMES}
    small = A["small"]
    assert small["ring_skipped"][:2] == [6, 1] and small["ring_candidates"][0] == 0 and small["ring_candidates"][1] == 10
    assert AC.case("small")["f"]["seg"]["end"][0] - AC.case("small")["f"]["seg"]["start"][0] < 0      # fewer than 11 points
    assert A["counts"]["ring_candidates"][:6] == [63, 64, 65, 255, 256, 257] and A["counts"]["ring_candidates"][6] == 0
    assert A["counts"]["ring_voxels"][7] == 1 < A["counts"]["ring_candidates"][7]                      # a whole ring inside one voxel
    wide = AC.case("wide")
    assert wide["config"].V == 2 and wide["config"].H == 4096 and wide["config"].gsi == 0
    assert min(A["wide"]["ring_candidates"]) > 4000 > 1024 and A["wide"]["n_scattered"] > 0 and A["wide"]["n_single"] > 0
    assert len(wide["f"]["lists"][FR.LESS_SHARP]) > 0                                                  # labels > 0 inside a long ring
    assert all(A["overflow"]["ring_overflow"]) and not any(A["small"]["ring_overflow"])
    assert A["overflow"]["clouds"][0][3][0][:, :3].max() > 1e4
    pts = A["wide"]["clouds"][0][3][0]
    assert (pts[:, :3].min(axis=0) < 0).all() and (pts[:, :3].max(axis=0) > 0).any()                   # both sides of zero
    ring0 = AC.case("flip-in-ring-0")["f"]["seg"]["row"]
    assert 0 < A["flip-in-ring-0"]["i0"] < 7 and (ring0[:8] == 0).all() and ring0[8] == 1      # inside ring 0, not at its end
    assert A["flip-at-the-last-point"]["i0"] == n_seg["flip-at-the-last-point"] - 1
    assert A["never-flips"]["i0"] == n_seg["never-flips"] and A["never-flips"]["diff"] < PI * 2
    assert A["empty"]["i0"] == 0 and (A["empty"]["start"], A["empty"]["end"], A["empty"]["diff"]) == (0, 0, 0)
    junk = AC.case("small-junk-ends")["raw"]
    assert not np.isfinite(junk[0]).all() and not np.isfinite(junk[-1]).all() and not np.isfinite(junk[1]).all()
    assert bits(A["small-junk-ends"]["start"]) == bits(A["small"]["start"]) and A["small-junk-ends"]["i0"] == small["i0"]
    # outliers: invalid labels at and below ground_scan_index and off the fifth columns exist and are left out
    for name in AC.SCENES:
        k = AC.case(name)
        inv = np.argwhere(k["ref"]["label"] == R.INVALID)
        gsi = k["config"].gsi
        assert ((inv[:, 0] <= gsi) & (inv[:, 1] % 5 == 0)).any() or name != "16x440-g7-m0.0"
        assert ((inv[:, 0] > gsi) & (inv[:, 1] % 5 != 0)).any()
        assert len(A[name]["outliers"]) == ((inv[:, 0] > gsi) & (inv[:, 1] % 5 == 0)).sum() > 0
        assert len(k["f"]["lists"][FR.FLAT]) > 0 and len(k["f"]["lists"][FR.SHARP]) > 0
    # voxel averages that differ from every summand's intensity: the intensity really is averaged
    lf, times = A["16x440-g7-m0.0"]["clouds"][0][3][0], A["16x440-g7-m0.0"]["times"]
    assert len(set(lf[:, 3].tolist()) - set(times.tolist())) > 0


# ---- 5. the public surface ------------------------------------------------------------------------------------------------------
def test_the_entries_and_the_class():
    from dddmr_navigation_amd import _capi as K, sweep_association
    names = ("set_lidar_sweep_association", "get_lidar_sweep_orientation", "get_lidar_sweep_times", "get_lidar_sweep_association",
             "get_lidar_sweep_outliers")
    header = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    for n in names:
        assert "dddmr_rollout_" + n in K.SIGNATURES and f"int dddmr_rollout_{n}(" in header
    assert len(K.SIZEOF_STRUCTS) == 23                                    # plain scalars and arrays: no new struct
    cls = sweep_association.SweepAssociation
    public = sorted(n for n, _ in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_"))
    assert public == ["close", "cloud", "orientation", "outliers", "times"]
    assert list(inspect.signature(cls.__init__).parameters) == ["self", "lp", "source_id", "scan_period"]
    assert inspect.signature(cls.__init__).parameters["scan_period"].default == 0.1
