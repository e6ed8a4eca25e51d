"""Hand-worked answers for the NumPy restatement of the depth camera's frustum, point tests and clearing verdicts
(tests/helpers/depth_frustum_ref.py), and the margins of the inputs tests/test_depth_clear_gpu.py draws: every
comparison the restatement makes for a kept input stays MARGIN_* away from its threshold, and rejection discards under
half of the draws.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import scenes
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_feed_ref as F  # noqa: E402
import depth_frustum_ref as R  # noqa: E402
import depth_clear_cases as cases  # noqa: E402

IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
HALF_PI = math.pi / 2.0


def square_frustum(T=IDENT):
    """FOV 90 x 90 degrees, 1 .. 2 m: side planes y = +-x, z = +-x"""
    return R.Frustum(HALF_PI, HALF_PI, 1.0, 2.0, T)


def test_identity_vertices_in_the_reference_order():
    fr = square_frustum()
    want = [(1, 1, 1), (1, -1, 1), (1, 1, -1), (1, -1, -1), (2, 2, 2), (2, -2, 2), (2, 2, -2), (2, -2, -2)]   # TLNear .. BRFar
    np.testing.assert_array_equal(fr.vtx, np.array(want, np.float32))
    assert fr.vtx.dtype == np.float32 and fr.nrm.dtype == np.float32 and fr.pl.dtype == np.float32
    np.testing.assert_array_equal(fr.origin, [0.0, 0.0, 0.0])


def test_normals_point_inward_and_planes_contain_their_vertices():
    fr = square_frustum()
    assert (fr.tests(np.array([[1.5, 0.0, 0.0]], np.float32)) > 0).all()
    # near, right, bottom, left, far, top: hand-computed cross products of the identity frustum
    np.testing.assert_array_equal(fr.nrm, np.array([(4, 0, 0), (4, 4, 0), (4, 0, 4), (4, -4, 0), (-16, 0, 0), (4, 0, -4)], np.float32))
    # plane 0 is the left side (TLNear, TLFar, BLNear): y = x
    a, b, c, d = fr.pl[0]
    assert d == 0 and a == -b and c == 0
    for tri, pl in zip(((0, 4, 2), (2, 3, 6), (1, 3, 7), (0, 1, 4), (0, 2, 3), (4, 5, 7)), fr.pl):
        for v in tri:
            assert abs(float(pl[:3] @ fr.vtx[v] + pl[3])) < 1e-5


def test_transformed_frustum_moves_with_the_pose():
    T = (10.0, -3.0, 0.5) + tuple(scenes.quat_from_rpy(0.0, 0.0, HALF_PI))          # yawed left by 90 degrees
    fr = square_frustum(T)
    np.testing.assert_allclose(fr.vtx[0], [10.0 - 1.0, -3.0 + 1.0, 0.5 + 1.0], atol=1e-6)     # TLNear (1, 1, 1) -> (-1, 1, 1) + t
    inside, attach, _ = R.point_tests([fr], np.array([[10.0, -1.5, 0.5], [9.7, -4.0, 1.0]], np.float32))
    # the second point is (-1, 0.3, 0.5) in the camera frame: behind the camera, 0.35 m or more from every (infinite) plane
    assert inside.tolist() == [True, False] and attach.tolist() == [False, False]


def test_attachment_near_a_side_plane_only():
    fr = square_frustum()
    near_plane = (1.5, 1.5 - 0.05 * math.sqrt(2.0), 0.0)         # 0.05 m inside the left plane y = x
    deep = (1.5, 0.0, 0.0)                                       # 0.5 m from the near and far planes, 1.06 m from the sides
    inside, attach, ok = R.point_tests([fr], np.array([near_plane, deep], np.float32))
    assert inside.tolist() == [True, True] and attach.tolist() == [True, False] and ok.all()
    _, dis, hyp = fr.plane_attach(np.array([near_plane], np.float32))
    assert abs(float(dis[0, 0]) - 0.05) < 1e-6 and dis.dtype == np.float32 and hyp.dtype == np.float64
    # beyond max_detect_distance_ + 0.5 = 2.5 m in the xy plane nothing attaches, however close the plane
    far = (2.0, 1.98, 0.0)
    assert math.hypot(far[0], far[1]) > 2.5
    assert R.point_tests([fr], np.array([far], np.float32))[1].tolist() == [False]


def test_another_cameras_interior_cancels_an_attachment():
    a = square_frustum()
    b = square_frustum((0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0))     # the same camera one metre to the left
    p = np.array([[1.5, 1.5 - 0.05 * math.sqrt(2.0), 0.0]], np.float32)   # attaches a's left plane, 0.76 m inside b's
    assert R.point_tests([a], p)[1].tolist() == [True]
    assert R.point_tests([a, b], p)[1].tolist() == [False]
    assert R.point_tests([b, a], p)[1].tolist() == [False]       # b attaches nothing, a is asked next, b cancels
    # a point that attaches both cameras stays attached: b holds it, but not unattached
    q = np.array([[1.5, 1.5 - 0.04, 0.0]], np.float32)
    c = square_frustum((0.0, 0.08, 0.0, 0.0, 0.0, 0.0, 1.0))
    assert R.point_tests([a, c], q)[1].tolist() == [True]


def hand_markings():
    """one marking per leaf of selfClear's tree (observation not clear), on the identity frustum"""
    obs = [(-1.0, 0.0, 0.02),                                    # 0.02 m from the voxel of L1
           (1.5, 1.45, 0.3), (1.5, 1.45, 0.4),                    # engaged by L3
           (1.5, 1.45, -0.3),                                     # engaged by L4
           (1.5, 0.0, 0.2), (1.5, 0.1, 0.2), (1.5, 0.2, 0.2), (1.5, 0.3, 0.2), (1.5, 0.4, 0.2)]   # engaged by L5
    obs = np.array(obs, np.float32)
    eps = np.array([0.005, 0.0, 0.0], np.float32)
    far = lambda k: np.array([[1.2, -0.5 + 0.03 * i, -0.4] for i in range(k)], np.float32)      # 0.02 m or more from everything
    vox, clusters = [], []
    vox.append((-20, 0, 0)); clusters.append(far(3))                                              # L1 outside, observed -> kept
    vox.append((-20, 20, 0)); clusters.append(far(3))                                             # L2 outside, nothing near -> removed
    vox.append((30, 29, 0)); clusters.append(np.concatenate([obs[1:3] + eps, far(8)]))            # L3 attached, 2 / 10 -> kept
    vox.append((30, 29, 1)); clusters.append(np.concatenate([obs[3:4] + eps, far(9)]))            # L4 attached, 1 / 10 = 0.1, not > 0.1 -> removed
    vox.append((30, 0, 0)); clusters.append(np.concatenate([obs[4:9] + eps, far(15)]))            # L5 inside, 5 / 20 -> kept
    vox.append((30, 0, 2)); clusters.append(far(20))                                              # L6 inside, 0 / 20 -> removed
    off = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.uint32)
    return obs, np.array(vox, np.int32), off, np.concatenate(clusters)


def test_every_leaf_of_the_verdict_tree():
    obs, vox, off, cl = hand_markings()
    verdict, engaged, _ = R.clear_verdicts([square_frustum()], obs, 0.05, 0.05, vox, off, cl)
    #                           outside   attached   inside    (branch << 1 | kept)
    assert verdict.tolist() == [3, 2,     5, 4,      7, 6]
    assert engaged.tolist() == [0, 0, 2, 1, 5, 0]


def test_observation_of_five_points_counts_as_clear():
    obs, vox, off, cl = hand_markings()
    fr = [square_frustum()]
    v5, e5, _ = R.clear_verdicts(fr, obs[:5], 0.05, 0.05, vox, off, cl)
    assert v5.tolist() == [2, 2, 4, 4, 6, 6] and not e5.any()          # nothing is searched: every marking goes
    v6, e6, _ = R.clear_verdicts(fr, obs[:6], 0.05, 0.05, vox, off, cl)
    assert v6.tolist() == [3, 2, 5, 4, 6, 6] and e6.tolist() == [0, 0, 2, 1, 2, 0]   # L5's points are obs[4:9]: two of them left, 2 / 20 = 0.1, not > 0.1


def test_empty_cluster_in_a_ratio_branch_divides_by_zero():
    obs, vox, off, cl = hand_markings()
    off2 = off.copy()
    off2[5:] = off2[4]                                                   # L5 and L6 lose their clusters
    with pytest.raises(ZeroDivisionError):
        R.clear_verdicts([square_frustum()], obs, 0.05, 0.05, vox, off2, cl[: off2[-1]])
    # outside the frustums the cluster is never read
    v, _, _ = R.clear_verdicts([square_frustum()], obs, 0.05, 0.05, vox[:2], np.zeros(3, np.uint32), cl[:0])
    assert v.tolist() == [3, 2]


def test_radius_search_is_strict_and_in_float():
    obs = np.array([[0.0, 0.0, 0.0]], np.float32)
    r2 = np.float32(0.01 * 0.01)
    inside = np.float32(np.sqrt(np.float64(r2)) * (1 - 1e-3))
    outside = np.float32(np.sqrt(np.float64(r2)) * (1 + 1e-3))
    hit, ok = R.radius_any(obs, np.array([[inside, 0, 0], [outside, 0, 0], [0.5, 0, 0]], np.float32), 0.01)
    assert hit.tolist() == [True, False, False] and ok.all()
    # a pair on the threshold is flagged
    on = np.float32(np.sqrt(np.float64(r2)))
    assert not R.radius_any(obs, np.array([[on, 0, 0]], np.float32), 0.01)[1][0]


# ---- the inputs of the GPU tests keep their margins ----------------------------------------------------------------
def scene_observation(sc):
    return np.concatenate([F.frame_observation(sc.frames[i], sc.T_base_cam[i], sc.T_gbl_base, sc.z_min, sc.z_max) for i in range(2)])


def test_scene_reaches_every_leaf_with_margins():
    sc = scenes.depth_clear_scene()
    obs = scene_observation(sc)
    assert len(obs) > 5000
    frs = [R.Frustum(sc.fov_w, sc.fov_v, sc.d_min, sc.d_max, sc.T_gbl_cam(i)) for i in range(2)]
    vox, off, cl = sc.markings(obs)
    verdict, engaged, ok = R.clear_verdicts(frs, obs, sc.res, sc.hres, vox, off, cl)
    assert 1.0 - ok.mean() < 0.5, "rejection discards half of the scene's markings"
    assert cases.leaves(verdict[ok]) == {2, 3, 4, 5, 6, 7}, cases.leaves(verdict[ok])
    size = off[1:].astype(np.int64) - off[:-1]
    assert size.min() >= 1 and size.max() <= 200
    assert (engaged[ok] > 0).sum() > 50
    print(f"scene: {len(obs)} observation points, {len(vox)} markings, {100 * (1 - ok.mean()):.1f}% discarded, "
          f"leaves {np.bincount(verdict[ok], minlength=8)[2:].tolist()}")


@pytest.mark.parametrize("far,cams", [(False, 1), (True, 2), (False, 2)])
def test_random_markings_keep_their_margins(far, cams):
    shift = cases.SHIFT_FAR if far else np.zeros(3)
    cloud = cases.shifted_cloud(shift)
    t_gb = cases.base_pose(shift)
    rig = (cases.T_BASE_CAM_ROLLED if far else cases.T_BASE_CAM)[:cams]
    obs = np.concatenate([F.frame_observation(cases.render(cloud, t_gb, t, 30 + i), t, t_gb, cases.Z_MIN, cases.Z_MAX)
                          for i, t in enumerate(rig)])
    frs = [cases.frustum(t_gb, t)[0] for t in rig]
    vox, off, cl, verdict, engaged, discarded = cases.draw(frs, obs, t_gb[:3], 2600, 77, cases.anchors_of(t_gb, rig))
    assert discarded < 0.5 and len(vox) >= 2000
    assert cases.leaves(verdict) == {2, 3, 4, 5, 6, 7}
    # the margins of the kept inputs, recomputed
    pt = np.stack([(vox[:, 0] * 0.05), (vox[:, 1] * 0.05), (vox[:, 2] * 0.05)], axis=1).astype(np.float32)
    for fr in frs:
        assert np.abs(fr.tests(pt)).min() >= R.MARGIN_TEST
        assert np.abs(fr.plane_attach(pt)[1].astype(np.float64) - float(R.DIS2REJ)).min() >= R.MARGIN_DIS
    print(f"far={far} cameras={cams}: {len(obs)} observation points, {len(vox)} markings kept, {100 * discarded:.1f}% discarded")


def test_random_points_keep_their_margins():
    t_gb = cases.base_pose(cases.SHIFT_FAR)
    frs = [cases.frustum(t_gb, t)[0] for t in cases.T_BASE_CAM_ROLLED]
    pts, inside, attach, discarded = cases.draw_points(frs, t_gb[:3], 150_000, 9, cases.anchors_of(t_gb, cases.T_BASE_CAM_ROLLED))
    assert discarded < 0.5 and len(pts) >= 100_000
    assert inside.sum() > 1000 and attach.sum() > 1000 and (inside & ~attach).sum() > 1000 and (~inside & attach).sum() > 100
    print(f"points: {len(pts)} kept, {100 * discarded:.1f}% discarded, {int(inside.sum())} inside, {int(attach.sum())} attached")


def test_depth_clear_bridge_compiles_and_behaves_without_ros():
    """feedDepthFrustum() / depthClearVerdicts() of perception_bridge.h against a fake C-ABI (tests/cpp/depth_clear_bridge_test.cpp)."""
    import shutil
    import subprocess
    import tempfile
    assert shutil.which("g++") is not None, "needs g++"
    ad = os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "depth_clear_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", ad,
                            os.path.join(ROOT, "tests", "cpp", "depth_clear_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "depth clear bridge OK" in r.stdout, (r.stdout, r.stderr)


def test_new_entry_points_are_exported_and_laid_out():
    """the library exports the depth clearing calls and agrees on dddmr_depth_frustum_config's layout"""
    import ctypes as C
    from dddmr_navigation_amd import _capi as K
    lib = K.load_library()
    for s in ("dddmr_rollout_set_depth_frustum", "dddmr_rollout_get_depth_frustum", "dddmr_rollout_depth_frustum_test",
              "dddmr_rollout_depth_clear_verdicts", "dddmr_rollout_depth_clear_launches"):
        assert s in K.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert C.sizeof(K.DepthFrustumConfig) == lib.dddmr_rollout_sizeof(10) == 32
