"""GPU parity of the depth image path (set_depth_image_source / set_depth_image / get_depth_image_cloud) against the
NumPy restatement of DepthImg2PointCloud::cbDepthImg (tests/helpers/depth_image_ref.py) followed by the restatement of
bufferCloud (tests/helpers/depth_feed_ref.py).

PCL sums a voxel's points in float in an unspecified order, so stage one's centroids are defined only up to that, and
stage two makes yes / no decisions on them.  Hence: stage one against the restatement with a tolerance taken from the
restatement's own two summation orders; stage two against the restatement applied to the library's own stage-one cloud
(the comparison the depth feed tests make); end to end only with height limits placed where the reference is decided.
Every measured figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

from dddmr_navigation_amd import _capi as K, configs, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT
import oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_feed_ref as R  # noqa: E402
import depth_image_ref as I  # noqa: E402
import depth_image_cases as Cs  # noqa: E402

pytestmark = pytest.mark.gpu

IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
MS = 1_000_000
TBO, POSES = Cs.TBO_CAM, Cs.POSES
TBS_LIDAR = (0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0)
ZMIN, ZMAX = 0.0, 2.0


def planner(max_points=200_000, theory="C2"):
    return LocalPlanner([configs.bench_theory(theory)], max_points=max_points)


def sort_rows(p):
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def assert_one_to_one(got, ref, tol, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    if not len(ref):
        return 0.0
    d, idx = cKDTree(ref).query(got)
    print(f"{what}: {len(ref)} points, largest distance {d.max():.3e} m, tolerance {tol:.3e} m")
    assert d.max() <= tol, (what, d.max(), tol)
    assert len(np.unique(idx)) == len(ref), what
    return float(d.max())


def source(lp, sid, img, K4, node, zmin=ZMIN, zmax=ZMAX, drop_zero=False, **kw):
    lp.set_depth_image_source(sid, zmin, zmax, img.shape[1], img.shape[0], *K4, max_distance=node["max_distance"],
                              leaf_size=node["leaf_size"], sample_step=node["sample_step"], drop_zero=drop_zero, **kw)


def stage_one_check(img, K4, node, drop_zero=False, what=""):
    ref, tol, spread = I.stage_one_tolerance(img, K4, drop_zero=drop_zero, **node)
    with planner() as lp:
        source(lp, 1, img, K4, node, zmin=-100.0, zmax=100.0, drop_zero=drop_zero)
        n_cam, n_frame, n_src, n_all = lp.set_depth_image(1, img, TBO, POSES[0], 10**9)
        got = lp.get_depth_image_cloud(1)
        # the camera-frame table was left clean: the same image again gives the same cloud
        again = lp.set_depth_image(1, img, TBO, POSES[0], 10**9 + 33 * MS)
        got2 = lp.get_depth_image_cloud(1)
    print(f"{what}: float summation orders differ by {spread:.3e} m")
    assert n_cam == len(ref) == len(got), (what, n_cam, len(ref), len(got))
    assert_one_to_one(got, ref, tol, what)
    assert again[0] == n_cam
    assert_one_to_one(got2, ref, tol, what + " (again)")
    return ref, got


# ---- 1. stage one ----------------------------------------------------------------------------------------------------
def test_stage_one_small_image():
    img, K4 = Cs.render(160, 120, 0, 1)
    stage_one_check(img, K4, dict(max_distance=4.0, leaf_size=0.05, sample_step=1), what="160x120 step 1")


@pytest.mark.parametrize("leaf", [0.05, 0.1])
@pytest.mark.parametrize("max_distance", [4.0, 6.0])
@pytest.mark.parametrize("step", [1, 2, 4])
@pytest.mark.parametrize("shape", [(640, 480), (848, 480)])
def test_stage_one_matches_the_node(shape, step, max_distance, leaf):
    img, K4 = Cs.render(shape[0], shape[1], 0, 10)
    assert 0.05 < (img == 0).mean() < 0.95                  # pixels without a return and pixels with one
    stage_one_check(img, K4, dict(max_distance=max_distance, leaf_size=leaf, sample_step=step),
                    what=f"{shape[0]}x{shape[1]} step {step} max {max_distance} leaf {leaf}")


@pytest.mark.parametrize("drop_zero", [False, True])
@pytest.mark.parametrize("kind", ["rendered", "all_zero", "no_zero", "padded"])
def test_stage_one_zero_pixels_and_padding(kind, drop_zero):
    img, K4 = Cs.render(640, 480, 1, 11)
    node = dict(Cs.DEFAULTS, sample_step=1)
    if kind == "all_zero":
        img = np.zeros_like(img)
    elif kind == "no_zero":
        img = np.where(img == 0, np.uint16(2500), img).astype(np.uint16)
    elif kind == "padded":
        wide = np.full((480, 640 + 24), 777, np.uint16)         # the padding holds plausible depths: it must not be read
        wide[:, :640] = img
        img = wide[:, :640]
        assert img.strides == (2 * 664, 2)
        node = dict(Cs.DEFAULTS, sample_step=2)
    ref, got = stage_one_check(img, K4, node, drop_zero=drop_zero, what=f"{kind} drop_zero={drop_zero}")
    if kind == "all_zero":
        assert len(ref) == (0 if drop_zero else 1)
        if not drop_zero:
            assert not got.any()                               # one point, (0, 0, 0)
    origin = (np.abs(ref) == 0).all(axis=1).sum()
    assert origin == (0 if drop_zero or kind == "no_zero" else 1)


# ---- 2. stage two, given stage one -----------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,above", [(0.05, False), (0.02, True)])
def test_stage_two_on_the_librarys_own_stage_one(leaf, above):
    img, K4 = Cs.render(848, 480, 0, 10)
    node = dict(max_distance=4.0, leaf_size=leaf, sample_step=1)
    ref_one = I.stage_one(img, K4, **node)
    n_band = len(R.height_band(R.transform(ref_one, TBO), ZMIN, ZMAX))
    print(f"leaf {leaf}: {len(ref_one)} stage-one points, {n_band} inside the band (restatement)")
    assert (n_band > R.VOXELIZE_ABOVE + 1000) if above else (1000 < n_band < R.VOXELIZE_ABOVE - 1000)
    tgb = POSES[1]
    with planner() as lp:
        source(lp, 1, img, K4, node)
        n_cam, n_frame, n_src, n_all = lp.set_depth_image(1, img, TBO, tgb, 10**9)
        one = lp.get_depth_image_cloud(1)
        got = lp.get_cloud()
    assert n_cam == len(one) == len(ref_one)
    ref, voxelised = R._frame(one, TBO, tgb, ZMIN, ZMAX)
    assert voxelised == above
    assert n_frame == n_src == n_all == len(got) == len(ref)
    assert not got[:, 3].any()
    if above:
        assert_one_to_one(got[:, :3], ref, 1e-5, f"stage two above 20000 (leaf {leaf})")
    else:
        np.testing.assert_array_equal(sort_rows(got[:, :3]), sort_rows(ref))


# ---- 3. end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Cs.end_to_end_cases(), ids=[c[0] for c in Cs.end_to_end_cases()])
def test_end_to_end_where_the_reference_is_decided(case):
    name, pose, seed, node = case
    img, K4 = Cs.render(848, 480, pose, seed)
    (zmin, zmax), gaps = Cs.end_to_end_band(pose, seed, node)
    print(f"{name}: limits {zmin:.6f} / {zmax:.6f}, gaps {gaps[0]:.3e} / {gaps[1]:.3e} m")
    assert min(gaps) >= Cs.MIN_GAP
    _, tol, _ = I.stage_one_tolerance(img, K4, **node)
    ref = I.observation(img, K4, TBO, POSES[pose], zmin, zmax, **node)
    assert 1000 < len(ref) <= R.VOXELIZE_ABOVE
    with planner() as lp:
        source(lp, 2, img, K4, node, zmin=zmin, zmax=zmax)
        n_cam, n_frame, n_src, n_all = lp.set_depth_image(2, img, TBO, POSES[pose], 10**9)
        got = lp.get_cloud()
    assert n_frame == n_src == n_all == len(got) == len(ref)
    assert_one_to_one(got[:, :3], ref, tol + 1e-6, name)


# ---- 4. sequence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistence_ms", [0, 100, 350])
def test_sequence_two_image_sources_and_a_lidar(persistence_ms):
    """12 images at 30 Hz (with jitter) per camera while the robot moves, a lidar scan every fourth step: after every call
    the sizes per frame, per source and of the aggregate are the restatement's, sources in source order."""
    cloud = scenes.cloud_c2()
    rng = np.random.default_rng(41)
    tbs = {1: (0.15, 0.1, 0.3) + tuple(scenes.quat_from_rpy(0.0, 0.05, 0.6)),
           2: (0.15, -0.1, 0.3) + tuple(scenes.quat_from_rpy(0.0, 0.05, -0.6))}
    tbo = {k: R.compose(v, scenes.T_LINK_OPTICAL) for k, v in tbs.items()}
    node = {1: dict(Cs.DEFAULTS), 2: dict(max_distance=6.0, leaf_size=0.1, sample_step=1)}
    shape = {1: (320, 240), 2: (160, 120)}
    bufs = {k: R.DepthBufferRef(-10.0, 10.0, persistence_ms * MS) for k in (1, 2)}
    n_lidar = 0
    with planner(max_points=400_000) as lp:
        K4 = {}
        for k in (1, 2):
            _, K4[k] = scenes.depth_image(cloud[:10], IDENT, *shape[k], 1.5, 1.0, 8.0)
            lp.set_depth_image_source(k, -10.0, 10.0, shape[k][0], shape[k][1], *K4[k], observation_persistence_ns=persistence_ms * MS,
                                      max_frames=16, **node[k])
        stamp = 1_700_000_000 * 10**9 + 123
        for k in range(12):
            tgb = (-2.0 + 0.05 * k, 0.1, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.02 * k))
            if k % 4 == 1:
                scan = scenes.lidar_scan(cloud, sensor_xyz=(tgb[0], tgb[1], 0.5), seed=60 + k)
                n_lidar, n_all = lp.set_scan_source(0, scan, TBS_LIDAR, tgb, 10.0, 2.0)
                assert n_lidar == len(oracle.feed(scan, TBS_LIDAR, tgb, 10.0, 2.0))
                assert n_all == n_lidar + sum(sum(b.frame_sizes()) for b in bufs.values())
            for cam in (1, 2):
                stamp += 16_666_666 + int(rng.integers(-2 * MS, 2 * MS))
                img, _ = scenes.depth_image(cloud, R.compose(tgb, tbs[cam]), *shape[cam], 1.5, 1.0, 8.0, seed=100 + 2 * k + cam)
                one = I.stage_one(img, K4[cam], **node[cam])
                assert len(one) <= R.VOXELIZE_ABOVE
                bufs[cam].buffer_cloud(one, tbo[cam], tgb, stamp)
                n_cam, n_frame, n_src, n_all = lp.set_depth_image(cam, img, tbo[cam], tgb, stamp)
                sizes = bufs[cam].frame_sizes()
                assert n_cam == len(one) and n_frame == sizes[-1] and n_src == sum(sizes), (k, cam, sizes)
                total = n_lidar + sum(sum(b.frame_sizes()) for b in bufs.values())
                got = lp.get_cloud()[:, :3]
                assert n_all == total == len(got)
                # segments in source order, frames oldest first, each with the coordinates of its arrival pose
                at = n_lidar
                for c in (1, 2):
                    for _, ref, _ in bufs[c].frames:
                        d = cKDTree(ref).query(got[at:at + len(ref)])[0]
                        assert d.max() <= 1e-3, (k, cam, c, d.max())   # which frame sits where (poses are 5 cm apart), not how close
                        at += len(ref)
                assert at == len(got)
        assert n_lidar > 0
        for b in bufs.values():
            assert (len(b.frames) == 1) if persistence_ms == 0 else (len(b.frames) > 2)


# ---- 5. refusals change nothing --------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    img, K4 = Cs.render(160, 120, 0, 1)
    big, K4b = Cs.render(640, 480, 0, 10)
    node = dict(max_distance=6.0, leaf_size=0.05, sample_step=1)
    n_small = len(I.observation(img, K4, TBO, POSES[0], ZMIN, ZMAX, **node))
    n_big = len(I.observation(big, K4b, TBO, POSES[0], ZMIN, ZMAX, **node))
    assert n_small > 500 and n_big > n_small
    fr = scenes.depth_frame(scenes.cloud_c2(), R.compose(POSES[0], Cs.TBS_CAM), 160, 120, 1.5, 1.0, 8.0, seed=1)
    pose = (K.C.c_double * 7)(*IDENT)
    with planner(max_points=n_big + n_small // 2) as lp:
        def refused(code, fn, *a, **kw):
            before = lp.get_cloud().tobytes()
            with pytest.raises(RolloutError) as e:
                fn(*a, **kw)
            assert e.value.code == code, (e.value.code, code)
            assert lp.get_cloud().tobytes() == before
        # configuration: sample_step 0, max_frame_points below the sampled pixels, unknown flag, a box of 2^31 cells
        refused(K.ERR_BAD_ARG, lp.set_depth_image_source, 1, ZMIN, ZMAX, 160, 120, *K4, sample_step=0)
        refused(K.ERR_BAD_ARG, lp.set_depth_image_source, 1, ZMIN, ZMAX, 160, 120, *K4, sample_step=1, max_frame_points=160 * 120 - 1)
        refused(K.ERR_BAD_ARG, lp.set_depth_image_source, 1, ZMIN, ZMAX, 160, 120, *K4, sample_step=2, max_frame_points=80 * 60 - 1)
        refused(K.ERR_BAD_ARG, lp.set_depth_image_source, 1, ZMIN, ZMAX, 160, 120, *K4, sample_step=1, max_distance=60.0, leaf_size=0.001)
        cfg = K.DepthSourceConfig(ZMIN, ZMAX, 0, 160 * 120, 1)
        icfg = K.DepthImageConfig(160, 120, *K4, 4.0, 0.05, 1, 2)
        assert lp._lib.dddmr_rollout_set_depth_image_source(lp._ctx, 1, K.C.byref(cfg), K.C.byref(icfg)) == K.ERR_BAD_ARG
        # an unconfigured source
        refused(K.ERR_BAD_ARG, lp.set_depth_image, 1, img, TBO, POSES[0], 10**9)
        with pytest.raises(RolloutError):
            lp.get_depth_image_cloud(1)
        lp.set_depth_image_source(1, ZMIN, ZMAX, 640, 480, *K4b, **node)
        lp.set_depth_image_source(2, ZMIN, ZMAX, 160, 120, *K4, **node)
        lp.set_depth_source(3, ZMIN, ZMAX, 0, max_frame_points=160 * 120, max_frames=1)
        got = lp.set_depth_image(1, big, TBO, POSES[0], 10**9)
        assert got[1:] == (n_big, n_big, n_big)
        one_before = lp.get_depth_image_cloud(1).tobytes()
        # the other kind of frame, both ways
        refused(K.ERR_BAD_ARG, lp.set_depth_frame, 2, fr, Cs.TBS_CAM, POSES[0], 10**9)
        refused(K.ERR_BAD_ARG, lp.set_depth_image, 3, img, TBO, POSES[0], 10**9)
        # a row stride below 2 * width
        before = lp.get_cloud().tobytes()
        rc = lp._lib.dddmr_rollout_set_depth_image(lp._ctx, 2, img.ctypes.data, 2 * 160 - 2, pose, pose, 0, None, None, None, None)
        assert rc == K.ERR_BAD_ARG and lp.get_cloud().tobytes() == before
        # the aggregate would exceed max_points: refused after the device work, and nothing of it stays
        refused(K.ERR_CAPACITY, lp.set_depth_image, 2, img, TBO, POSES[0], 10**9)
        assert len(lp.get_depth_image_cloud(2)) == 0 and lp.get_depth_image_cloud(1).tobytes() == one_before
        # lidar calls on an image source
        scan = scenes.lidar_scan(scenes.cloud_c2(), seed=1)[:500]
        refused(K.ERR_BAD_ARG, lp.set_scan_source, 1, scan, TBS_LIDAR, IDENT, 10.0, 2.0)
        # a smaller image then succeeds on the same source, nothing of the refused one left behind
        few = np.zeros_like(img)
        few[40:80, 40:120] = img[40:80, 40:120]
        n_few = len(I.observation(few, K4, TBO, POSES[0], ZMIN, ZMAX, **node))
        assert 0 < n_few < n_small // 2
        got = lp.set_depth_image(2, few, TBO, POSES[0], 10**9 + MS)
        assert got[1:] == (n_few, n_few, n_big + n_few)
        # re-configuring as a cloud source empties it, and it then takes clouds, not images
        lp.set_depth_source(2, ZMIN, ZMAX, 0, max_frame_points=160 * 120, max_frames=1)
        assert len(lp.get_cloud()) == n_big
        refused(K.ERR_BAD_ARG, lp.set_depth_image, 2, few, TBO, POSES[0], 10**9 + 2 * MS)


# ---- 6. a tick on it -------------------------------------------------------------------------------------------------
def test_tick_on_image_fed_aggregate_equals_tick_on_the_same_points():
    sc = scenes.bench_scene("C2")
    scan = scenes.lidar_scan(sc.cloud, seed=9)
    img, K4 = scenes.depth_image(sc.cloud, R.compose(IDENT, Cs.TBS_CAM), 640, 480, 1.5, 1.0, 8.0, seed=9)
    name = sc.theory.name.decode()
    with LocalPlanner([sc.theory], max_points=200_000) as lp:
        lp.setPlan(sc.plan)
        # the camera sits inside the height band and inside the robot's footprint: kept literally, the point (0, 0, 0)
        # that the pixels without a return become makes every trajectory collide, so this planner drops them
        source(lp, 1, img, K4, Cs.DEFAULTS, drop_zero=True)
        n_lid, _ = lp.set_scan_source(0, scan, TBS_LIDAR, IDENT, 10.0, 2.0)
        n_cam, n_frame, _, n_all = lp.set_depth_image(1, img, TBO, IDENT, 10**9)
        assert n_frame > 1000 and n_all == n_lid + n_frame
        fed = lp.get_cloud().copy()
        r1 = lp.tick(name, sc.tick)
        c1 = lp.debug()[0].copy()
    with LocalPlanner([sc.theory], max_points=200_000) as lp:
        lp.setPlan(sc.plan)
        lp.set_cloud(fed)
        r2 = lp.tick(name, sc.tick)
        c2 = lp.debug()[0].copy()
    assert np.array_equal(c1, c2)
    assert (r1.best_index, r1.best_cost, r1.vx, r1.wz) == (r2.best_index, r2.best_cost, r2.vx, r2.wz)
    assert (c1 == -1.0).any() and (c1 >= 0).any()
