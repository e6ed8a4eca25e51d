"""CPU tests of the depth image path: the ABI and its mirrors exist, the NumPy restatement of
DepthImg2PointCloud::cbDepthImg (tests/helpers/depth_image_ref.py) gives answers worked out by hand here,
scenes.depth_image agrees with scenes.depth_frame, feedDepthImage() passes its arguments on, and the end-to-end cases of
the GPU test have their height limits where the reference is decided."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

from dddmr_navigation_amd import _capi as K, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_feed_ref as R  # noqa: E402
import depth_image_ref as I  # noqa: E402
import depth_image_cases as Cs  # noqa: E402

f32, f64 = np.float32, np.float64
K4 = (421.5, 420.25, 423.7, 239.3)            # fx, fy, cx, cy


def test_abi_and_mirrors_have_the_three_calls():
    lib = K.load_library()
    for sym in ("dddmr_rollout_set_depth_image_source", "dddmr_rollout_set_depth_image", "dddmr_rollout_get_depth_image_cloud"):
        assert sym in K.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert C.sizeof(K.DepthImageConfig) == lib.dddmr_rollout_sizeof(9) == 64
    assert C.sizeof(K.DepthSourceConfig) == lib.dddmr_rollout_sizeof(8)
    for m in ("set_depth_image_source", "set_depth_image", "get_depth_image_cloud"):
        assert callable(getattr(LocalPlanner, m))
    hpp = open(os.path.join(ROOT, "include", "dddmr_rollout.hpp")).read()
    for m in ("setDepthImageSource", "setDepthImage", "getDepthImageCloud"):
        assert m + "(" in hpp, m
    # a null context is refused before anything else is looked at
    assert lib.dddmr_rollout_set_depth_image_source(None, 0, None, None) == K.ERR_BAD_ARG
    assert lib.dddmr_rollout_set_depth_image(None, 0, None, 0, None, None, 0, None, None, None, None) == K.ERR_BAD_ARG
    assert lib.dddmr_rollout_get_depth_image_cloud(None, 0, None, 0, None) == K.ERR_BAD_ARG


def one_pixel(u, v, d, width=8, height=6):
    img = np.zeros((height, width), np.uint16)
    img[v, u] = d
    return img


def test_one_pixel_to_the_float():
    u, v, d = 5, 3, 1234
    p = I.deproject(one_pixel(u, v, d), K4, max_distance=4.0, sample_step=1, drop_zero=True)
    assert p.shape == (1, 3) and p.dtype == f32
    # by hand, with the node's types: float cx, cy; float fx = 1.0f / K[0] (a double division); float z = d * 0.001
    cx, cy = f32(423.7), f32(239.3)
    fx, fy = f32(1.0 / 421.5), f32(1.0 / 420.25)
    z = f32(1234 * 0.001)
    x = f32(f32(f32(5.0) - cx) * z) * fx
    y = f32(f32(f32(3.0) - cy) * z) * fy
    assert (p[0, 0], p[0, 1], p[0, 2]) == (f32(x), f32(y), z)
    # the float of 1 / 421.5 is not the float of 1 / (float)421.5 ... for some K it is; this K[0] = 0.1 shows the double division
    assert I.intrinsics((0.1, 0.1, 0, 0))[2] == f32(1.0 / 0.1) == f32(10.0)
    assert f32(1.0) / f32(0.1) == f32(10.0)                       # (same here; the cast that matters is tested next)
    k0 = 3.0000001                                                # not a float: float(k0) = 3.0
    assert I.intrinsics((k0, k0, 0, 0))[2] == f32(1.0 / k0) and f32(1.0 / k0) != f32(1.0) / f32(k0)


def test_depth_is_scaled_in_double_then_rounded_to_float():
    # 1234 * 0.001 in double = 1.2340000000000000(2), rounded to float; the float product 1234.0f * 0.001f differs
    ds = np.arange(1, 65536, dtype=np.uint16)
    img = ds.reshape(1, -1)
    p = I.deproject(img, (1.0, 1.0, 0.0, 0.0), max_distance=100.0, sample_step=1)
    want = np.array([f32(int(d) * 0.001) for d in ds[:5000]], dtype=f32)
    assert np.array_equal(p[:5000, 2], want)
    in_float = ds.astype(f32) * f32(0.001)
    assert (p[:, 2] != in_float).sum() > 1000                      # the two roundings differ for many depths ...
    assert p[3, 2] == f32(0.004) and in_float[3] == f32(0.004)     # ... not for all


def test_max_distance_is_strict_and_compared_in_double():
    # z > max_distance with z a float and max_distance a double.  4.0 is a float: depth 4000 gives z = 4.0f, kept.
    img = np.array([[3999, 4000, 4001]], np.uint16)
    p = I.deproject(img, (1.0, 1.0, 0.0, 0.0), max_distance=4.0, sample_step=1)
    assert list(p[:, 2]) == [f32(3.999), f32(4.0)]
    # 4.1 is not a float: (float)4.1 = 4.099999904..., below the double 4.1: depth 4100 is kept, and would also be kept
    # by a float comparison; 4.3 rounds UP in float ((float)4.3 = 4.30000019...): depth 4300 is dropped by the node's
    # double comparison although its millimetres equal max_distance, and a float comparison would have kept it
    assert float(f32(4.1)) < 4.1 and float(f32(4.3)) > 4.3
    one = lambda d, m: len(I.deproject(np.array([[d]], np.uint16), (1.0, 1.0, 0.0, 0.0), max_distance=m, sample_step=1))
    assert one(4100, 4.1) == 1 and one(4101, 4.1) == 0
    assert one(4300, 4.3) == 0 and one(4299, 4.3) == 1
    assert not (f32(4.3) > f32(4.3))                               # what a float comparison would have said


def test_sample_step_three_on_a_width_that_is_no_multiple():
    img = np.arange(1, 1 + 5 * 8, dtype=np.uint16).reshape(5, 8) * 100      # width 8, height 5: u = 0 3 6, v = 0 3
    p = I.deproject(img, (1.0, 1.0, 0.0, 0.0), max_distance=100.0, sample_step=3)
    assert len(p) == 6
    zs = [f32(int(img[v, u]) * 0.001) for v in (0, 3) for u in (0, 3, 6)]
    assert list(p[:, 2]) == zs                                     # rows outer, columns inner: the node's push_back order
    # fx = fy = 1, cx = cy = 0: x = u * z, y = v * z
    assert list(p[:, 0]) == [f32(u) * z for (u, z) in zip((0, 3, 6, 0, 3, 6), zs)]
    assert list(p[:, 1]) == [f32(v) * z for (v, z) in zip((0, 0, 0, 3, 3, 3), zs)]


def test_padded_row_stride():
    width, height, stride = 6, 4, 2 * 6 + 10
    buf = bytearray(b"\xAB" * (stride * height))                   # the padding is not zero
    rows = np.arange(1, 1 + width * height, dtype=np.uint16).reshape(height, width) * 50
    for v in range(height):
        buf[v * stride:v * stride + 2 * width] = rows[v].tobytes()
    img = I.image_rows(bytes(buf), width, height, stride)
    assert np.array_equal(img, rows)
    a = I.deproject(img, K4, 4.0, 1)
    b = I.deproject(rows, K4, 4.0, 1)
    assert np.array_equal(a, b) and len(a) == width * height


def test_all_zero_image_is_one_point_at_the_origin():
    img = np.zeros((48, 64), np.uint16)
    p = I.deproject(img, K4, 4.0, 2)
    assert p.shape == (24 * 32, 3) and not p.any()                  # every pixel is kept, as (+-0, +-0, 0)
    c = I.stage_one(img, K4, 4.0, 0.05, 2)
    assert c.shape == (1, 3) and not c.any()
    assert I.stage_one(img, K4, 4.0, 0.05, 2, drop_zero=True).shape == (0, 3)
    # a zero pixel and a 1 mm pixel right of and below the principal point share voxel (0, 0, 0): one centroid, the mean
    img = np.zeros((480, 848), np.uint16)
    img[300, 500] = 1
    c = I.stage_one(img, K4, 4.0, 0.05, 1)
    assert c.shape == (1, 3) and 0 < c[0, 2] < 1e-8


def test_inverse_leaf_in_float():
    # pcl::VoxelGrid::setLeafSize stores floats; inverse_leaf_size = 1.0f / leaf
    assert f32(1.0) / f32(0.05) == f32(20.0) and f32(1.0) / f32(0.1) == f32(10.0)
    assert 1.0 / float(f32(0.05)) != 20.0                           # only the float division lands on 20 exactly
    pts = np.array([[0.05, 0.1, 0.15], [0.049999997, 0.099999994, 0.14999999]], f32)
    assert R.voxel_keys(pts, 0.05).tolist() == [[1, 2, 3], [0, 1, 2]]
    assert R.voxel_keys(pts, 0.1).tolist() == [[0, 1, 1], [0, 0, 1]]


def test_tolerance_helper_takes_both_summation_orders():
    img, K4r = Cs.render(160, 120, 0, 1)
    fwd, tol, spread = I.stage_one_tolerance(img, K4r, 4.0, 0.05, 1)
    assert np.array_equal(fwd, I.stage_one(img, K4r, 4.0, 0.05, 1))
    assert 0 < spread < 1e-4 and tol == max(1e-5, 2 * spread)


def test_depth_image_is_deterministic_and_matches_depth_frame():
    cloud = scenes.cloud_c2()
    tgs = R.compose(Cs.POSES[0], Cs.TBS_CAM)
    a, Ka = scenes.depth_image(cloud, tgs, 160, 120, 1.5, 1.0, 8.0, seed=5)
    b, Kb = scenes.depth_image(cloud, tgs, 160, 120, 1.5, 1.0, 8.0, seed=5)
    assert a.dtype == np.uint16 and a.shape == (120, 160) and np.array_equal(a, b) and Ka == Kb
    assert Ka[2:] == (79.5, 59.5)
    assert not np.array_equal(a, scenes.depth_image(cloud, tgs, 160, 120, 1.5, 1.0, 8.0, seed=6)[0])
    fr = scenes.depth_frame(cloud, tgs, 160, 120, 1.5, 1.0, 8.0, seed=5)
    hit = np.isfinite(fr).all(axis=1)
    assert np.array_equal(hit, a.ravel() != 0) and 1000 < hit.sum() < 160 * 120
    p = I.deproject(a, Ka, max_distance=100.0, sample_step=1)
    assert len(p) == 160 * 120
    # optical (z forward, x right, y down) -> camera_link (x forward, y left, z up) with the fixed rotation
    link = R.transform(p, scenes.T_LINK_OPTICAL)
    assert np.array_equal(link, np.stack([p[:, 2], -p[:, 0], -p[:, 1]], axis=1))
    # depth is quantised to 1 mm: at most 0.5 mm along the axis, and that times the ray's slope (< 1) sideways
    err = np.abs(link[hit].astype(f64) - fr[hit].astype(f64))
    assert err[:, 0].max() <= 0.5e-3 + 1e-6 and err[:, 1:].max() <= 0.5e-3 + 1e-6
    assert not link[~hit].any()


def test_depth_image_bridge_compiles_and_behaves_without_ros():
    """feedDepthImage() of perception_bridge.h against a fake C-ABI (tests/cpp/depth_image_bridge_test.cpp)."""
    assert shutil.which("g++") is not None, "needs g++"
    ad = os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "depth_image_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", ad,
                            os.path.join(ROOT, "tests", "cpp", "depth_image_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "depth image bridge OK" in r.stdout, (r.stdout, r.stderr)


def test_end_to_end_cases_have_their_limits_where_the_reference_is_decided():
    """The cases of test_depth_image_gpu.test_end_to_end_where_the_reference_is_decided, on the restatement alone: the
    limits sit in a gap of at least 2e-4 m between the base-frame heights of the reference's stage-one centroids, within
    0.02 m of 0.0 and 2.0, no centroid is closer to a limit than half that gap, and the frame stays below 20000 points."""
    for name, pose, seed, node in Cs.end_to_end_cases():
        img, K4r = Cs.render(848, 480, pose, seed)
        (zmin, zmax), gaps = Cs.end_to_end_band(pose, seed, node)
        print(name, zmin, zmax, gaps)
        assert abs(zmin - 0.0) <= 0.02 and abs(zmax - 2.0) <= 0.02
        assert min(gaps) >= Cs.MIN_GAP, (name, gaps)
        z = R.transform(I.stage_one(img, K4r, **node), Cs.TBO_CAM)[:, 2].astype(f64)
        for lim, gap in zip((zmin, zmax), gaps):
            assert np.abs(z - lim).min() >= 0.5 * gap - 1e-12
        inside = ((z >= zmin) & (z <= zmax)).sum()
        assert 1000 < inside <= R.VOXELIZE_ABOVE and (z < zmin).sum() + (z > zmax).sum() > 0, name
