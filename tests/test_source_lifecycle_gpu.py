"""Sensor sources that are configured again and again during a context's life (csrc/sensor_sources.hip.h): source 1 is a
depth cloud source, then an image source; source 2 a sweep source with its features on and off again (the source table
refuses to turn a depth camera source into a lidar one, so the sweep has a source of its own); and all of that a second
time, while scan source 0 is fed beside them.  Every reconfiguration tears the source's state down and builds the next;
at every step the context must deliver, bit for bit, what a fresh context delivers that only ever saw that step's
configuration.  Likewise the point test's pinned staging, which starts at 64 KiB and is freed and made again when a
call needs more.

The feeds append their points in the order their waves finish, so a cloud is compared as a set of rows (sorted by
their bit patterns); the sweep's images, its cloud and its feature lists have a fixed order and are compared as they
come.  The cases are the smallest of tests/helpers/*_cases.py that leave no product empty."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import configs, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_clear_cases as Dc  # noqa: E402
import depth_image_cases as Di  # noqa: E402
import lidar_features_cases as Lf  # noqa: E402

pytestmark = pytest.mark.gpu

T_BS_LIDAR = (0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0)
T_GB = Dc.base_pose(np.zeros(3))
STAMP = 10**9
MAX_POINTS = 1 << 16
SWEEP = "16x64-g7-m0.2"     # the smallest sweep case whose feature lists are not empty (4x8-g1 has none)


def planner():
    return LocalPlanner([configs.bench_theory("C2")], max_points=MAX_POINTS)


def rows(a):
    """the rows of a float32 array as a set: sorted by their bit patterns"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(len(a), a.shape[1])
    return bits[np.lexsort(bits.T[::-1])]


def aggregate(lp, held, sid, n_scan, n_src, n_all):
    """The aggregate is in source order.  held: the points sources 1 and 2 held before this step; source sid now holds n_src
    -> the rows of scan source 0 and of source sid, and the aggregate's size without the other source's points."""
    held[sid] = n_src
    cloud = lp.get_cloud()
    assert len(cloud) == n_all == n_scan + held[1] + held[2]
    at = n_scan + (held[1] if sid == 2 else 0)
    return dict(scan=rows(cloud[:n_scan]), points=rows(cloud[at: at + n_src]), n_own=np.array([n_all - held[3 - sid]]))


def scan(lp, seed):
    n_scan, _ = lp.set_scan_source(0, scenes.lidar_scan(scenes.cloud_c2(), seed=seed)[:4000], T_BS_LIDAR, T_GB, 5.0, 2.0)
    assert n_scan > 100
    return n_scan


def step_depth_cloud(lp, held):
    t_bc = Dc.T_BASE_CAM[0]
    n_scan = scan(lp, 1)
    lp.set_depth_source(1, Dc.Z_MIN, Dc.Z_MAX, 0, max_frame_points=160 * 120, max_frames=1)
    n_frame, n_src, n_all = lp.set_depth_frame(1, Dc.render(scenes.cloud_c2(), T_GB, t_bc, 5), t_bc, T_GB, STAMP)
    assert n_frame == n_src > 100
    return dict(counts=np.array([n_scan, n_frame, n_src]), **aggregate(lp, held, 1, n_scan, n_src, n_all))


def step_depth_image(lp, held):
    img, k4 = Di.render(160, 120, 0, 1)
    n_scan = scan(lp, 2)
    lp.set_depth_image_source(1, 0.0, 2.0, 160, 120, *k4, max_distance=4.0, leaf_size=0.05, sample_step=1)
    n_cam, n_frame, n_src, n_all = lp.set_depth_image(1, img, Di.TBO_CAM, Di.POSES[0], STAMP)
    one = lp.get_depth_image_cloud(1)
    assert len(one) == n_cam > 100 and n_frame == n_src > 100
    return dict(counts=np.array([n_scan, n_cam, n_frame, n_src]), image_cloud=rows(one), **aggregate(lp, held, 1, n_scan, n_src, n_all))


def step_sweep(lp, held):
    cfg, raw, _, _ = Lf.case(SWEEP)
    a, kw = cfg.planner_args()
    n_scan = scan(lp, 3)
    if held[1]:                                        # what keeps the whole sequence from running on one source
        with pytest.raises(RolloutError, match="is a depth camera source"):
            lp.set_lidar_sweep_source(1, *a, **kw)
    lp.set_lidar_sweep_source(2, *a, **kw)             # (the second time round: empties the sweep source of the first)
    held[2] = 0
    lp.set_lidar_sweep_features(2, Lf.EDGE, Lf.SURF)
    n_seg, n_src, n_all = lp.set_lidar_sweep(2, raw, T_BS_LIDAR, T_GB, 8.0, 2.0)
    assert n_seg > 0
    out = dict(counts=np.array([n_scan, n_seg, n_src]), sweep_cloud=lp.get_lidar_sweep_cloud(2).view(np.uint32),
               **aggregate(lp, held, 2, n_scan, n_src, n_all))
    for name, img in zip(("range", "label", "ground"), lp.get_lidar_sweep_image(2, cfg.V, cfg.H)):
        out[name] = img.view(np.uint32) if img.dtype == np.float32 else img
    for key, v in lp.get_lidar_sweep_segmented(2, cfg.V).items():
        out["segmented_" + key] = v.view(np.uint32) if v.dtype == np.float32 else v
    for which in range(3):
        xyzr, idx = lp.get_lidar_sweep_features(2, which)
        out[f"features_{which}"], out[f"features_{which}_index"] = xyzr.view(np.uint32), idx
    lp.set_lidar_sweep_features(2, enable=False)
    return out


STEPS = (step_depth_cloud, step_depth_image, step_sweep)


def test_reconfigured_source_delivers_what_a_fresh_context_delivers():
    fresh = []
    for step in STEPS:
        with planner() as lp:
            fresh.append(step(lp, {1: 0, 2: 0}))
    assert len(fresh[2]["sweep_cloud"]) == fresh[2]["counts"][1] and fresh[2]["range"].shape == (16, 64)
    assert fresh[2]["counts"][2] > 0 and len(fresh[2]["features_1_index"]) > 5 and len(fresh[2]["segmented_xyz"]) > 100
    with planner() as lp:
        held = {1: 0, 2: 0}
        for round_ in range(2):
            for step, want in zip(STEPS, fresh):
                got = step(lp, held)
                assert got.keys() == want.keys()
                for key in want:
                    np.testing.assert_array_equal(got[key], want[key], err_msg=f"round {round_}, {step.__name__}: {key}")


def test_point_test_staging_grows_and_answers_as_a_fresh_context():
    """12 bytes a point into staging that starts at 64 KiB: 100 points fit, 6 000 need 128 KiB, 30 000 need 512 KiB; the
    6 000-point call that follows runs in the grown buffer."""
    rig = Dc.T_BASE_CAM
    frs = [Dc.frustum(T_GB, t_bc) for t_bc in rig]
    pts, inside, attach, _ = Dc.draw_points([fr for fr, _ in frs], T_GB[:3], 60_000, 9, Dc.anchors_of(T_GB, rig))
    assert len(pts) >= 30_000 and 6_000 * 12 > (1 << 16) and 30_000 * 12 > (1 << 17)

    def configured():
        lp = planner()
        for i, (_, m2s) in enumerate(frs):
            lp.set_depth_source(i, Dc.Z_MIN, Dc.Z_MAX, 0, max_frame_points=64, max_frames=1)
            lp.set_depth_frustum(i, Dc.FOV_W, Dc.FOV_V, Dc.D_MIN, Dc.D_MAX, m2s)
        return lp

    sizes = (100, 6_000, 30_000, 6_000)
    fresh = {}
    for n in set(sizes):
        with configured() as lp:
            fresh[n] = lp.depth_frustum_test(pts[:n])
    with configured() as lp:
        for n in sizes:
            got_in, got_at = lp.depth_frustum_test(pts[:n])
            np.testing.assert_array_equal(got_in, fresh[n][0], err_msg=f"{n} points: in_frustums")
            np.testing.assert_array_equal(got_at, fresh[n][1], err_msg=f"{n} points: attach")
            np.testing.assert_array_equal(got_in, inside[:n])          # ... and both as the restatement answers
            np.testing.assert_array_equal(got_at, attach[:n])
    assert inside[:6_000].any() and not inside[:6_000].all()
