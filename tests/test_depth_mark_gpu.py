"""GPU parity of the depth camera's selfMark slice (depth_mark_create / depth_mark_clusters) against the NumPy / SciPy
restatement (tests/helpers/depth_mark_ref.py).

As in test_depth_clear_gpu.py the restatement is given the observation the device holds (get_cloud, the depth sources'
part of it when a lidar is present).  Counts, voxel keys, sizes, offsets are integers and must be EQUAL; centroids,
downsampled points and the plane are floats and must be BIT-equal (sequential float sums in the same order, nothing
contracted).  The cluster order must be the restatement's, except that a run of clusters of equal size (whose order is
libstdc++'s introsort's) is compared as a set.  The cases and their margins: tests/helpers/depth_mark_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, configs, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_clear_cases as dcases  # noqa: E402
import depth_frustum_ref as R  # noqa: E402
import depth_mark_cases as cases  # noqa: E402
import depth_mark_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("n_observation", "n_clusters", "n_ground_rejected", "n_static_rejected", "n_outside_frustums", "n_accepted", "n_points")


def planner(max_points=200_000):
    return LocalPlanner([configs.bench_theory("C2")], max_points=max_points)


def configure(lp, case):
    for i in range(case.cams):
        sid = case.first_source + i
        if case.kind == "image" and case.few is None:
            k4 = next(st["K4"] for st in cases.built(case.name)[1] if st["kind"] == "image")
            lp.set_depth_image_source(sid, dcases.Z_MIN, dcases.Z_MAX, case.width, case.height, *k4, observation_persistence_ns=case.persistence_ns,
                                      max_frames=case.max_frames, **cases.IMAGE_NODE)
        else:
            lp.set_depth_source(sid, dcases.Z_MIN, dcases.Z_MAX, case.persistence_ns, max_frame_points=case.width * case.height,
                                max_frames=case.max_frames)


def feed(lp, st, frustum=True):
    """one feed step; -> points of a lidar step, else None"""
    if st["kind"] == "lidar":
        return lp.set_scan_source(st["sid"], st["data"], st["t_bs"], st["t_gb"], 5.0, 2.0)[0]
    if st["kind"] == "image":
        lp.set_depth_image(st["sid"], st["data"], st["t_bs"], st["t_gb"], st["stamp"])
    else:
        lp.set_depth_frame(st["sid"], st["data"], st["t_bs"], st["t_gb"], st["stamp"])
    if frustum:
        lp.set_depth_frustum(st["sid"], dcases.FOV_W, dcases.FOV_V, dcases.D_MIN, dcases.D_MAX, st["m2s"])
    return None


def create(lp, case, ground, smap, max_obs=1 << 16):
    lp.depth_mark_create(case.res, case.hres, ground, smap, tolerance=case.tol, min_cluster_size=case.min_size,
                         segmentation_ignore_ratio=case.ratio, max_observation_points=max_obs)


def setup(lp, name):
    """configure, feed and create one case -> (case, frustums, device observation, ground, map)"""
    case, steps, _, frs, _, ground, smap, _ = cases.built(name)
    configure(lp, case)
    n_lidar = 0
    for st in steps:
        n_lidar += feed(lp, st) or 0
    create(lp, case, ground, smap)
    obs = lp.get_cloud()[n_lidar:, :3]                   # the aggregate is in source order: lidar first
    return case, frs, obs, ground, smap


def as_items(cen, vox, size, off, pts):
    return [(int(size[i]), cen[i].tobytes(), vox[i].tobytes(), pts[off[i]:off[i + 1]].tobytes()) for i in range(len(size))]


def assert_equal(got, ref, what=""):
    cen, vox, size, off, pts, plane, st = got
    want = {k: ref["stats"][k] for k in STAT_FIELDS}
    have = {k: int(getattr(st, k)) for k in STAT_FIELDS}
    print(f"{what}: device {have}, launches {st.launches}")
    assert have == want
    assert off[0] == 0 and len(off) == len(size) + 1 and int(off[-1]) == len(pts) == want["n_points"]
    assert np.all(np.diff(size.astype(np.int64)) <= 0)                 # sizes are non-increasing
    np.testing.assert_array_equal(plane.view(np.uint32), ref["plane"].view(np.uint32))
    r_cen, r_vox, r_size, r_off, r_pts = M.packed(ref)
    np.testing.assert_array_equal(size, r_size)
    a, b = as_items(cen, vox, size, off, pts), as_items(r_cen, r_vox, r_size, r_off, r_pts)
    # the order is the restatement's; a run of equal sizes is compared as a set
    assert sorted(a, key=lambda t: (-t[0],) + t[1:]) == sorted(b, key=lambda t: (-t[0],) + t[1:])
    singles = [i for i in range(len(size)) if (size == size[i]).sum() == 1]
    assert [a[i] for i in singles] == [b[i] for i in singles]


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_case_equals_the_restatement(name):
    with planner() as lp:
        case, frs, obs, ground, smap = setup(lp, name)
        got = lp.depth_mark_clusters(case.t_gb)
    ref = cases.restate(case, frs, obs, ground, smap)
    assert_equal(got, ref, name)
    if name == "few_points":
        assert len(obs) <= 5 and got[6].n_accepted == 0
    else:
        assert got[6].n_accepted > 0
    if name == "lidar_beside":
        assert len(obs) < len(cases.built(name)[1][0]["data"]) + len(obs)      # a lidar was fed beside the cameras
    if name == "contested_voxels":
        assert len(np.unique(got[1], axis=0)) < len(got[1])              # two accepted clusters in one voxel


def raw_call(lp, t_gb, cap_c, cap_p, fill=0xAB):
    """the C entry with buffers of its own, pre-filled -> (code, buffers, stats)"""
    bufs = [np.full(max(3 * cap_c, 1) * 4, fill, np.uint8), np.full(max(3 * cap_c, 1) * 4, fill, np.uint8), np.full(max(cap_c, 1) * 4, fill, np.uint8),
            np.full((cap_c + 1) * 4, fill, np.uint8), np.full(max(3 * cap_p, 1) * 4, fill, np.uint8), np.full(16, fill, np.uint8)]
    st = K.DepthMarkStats()
    tgb = (C.c_double * 7)(*[float(v) for v in t_gb])
    rc = lp._lib.dddmr_rollout_depth_mark_clusters(lp._ctx, tgb, cap_c, cap_p, *[b.ctypes.data for b in bufs], C.byref(st))
    return rc, bufs, st


def count_only(lp, t_gb):
    """the C entry with every output but stats NULL -> (code, stats)"""
    st = K.DepthMarkStats()
    tgb = (C.c_double * 7)(*[float(v) for v in t_gb])
    return lp._lib.dddmr_rollout_depth_mark_clusters(lp._ctx, tgb, 0, 0, None, None, None, None, None, None, C.byref(st)), st


def test_refusals_leave_a_following_call_equal_to_the_restatement():
    case, steps, _, frs, _, ground, smap, _ = cases.built("two_cameras")

    def refused(code, fn, *a):
        with pytest.raises(RolloutError) as e:
            fn(*a)
        assert e.value.code == code, e.value

    with planner() as lp:
        refused(K.ERR_STATE, lp.depth_mark_clusters, case.t_gb)             # before create
        create(lp, case, ground, smap)
        refused(K.ERR_STATE, lp.depth_mark_clusters, case.t_gb)             # no depth source
        configure(lp, case)
        feed(lp, steps[0])
        feed(lp, steps[1], frustum=False)
        refused(K.ERR_STATE, lp.depth_mark_clusters, case.t_gb)             # source 1 has no frustum yet
        feed(lp, steps[1])
        obs = lp.get_cloud()[:, :3]
        ref = cases.restate(case, frs, obs, ground, smap)
        assert_equal(lp.depth_mark_clusters(case.t_gb), ref, "after the state refusals")
        # bad arguments
        refused(K.ERR_BAD_ARG, lp.depth_mark_create, 0.0, 0.05, ground, smap)
        refused(K.ERR_BAD_ARG, lp.depth_mark_create, 0.05, 0.05, ground, smap, -1.0)
        refused(K.ERR_CAPACITY, lp.depth_mark_create, 0.05, 0.05, ground, smap, 0.1, 1, 0.5, (1 << 20) + 1)
        st = K.DepthMarkStats()
        tgb = (C.c_double * 7)(*[float(v) for v in case.t_gb])
        one = np.zeros(4, np.float32)
        assert lp._lib.dddmr_rollout_depth_mark_clusters(lp._ctx, tgb, 0, 0, one.ctypes.data, None, None, None, None, None, C.byref(st)) == K.ERR_BAD_ARG
        assert lp._lib.dddmr_rollout_depth_mark_clusters(lp._ctx, tgb, 0, 0, None, None, None, None, None, None, None) == K.ERR_BAD_ARG
        # capacity one short in clusters, then in points: outputs untouched, stats say what is needed
        n_c, n_p = ref["stats"]["n_accepted"], ref["stats"]["n_points"]
        for cap_c, cap_p in ((n_c - 1, n_p), (n_c, n_p - 1)):
            rc, bufs, st = raw_call(lp, case.t_gb, cap_c, cap_p)
            assert rc == K.ERR_CAPACITY and (st.n_accepted, st.n_points) == (n_c, n_p)
            assert all((b == 0xAB).all() for b in bufs)
        rc, bufs, st = raw_call(lp, case.t_gb, n_c, n_p)
        assert rc == K.OK and not (bufs[3] == 0xAB).all()
        assert_equal(lp.depth_mark_clusters(case.t_gb), ref, "after the capacity refusals")
        # an observation above max_observation_points
        create(lp, case, ground, smap, max_obs=len(obs) - 1)
        refused(K.ERR_CAPACITY, lp.depth_mark_clusters, case.t_gb)
        create(lp, case, ground, smap, max_obs=len(obs))
        assert_equal(lp.depth_mark_clusters(case.t_gb), ref, "after the observation refusal")
        np.testing.assert_array_equal(lp.get_cloud()[:, :3], obs)


def test_between_tick_begin_and_tick_end_the_answer_is_the_serial_one():
    sc = scenes.bench_scene("C2")
    with planner() as lp:
        case, frs, obs, ground, smap = setup(lp, "two_cameras")
        ref = cases.restate(case, frs, obs, ground, smap)
        lp.setPlan(sc.plan)
        serial = lp.tick(sc.theory.name.decode(), sc.tick)
        lp.tick_begin(sc.theory.name.decode(), sc.tick)
        got = lp.depth_mark_clusters(case.t_gb)
        res = lp.tick_end()
    assert_equal(got, ref, "inside a pending tick")
    assert res.best_index == serial.best_index and res.best_cost == serial.best_cost


def test_alternating_with_the_clearing_verdicts_over_several_frames():
    """the two calls share the observation grid: whichever comes first after a frame builds it, the other does not"""
    case, steps, _, _, _, ground, smap, _ = cases.built("three_alive_frames")
    with planner() as lp:
        configure(lp, case)
        create(lp, case, ground, smap)
        bare = None
        for k, st in enumerate(steps):
            feed(lp, st)
            fr = [R.Frustum(dcases.FOV_W, dcases.FOV_V, dcases.D_MIN, dcases.D_MAX, st["m2s"])]
            obs = lp.get_cloud()[:, :3]
            t_gb = st["t_gb"]
            ref = M.self_mark(fr, obs, ground, smap, case.res, case.hres, case.tol, case.min_size, case.ratio, t_gb)
            vox, off, cl, verdict, engaged, _ = dcases.draw(fr, obs, t_gb[:3], 400, 500 + k, dcases.anchors_of(t_gb, case.rig))
            if k % 2 == 0:                                   # the verdicts first, then the clusters twice
                got_v, got_e = lp.depth_clear_verdicts(dcases.RES, dcases.HRES, vox, off, cl)
                assert lp.depth_clear_launches() > 1
                got = lp.depth_mark_clusters(t_gb)
                bare = got[6].launches
            else:                                            # the clusters first: the count-only call builds the grid,
                rc, first = count_only(lp, t_gb)                 # which is the call depth_mark_clusters itself begins with
                assert rc == K.OK and bare is not None and first.launches > bare
                got = lp.depth_mark_clusters(t_gb)
                assert got[6].launches == bare
                got_v, got_e = lp.depth_clear_verdicts(dcases.RES, dcases.HRES, vox, off, cl)
                assert lp.depth_clear_launches() == 1
            assert_equal(got, ref, f"frame {k}")
            np.testing.assert_array_equal(got_v, verdict)
            np.testing.assert_array_equal(got_e, engaged)
            again = lp.depth_mark_clusters(t_gb)
            assert again[6].launches == bare
            assert_equal(again, ref, f"frame {k} again")
