"""GPU parity of the lidar sweep path (set_lidar_sweep_source / set_lidar_sweep / get_lidar_sweep_cloud /
get_lidar_sweep_image) against the NumPy restatement of ImageProjection::cloudHandler's front half
(tests/helpers/lidar_sweep_ref.py, whose BFS is the reference's queue, not a union-find).

Stage one is compared bit for bit: every sweep used here has zero fragile decisions by the restatement's own report
(tests/helpers/lidar_sweep_cases.py draws them so; tests/test_lidar_sweep_cpu.py asserts it), and everything else is the
same IEEE operations on both sides.  Stage two is compared against the library's own scan feed given the library's own
stage-one cloud, with the comparison tests/test_feed_gpu.py makes for two feeds."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

from dddmr_navigation_amd import _capi as K, configs, marking, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lidar_sweep_ref as R  # noqa: E402
import lidar_sweep_cases as Cs  # noqa: E402

pytestmark = pytest.mark.gpu

TBS = (0.1, 0.0, 0.6) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.05))
TGB = (1.0, -0.5, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.3))
WINDOW, HEIGHT = 8.0, 1.8


def planner(max_points=200_000):
    return LocalPlanner([configs.bench_theory("C2")], max_points=max_points)


def configure(lp, sid, c, **kw):
    args, kwargs = c.planner_args()
    kwargs.update(kw)
    lp.set_lidar_sweep_source(sid, *args, **kwargs)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sweep(lp, sid, c, raw, tbs=TBS, tgb=TGB):
    counts = lp.set_lidar_sweep(sid, raw, tbs, tgb, WINDOW, HEIGHT)
    rng, lab, gnd = lp.get_lidar_sweep_image(sid, c.V, c.H)
    return counts, rng, lab, gnd, lp.get_lidar_sweep_cloud(sid)


def assert_stage_one(got, ref, what):
    counts, rng, lab, gnd, cloud = got
    assert ref["n_fragile"] == 0, what                             # a condition on the input, checked on the restatement alone
    print(f"{what}: {len(ref['cloud'])} output points, {ref['n_labels']} valid segments, {int(ref['ground'].sum())} ground pixels")
    np.testing.assert_array_equal(bits(rng), bits(ref["range"]), err_msg=what + ": range image")
    np.testing.assert_array_equal(gnd, ref["ground"], err_msg=what + ": ground mask")
    np.testing.assert_array_equal(lab, ref["label"], err_msg=what + ": labels")
    assert counts[0] == len(ref["cloud"]) == len(cloud), (what, counts, len(ref["cloud"]), len(cloud))
    np.testing.assert_array_equal(bits(cloud), bits(ref["cloud"]), err_msg=what + ": output cloud (order, xyz bits, labels)")


def _match(got_xyz, ref_xyz):
    """tests/test_feed_gpu.py's comparison of two feeds"""
    assert len(got_xyz) == len(ref_xyz)
    if len(ref_xyz) == 0:
        return
    d, idx = cKDTree(ref_xyz).query(got_xyz)
    assert d.max() <= 1e-5 and len(np.unique(idx)) == len(ref_xyz)


# ---- 1. stage one, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Cs.NAMES)
def test_stage_one_matches_the_node_bit_for_bit(name):
    c, raw, ref = Cs.case(name)
    assert ref["n_fragile"] == 0
    with planner() as lp:
        configure(lp, 0, c)
        assert_stage_one(sweep(lp, 0, c, raw), ref, name)


@pytest.mark.parametrize("name", sorted(Cs.known_answers()))
def test_stage_one_known_answers(name):
    c, raw = Cs.known_answers()[name]
    ref = R.stage_one(raw, c)
    assert ref["n_fragile"] == 0
    with planner() as lp:
        configure(lp, 1, c)
        assert_stage_one(sweep(lp, 1, c, raw), ref, name)


def test_stage_one_record_strides_and_junk():
    """32-byte records as PCL lays them out, an empty sweep, a sweep of nothing but dropped records"""
    c, raw, ref = Cs.case("16x64-g7-m0.2")
    wide = np.full((len(raw), 8), 7.0, np.float32)
    wide[:, :3] = raw
    with planner() as lp:
        configure(lp, 0, c)
        assert_stage_one(sweep(lp, 0, c, wide), ref, "32-byte records")
        empty = R.stage_one(np.zeros((0, 3), np.float32), c)
        assert_stage_one(sweep(lp, 0, c, np.zeros((0, 3), np.float32)), empty, "empty sweep")
        junk = np.array([[np.nan, 1, 1], [0, 0, 0], [np.inf, 0, 1], [0.01, 0.01, 0.0], [500.0, 0.0, 1.0]], np.float32)
        assert_stage_one(sweep(lp, 0, c, junk), R.stage_one(junk, c), "junk")
        assert len(lp.get_cloud()) == 0
        assert_stage_one(sweep(lp, 0, c, raw), ref, "after junk")


# ---- 2. repeatability: the tables are left clean -----------------------------------------------------------------------
@pytest.mark.parametrize("names", [("16x64-g7-m0.0", "16x64-g15-m0.0"), ("16x1000-g7-m0.2", "16x1000-g7-m0.2-b")])
def test_the_same_sweep_again_gives_the_same_result(names):
    c, raw, ref = Cs.case(names[0])
    other = Cs.case(names[1])[1]
    with planner() as lp:
        configure(lp, 0, c)
        first = sweep(lp, 0, c, raw)
        assert_stage_one(first, ref, "first")
        agg = lp.get_cloud()
        for what, data in (("again", raw), ("another sweep", other), ("the first again", raw)):
            got = sweep(lp, 0, c, data)
            if data is raw:
                assert got[0] == first[0], what
                for a, b in zip(got[1:], first[1:]):
                    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)
                _match(lp.get_cloud()[:, :3], agg[:, :3])
            else:
                assert_stage_one(got, R.stage_one(data, c), what)


# ---- 3. stage two -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4x8-g1", "16x64-g7-m0.2", "16x1000-g7-m0.0", "64x2048-g7-m0.2"])
def test_stage_two_equals_the_scan_feed_of_the_stage_one_cloud(name):
    c, raw, ref = Cs.case(name)
    with planner() as lp:
        configure(lp, 0, c)
        n_seg, n_src, n_all = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        cloud = lp.get_lidar_sweep_cloud(0)
        agg = lp.get_cloud()
    with planner() as lp2:
        want = lp2.set_scan_source(0, np.ascontiguousarray(cloud[:, :3]), TBS, TGB, WINDOW, HEIGHT)
        agg2 = lp2.get_cloud()
    print(f"{name}: {n_seg} segmented points -> {n_src} observation points")
    assert n_seg == len(ref["cloud"]) == len(cloud)
    assert (n_src, n_all) == want == (len(agg), len(agg))
    assert n_src > 0 or name.startswith("4x8")
    _match(agg[:, :3], agg2[:, :3])


def test_a_sweep_source_beside_a_scan_source_and_a_depth_source():
    c, raw, _ = Cs.case("16x440-g7-m0.0")
    scan = scenes.lidar_scan(scenes.cloud_c2(), sensor_xyz=(1.0, -0.5, 0.6), seed=31)
    rng = np.random.default_rng(5)
    frame = np.stack([rng.uniform(0.5, 3.0, 30_000), rng.uniform(-1.5, 1.5, 30_000), rng.uniform(-0.4, 1.0, 30_000)], axis=1).astype(np.float32)
    parts = {}
    with planner() as lp:                                          # each sensor alone
        parts[0] = (lp.set_scan_source(0, scan, TBS, TGB, WINDOW, HEIGHT)[0], lp.get_cloud()[:, :3].copy())
    with planner() as lp:
        configure(lp, 1, c)
        parts[1] = (lp.set_lidar_sweep(1, raw, TBS, TGB, WINDOW, HEIGHT)[1], lp.get_cloud()[:, :3].copy())
    with planner() as lp:
        lp.set_depth_source(2, 0.0, 2.0)
        parts[2] = (lp.set_depth_frame(2, frame, TBS, TGB, 10**9)[1], lp.get_cloud()[:, :3].copy())
    assert all(n > 0 and n == len(p) for n, p in parts.values())
    n0, n1, n2 = (parts[i][0] for i in range(3))
    with planner() as lp:
        configure(lp, 1, c)
        lp.set_depth_source(2, 0.0, 2.0)
        assert lp.set_depth_frame(2, frame, TBS, TGB, 10**9)[1:] == (n2, n2)
        assert lp.set_lidar_sweep(1, raw, TBS, TGB, WINDOW, HEIGHT)[1:] == (n1, n1 + n2)
        assert lp.set_scan_source(0, scan, TBS, TGB, WINDOW, HEIGHT) == (n0, n0 + n1 + n2)
        got = lp.get_cloud()[:, :3]
        _match(got[:n0], parts[0][1])                              # source order, not arrival order
        _match(got[n0:n0 + n1], parts[1][1])
        _match(got[n0 + n1:], parts[2][1])
        half = raw[: len(raw) // 2]                                # the sweep source again: only its part changes
        n_seg, n1b, n_all = lp.set_lidar_sweep(1, half, TBS, TGB, WINDOW, HEIGHT)
        assert n_all == n0 + n1b + n2
        got = lp.get_cloud()[:, :3]
        _match(got[:n0], parts[0][1])
        _match(got[n0 + n1b:], parts[2][1])


# ---- 4. a marking layer over a sweep source ------------------------------------------------------------------------------
def test_marking_layer_over_a_sweep_source():
    c, raw, _ = Cs.case("16x1000-g7-m0.0")
    cfg = marking.shipped_config()
    ground = marking.ground_lattice()
    static_map = np.array([[50.0, 50.0, 0.0]], np.float32)
    voxels = []
    with planner(1 << 16) as lp:
        configure(lp, 0, c)
        n_seg, n_src, _ = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        cloud = lp.get_lidar_sweep_cloud(0)
        layer = marking.MarkingLayer(lp, cfg, ground, static_map)
        st = layer.update(TBS, TGB)                                # raises unless DDDMR_OK
        voxels.append(set(map(tuple, layer.voxels().tolist())))
        n_obs = st.n_observation
    with planner(1 << 16) as lp:
        assert lp.set_scan_source(0, np.ascontiguousarray(cloud[:, :3]), TBS, TGB, WINDOW, HEIGHT)[0] == n_src
        layer = marking.MarkingLayer(lp, cfg, ground, static_map)
        st2 = layer.update(TBS, TGB)
        voxels.append(set(map(tuple, layer.voxels().tolist())))
    print(f"marking over a sweep source: {n_obs} observation points, {len(voxels[0])} voxels")
    assert n_obs == st2.n_observation == n_src and n_src > 100
    assert len(voxels[0]) > 0 and voxels[0] == voxels[1]


# ---- 5. error paths leave the context usable -----------------------------------------------------------------------------
def _refused(code, fn, *a, **kw):
    with pytest.raises(RolloutError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, code, str(e.value))


def test_error_paths_leave_the_context_usable():
    c, raw, ref = Cs.case("16x64-g7-m0.2")
    scan = scenes.lidar_scan(scenes.cloud_c2(), sensor_xyz=(1.0, -0.5, 0.6), seed=32)[:2000]
    args, kw = c.planner_args()
    with planner() as lp:
        # getters and sweeps on sources that are not sweep sources
        _refused(K.ERR_STATE, lp.get_lidar_sweep_cloud, 0)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_image, 0, c.V, c.H)
        _refused(K.ERR_BAD_ARG, lp.set_lidar_sweep, 0, raw, TBS, TGB, WINDOW, HEIGHT)         # not configured
        lp.set_scan_source(1, scan, TBS, TGB, WINDOW, HEIGHT)
        lp.set_depth_source(2, 0.0, 2.0)
        _refused(K.ERR_BAD_ARG, configure, lp, 1, c)                                          # a scan source
        _refused(K.ERR_BAD_ARG, configure, lp, 2, c)                                          # a depth source
        _refused(K.ERR_BAD_ARG, lp.set_lidar_sweep, 1, raw, TBS, TGB, WINDOW, HEIGHT)
        _refused(K.ERR_BAD_ARG, lp.set_lidar_sweep, 2, raw, TBS, TGB, WINDOW, HEIGHT)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_cloud, 1)
        _refused(K.ERR_BAD_ARG, configure, lp, 7, c)
        # configurations
        for bad in (dict(V=1), dict(H=3), dict(gsi=c.V), dict(top=c.bottom), dict(top=c.bottom - 1.0), dict(min_range=c.max_range), dict(flags=2)):
            b = dict(V=c.V, H=c.H, bottom=c.bottom, top=c.top, gsi=c.gsi, min_range=c.min_range, flags=0)
            b.update(bad)
            kw2 = dict(kw, minimum_detection_range=b["min_range"], flags=b["flags"])
            _refused(K.ERR_BAD_ARG, lp.set_lidar_sweep_source, 0, b["V"], b["H"], b["bottom"], b["top"], b["gsi"], **kw2)
        _refused(K.ERR_CAPACITY, lp.set_lidar_sweep_source, 0, 129, 64, c.bottom, c.top, 7, **kw)
        _refused(K.ERR_CAPACITY, lp.set_lidar_sweep_source, 0, 16, 4097, c.bottom, c.top, 7, **kw)
        _refused(K.ERR_CAPACITY, lp.set_lidar_sweep_source, 0, *args, max_sweep_points=(1 << 20) + 1, **kw)
        _refused(K.ERR_STATE, lp.get_lidar_sweep_cloud, 0)                                    # none of them configured it
        agg = lp.get_cloud()

        # a sweep source: before the first sweep the getters report zero points and an empty image
        configure(lp, 0, c, max_sweep_points=len(raw))
        assert len(lp.get_lidar_sweep_cloud(0)) == 0
        rng, lab, gnd = lp.get_lidar_sweep_image(0, c.V, c.H)
        assert (rng == R.FLT_MAX).all() and (lab == -1).all() and (gnd == 0).all()
        np.testing.assert_array_equal(lp.get_cloud(), agg)
        first = sweep(lp, 0, c, raw)
        assert_stage_one(first, ref, "first sweep")
        agg = lp.get_cloud()
        assert len(agg) == first[0][2] > first[0][1] > 0                   # the scan source's part is in it too

        def unchanged(what):
            rng, lab, gnd = lp.get_lidar_sweep_image(0, c.V, c.H)
            for a, b in zip((rng, lab, gnd, lp.get_lidar_sweep_cloud(0)), first[1:]):
                np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)
            np.testing.assert_array_equal(lp.get_cloud(), agg, err_msg=what)

        _refused(K.ERR_CAPACITY, lp.set_lidar_sweep, 0, np.concatenate([raw, raw[:1]]), TBS, TGB, WINDOW, HEIGHT)
        unchanged("a sweep above max_sweep_points")
        _refused(K.ERR_BAD_ARG, lp.set_scan_source, 0, scan, TBS, TGB, WINDOW, HEIGHT)        # another kind of feed
        unchanged("a scan for a sweep source")
        _refused(K.ERR_BAD_ARG, lp.set_scan, scan, TBS, TGB, WINDOW, HEIGHT)                  # plain set_scan means source 0
        _refused(K.ERR_BAD_ARG, lp.set_depth_frame, 0, scan, TBS, TGB, 10**9)
        _refused(K.ERR_BAD_ARG, lp.set_depth_source, 0, 0.0, 2.0)
        _refused(K.ERR_BAD_ARG, lp.set_stitcher_source, 0, 2)
        _refused(K.ERR_BAD_ARG, lp.set_stitcher, 2)
        _refused(K.ERR_CAPACITY, lp.get_lidar_sweep_image, 0, c.V - 1, c.H)
        unchanged("feeds of another kind")
        assert_stage_one(sweep(lp, 0, c, raw[::-1]), R.stage_one(raw[::-1], c), "a good sweep afterwards")
        # re-configuring empties the source: its part of the aggregate goes
        configure(lp, 0, c)
        assert len(lp.get_lidar_sweep_cloud(0)) == 0
        assert len(lp.get_cloud()) == len(agg) - first[0][1]
        assert_stage_one(sweep(lp, 0, c, raw), ref, "after re-configuring")


def test_reconfiguring_a_sweep_source_releases_all_of_it():
    """Configuring a configured sweep source tears the old one down as a whole: its segment leaves the aggregate, its
    features are off and its range image reads as never projected."""
    c, raw, ref = Cs.case("4x8-g1")
    with planner() as lp:
        configure(lp, 0, c)
        lp.set_lidar_sweep_features(0, 0.1, 0.1)
        n_seg, n_src, n_all = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
        assert n_seg == len(ref["cloud"]) > 0 and n_src == n_all == len(lp.get_cloud()) > 0
        assert lp.get_lidar_sweep_features(0, 1) is not None                                  # on, and answering
        assert not (lp.get_lidar_sweep_image(0, c.V, c.H)[0] == R.FLT_MAX).all()
        configure(lp, 0, c)
        assert len(lp.get_cloud()) == 0 and len(lp.get_lidar_sweep_cloud(0)) == 0
        with pytest.raises(RolloutError) as e:
            lp.get_lidar_sweep_features(0, 1)
        assert e.value.code == K.ERR_STATE and "features of source 0 are off" in str(e.value)
        rng, lab, gnd = lp.get_lidar_sweep_image(0, c.V, c.H)
        assert (rng == R.FLT_MAX).all() and (lab == -1).all() and (gnd == 0).all()


def test_an_aggregate_above_max_points_refuses_the_sweep_and_changes_nothing():
    c, raw, ref = Cs.case("16x64-g7-m0.2")
    small = raw[: len(raw) // 4]
    with planner() as lp:
        configure(lp, 0, c)
        n_small = lp.set_lidar_sweep(0, small, TBS, TGB, WINDOW, HEIGHT)[1]
        n_full = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)[1]
    assert 0 < n_small < n_full
    with planner(max_points=n_full - 1) as lp:
        configure(lp, 0, c)
        _refused(K.ERR_CAPACITY, lp.set_lidar_sweep, 0, raw, TBS, TGB, WINDOW, HEIGHT)
        assert len(lp.get_lidar_sweep_cloud(0)) == 0 and len(lp.get_cloud()) == 0
        first = sweep(lp, 0, c, small)
        assert_stage_one(first, R.stage_one(small, c), "the small sweep")
        agg = lp.get_cloud()
        assert len(agg) == n_small
        _refused(K.ERR_CAPACITY, lp.set_lidar_sweep, 0, raw, TBS, TGB, WINDOW, HEIGHT)
        rng, lab, gnd = lp.get_lidar_sweep_image(0, c.V, c.H)
        for a, b in zip((rng, lab, gnd, lp.get_lidar_sweep_cloud(0)), first[1:]):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
        np.testing.assert_array_equal(lp.get_cloud(), agg)
        again = sweep(lp, 0, c, small)                             # the tables were left clean by the refused sweep
        assert_stage_one(again, R.stage_one(small, c), "the small sweep again")
