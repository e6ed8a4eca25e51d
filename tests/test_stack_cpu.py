"""Without a GPU: the perception stack's restatement (tests/helpers/stack_ref.py) against hand-written cases, the adequacy
of the sequence tests/test_stack_gpu.py runs (tests/helpers/stack_cases.py) from the restatements alone, the bindings, and
the adapter's PerceptionStackBridge driven by a stand-alone C++ program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from dddmr_navigation_amd import _capi as K
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_layer_ref as L  # noqa: E402
import stack_cases as sc  # noqa: E402
import stack_ref as S  # noqa: E402

ENTRIES = ("create", "set_host_layer", "update", "get_changes", "get_min_dgraph", "get_lethal_mask", "get_lethal_nodes", "reset")
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    for e in ENTRIES:
        assert f"int dddmr_rollout_stack_{e}(" in header
        assert f"dddmr_rollout_stack_{e}" in K.EXPORTED_SYMBOLS
    lib = K.load_library()
    assert C.sizeof(K.StackConfig) == lib.dddmr_rollout_sizeof(15) == 48
    assert C.sizeof(K.StackStats) == lib.dddmr_rollout_sizeof(16) == C.sizeof(K.MarkingStats) + C.sizeof(K.DepthLayerStats) + 24
    assert C.sizeof(K.DepthLayerConfig) == lib.dddmr_rollout_sizeof(13) and C.sizeof(K.DepthLayerStats) == lib.dddmr_rollout_sizeof(14)
    assert f"#define DDDMR_STACK_MAX_LAYERS {K.STACK_MAX_LAYERS}" in header and f"#define DDDMR_STACK_HOST0 {K.STACK_HOST0}" in header


def test_the_minimum_against_hand_written_cases():
    above = 123456.0
    #            node:  0     1      2      3     4      5       6       7        8
    a = np.array([1.0,  NAN,   INF,  -INF,  above, 3.0,    NAN,    S.START, -0.0])
    b = np.array([2.0,  5.0,   7.0,   0.0,  above, 3.0,    NAN,    INF,      0.0])
    want = [1.0,        5.0,   7.0,  -INF,  S.START, 3.0,  S.START, S.START, -0.0]
    v, m = S.stacked([(a, None), (b, None)])
    np.testing.assert_array_equal(bits(v), bits(np.array(want)))
    assert not m.any()
    # node 1: a NaN leaves v alone whichever side it comes from; node 4: a value above 99999.9 comes out as 99999.9;
    # node 5: equal values in two layers; node 8: -0.0 < +0.0 is false, so the FIRST zero stays, bit pattern and all
    v2, _ = S.stacked([(b, None), (a, None)])
    np.testing.assert_array_equal(bits(v2), bits(np.array([1.0, 5.0, 7.0, -INF, S.START, 3.0, S.START, S.START, 0.0])))
    assert bits(v)[8] != bits(v2)[8]
    # an unset slot does not take part, wherever it stands
    for layers in ([(None, None), (a, None), (b, None)], [(a, None), (None, None), (b, None)], [(a, None), (b, None), (None, None)]):
        np.testing.assert_array_equal(bits(S.stacked(layers)[0]), bits(v))
    np.testing.assert_array_equal(S.stacked([(None, None)], n=3)[0], np.full(3, S.START))
    # the vector form against one comparison at a time
    rng = np.random.Generator(np.random.PCG64(3))
    cols = [rng.choice([NAN, INF, -INF, above, 0.0, 1.5, 99999.9, 99999.8], 64) for _ in range(4)]
    vec = S.stacked([(c, None) for c in cols])[0]
    one = np.array([S.scalar_min([c[i] for c in cols]) for i in range(64)])
    np.testing.assert_array_equal(bits(vec), bits(one))


def test_masks_changed_set_and_lethal_nodes_against_hand_written_cases():
    d = np.full(5, 9999.0)
    host = (np.array([1.0, 2.0, NAN, 4.0, 5.0]), None)
    lid = (d, np.array([1, 0, 1, 0, 1], bool))
    dep = (d, np.array([1, 1, 0, 0, 1], bool))
    v, m = S.stacked([host, lid, dep])
    np.testing.assert_array_equal(m, np.array([6, 4, 2, 0, 6], np.uint8))           # bit = position in the order; host bits stay 0
    np.testing.assert_array_equal(S.stacked([lid, host, dep])[1], np.array([5, 4, 1, 0, 5], np.uint8))
    # aggregateLethal: layer by layer, ascending inside a layer, a node lethal in two layers twice; the last node (n_ground) never
    np.testing.assert_array_equal(S.lethal_nodes(m, [1, 2], 4), [0, 2, 0, 1])
    np.testing.assert_array_equal(S.lethal_nodes(m, [2, 1], 4), [0, 1, 0, 2])
    # changed: bit patterns, so NaN -> the same NaN is no change and +0.0 -> -0.0 is one; a mask change alone counts
    before = (np.array([NAN, 0.0, 1.0, 1.0]), np.array([0, 0, 0, 1], np.uint8))
    after = (np.array([NAN, -0.0, 1.0, 1.0]), np.array([0, 0, 2, 1], np.uint8))
    np.testing.assert_array_equal(S.changed(before, after), [1, 2])
    tr = S.Tracker(5)
    tr.publish([host, lid, dep])
    assert len(tr.step([host, lid, dep])) == 0
    mv, mm = tr.values.copy(), tr.mask.copy()
    host2 = (np.array([1.0, 0.5, NAN, 4.0, 5.0]), None)
    ch = tr.step([host2, lid, (d, np.zeros(5, bool))])
    np.testing.assert_array_equal(ch, [0, 1, 4])
    S.apply_changes(mv, mm, ch, tr.values[ch], tr.mask[ch])
    np.testing.assert_array_equal(bits(mv), bits(tr.values))
    np.testing.assert_array_equal(mm, tr.mask)


def test_the_gpu_sequence_is_adequate():
    """asserted from the restatements alone; a seed that does not satisfy it is replaced, the assertions stay"""
    b = sc.built()
    case, ups, ground, depth = b["case"], b["ups"], b["ground"], b["depth"]
    n = len(ground)
    assert 4 <= len(ups) <= 5 and case.cams == 2 and [f["sid"] for f in ups[0]["feeds"]] == [0, 1, 2]
    assert all(u["feeds"][0]["kind"] == "lidar" for u in ups) and len({u["t_gb"] for u in ups}) == len(ups)      # a fresh scan, a moving pose
    assert all(L.margins_kept(r) for r in depth)                           # the depth layer's comparisons keep their margins
    st = b["static"]
    strict = {"static": 0, "lidar": 0, "depth": 0}
    both, small = 0, 0
    for k, u in enumerate(b["updates"]):
        li, de = u["lidar_dgraph"], u["depth_dgraph"]
        with np.errstate(invalid="ignore"):
            s_min = (st < li) & (st < de) & (st < S.START)
            l_min = (li < de) & (li < S.START) & ~(st <= li)
            d_min = (de < li) & (de < S.START) & ~(st <= de)
        # (the stacked value really is that layer's there)
        v = u["stacked"][0]
        assert (v[s_min] == st[s_min]).all() and (v[l_min] == li[l_min]).all() and (v[d_min] == de[d_min]).all()
        strict["static"] += int(s_min.sum()); strict["lidar"] += int(l_min.sum()); strict["depth"] += int(d_min.sum())
        both += int((u["lidar_lethal"] & u["depth_lethal"]).sum())
        small += 0 < len(u["changed"]) < (n + 1) / 10
        print(f"update {k}: {len(u['lidar_obs'])} lidar points, {len(u['changed'])} of {n + 1} nodes changed, strict minima "
              f"{int(s_min.sum())} / {int(l_min.sum())} / {int(d_min.sum())}, lethal in both {int((u['lidar_lethal'] & u['depth_lethal']).sum())}")
        assert len(u["lidar_obs"]) > 5 and u["lidar_stats"].n_marked > 0
    assert all(c > 0 for c in strict.values()), strict                     # each of the three layers is the strict minimum somewhere
    assert both > 0                                                        # some node is lethal in both device layers at once
    assert small >= 2                                                      # change lists that are worth having
    # the lidar restatement fed the whole aggregate ends elsewhere: the "lidar sources only" comparison can fail
    assert b["updates"][-1]["whole_voxels"] != b["updates"][-1]["lidar_voxels"]
    # the host layer's special values are in play
    assert np.isnan(st).any() and np.isinf(st).any() and (st[np.isfinite(st)] > S.START).any()
    # a reset in mid-sequence changes what follows (the reset test compares something)
    r = sc.built(reset_at=sc.RESET_AT)["updates"]
    assert r[sc.RESET_AT]["lidar_voxels"] != b["updates"][sc.RESET_AT]["lidar_voxels"] or \
        not np.array_equal(r[sc.RESET_AT]["stacked"][0], b["updates"][sc.RESET_AT]["stacked"][0])


def test_the_bridge_under_the_sanitizers(tmp_path):
    """PerceptionStackBridge against a fake C ABI: random sequences of change lists, an overflow followed by
    resynchronisation; after every pass the mirror equals the fake's full arrays (the program checks and exits non-zero)"""
    exe = str(tmp_path / "stack_bridge_test")
    inc = [os.path.join(ROOT, "include"), os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror"]
    cmd += [f"-I{i}" for i in inc] + [os.path.join(ROOT, "tests", "cpp", "stack_bridge_test.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    print(out)
    assert "overflows" in out and "all mirrors equal" in out
