"""The wave and workgroup primitives of csrc/wave_ops.hip.h, through their one entry point (selftest_wave_ops: a single
workgroup of 256 lanes, the lanes at or past n taking part with value 0 and a clear flag), against NumPy bit for bit.
Sums wrap as their integer type does.  The four waves race for the append's counter, so of the append only what is
guaranteed is asserted: inside a wave the keeping lanes hold consecutive ascending indices, the waves' ranges are
disjoint and tile [base, base + count), the final counter is base + count; a lane that does not keep is not looked at.

Sizes: one lane, a wave less one, a wave, a wave and one, the workgroup less one, the workgroup, and nothing at all.

What that workgroup of 256 lanes with unsigned values cannot show goes through selftest_wave_wide: block_excl_scan<16>
with wave_last in one workgroup of 1024 lanes, the reductions on the other types, and last_block's hand-off.  The
(operation, type) pairs a kernel of csrc/ instantiates, by grep for wave_min / wave_max / wave_sum:
    wave_min  float (mcl_measure, depth_clear: coordinates, negative too), int (marking_fused's block_minmax3),
              unsigned long long (global_plan, global_plan_cloud, mcl_submap)
    wave_max  uint32_t (static_layer), int (marking_fused, mcl_submap), float (depth_clear)
    wave_sum  uint32_t (mcl_measure, lidar_sweep, lidar_features), unsigned long long (static_layer)
selftest_wave_ops holds min / max / sum on uint32_t, min / sum on unsigned long long and min on float from unsigned
values; the pairs it lacks are wave_max on float, wave_min on float over negative and mixed values, and wave_min /
wave_max on int: test_wave_reductions_on_float_and_int.  (Nothing instantiates wave_max on unsigned long long.)"""
import numpy as np
import pytest

from dddmr_navigation_amd import configs
from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError

pytestmark = pytest.mark.gpu

BASE = 1000
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
LANE = np.arange(256) % 64


def _flag_patterns():
    rng = np.random.default_rng(31)
    only = lambda i: np.arange(256) == i
    return {"none": np.zeros(256, bool), "all": np.ones(256, bool), "lane 0": only(0), "lane 63 of wave 1": only(127),
            "alternating": np.arange(256) % 2 == 1, "random": rng.random(256) < 0.4}


def _value_patterns():
    rng = np.random.default_rng(32)
    return {"zero": np.zeros(256, np.uint32), "ones": np.full(256, 0xFFFFFFFF, np.uint32),
            "random": rng.integers(0, 1 << 32, 256, dtype=np.uint32)}


FLAGS, VALUES = _flag_patterns(), _value_patterns()


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C1")]) as p:
        yield p


def _per_wave(x):
    return np.repeat(x, 64)


def _check_append(idx, final, keep, what):
    ranges = []
    for w in range(4):
        k = keep[64 * w:64 * w + 64]
        got = idx[64 * w:64 * w + 64][k].astype(np.int64)
        if got.size:
            assert np.array_equal(got, got[0] + np.arange(got.size)), f"{what}: wave {w} is not consecutive in lane order"
            ranges.append((int(got[0]), got.size))
    at = BASE
    for start, size in sorted(ranges):
        assert start == at, f"{what}: the waves' ranges do not tile [base, base + count)"
        at += size
    assert at == BASE + int(keep.sum()) and int(final) == at, f"{what}: final counter"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256])
def test_wave_ops_against_numpy(lp, n):
    for vname, values in VALUES.items():
        for fname, flags in FLAGS.items():
            what = f"n={n} values={vname} flags={fname}"
            out32, out64 = lp.selftest_wave_ops(values[:n], flags[:n], BASE)
            v = np.zeros(256, np.uint64)
            v[:n] = values[:n]
            keep = np.zeros(256, bool)
            keep[:n] = flags[:n]
            waves = v.reshape(4, 64)
            total = int(v.sum()) & M32
            assert np.array_equal(out32[0], (np.cumsum(waves, axis=1) & M32).ravel()), f"{what}: wave_incl_scan_u32"
            assert np.array_equal(out32[1], (np.cumsum(v) - v) & M32), f"{what}: block_excl_scan"
            assert np.array_equal(out32[2], np.cumsum(keep) - keep), f"{what}: block_rank"
            assert (int(out32[9, 0]), int(out32[9, 1])) == (total, int(keep.sum())), f"{what}: totals"
            _check_append(out32[3], out32[9, 2], keep, what + " (global counter)")
            _check_append(out32[4], out32[9, 3], keep, what + " (LDS counter)")
            assert np.array_equal(out32[5], _per_wave(waves.min(axis=1))), f"{what}: wave_min u32"
            assert np.array_equal(out32[6], _per_wave(waves.max(axis=1))), f"{what}: wave_max u32"
            assert np.array_equal(out32[7], _per_wave(waves.sum(axis=1) & M32)), f"{what}: wave_sum u32"
            fmin = v.astype(np.uint32).astype(np.float32).reshape(4, 64).min(axis=1)
            assert np.array_equal(out32[8], _per_wave(fmin.view(np.uint32))), f"{what}: wave_min float"
            v64 = [(int(x) << 32) | int(l) for x, l in zip(v, LANE)]
            min64 = [min(v64[64 * w:64 * w + 64]) for w in range(4)]
            sum64 = [sum(v64[64 * w:64 * w + 64]) & M64 for w in range(4)]
            assert np.array_equal(out64[0], _per_wave(np.array(min64, np.uint64))), f"{what}: wave_min u64"
            assert np.array_equal(out64[1], _per_wave(np.array(sum64, np.uint64))), f"{what}: wave_sum u64"


def test_wave_ops_refuses_more_than_a_workgroup(lp):
    with pytest.raises(RolloutError):
        lp.selftest_wave_ops(np.zeros(257, np.uint32), np.zeros(257, np.uint8))


# ---- selftest_wave_wide ------------------------------------------------------------------------------------------------
def _wide_values():
    rng = np.random.default_rng(33)
    return {"zero": np.zeros(1024, np.uint32), "ones": np.full(1024, 0xFFFFFFFF, np.uint32),
            "random": rng.integers(0, 1 << 32, 1024, dtype=np.uint32)}


WIDE_VALUES = _wide_values()
LANES = np.arange(64, dtype=np.uint32)


@pytest.mark.parametrize("n", [0, 1, 65, 960, 1023, 1024])
def test_block_scan_of_sixteen_waves(lp, n):
    for vname, values in WIDE_VALUES.items():
        scan, _, misc = lp.selftest_wave_wide(values[:n], LANES, 1)
        v = np.zeros(1024, np.uint64)
        v[:n] = values[:n]
        what = f"n={n} values={vname}"
        assert np.array_equal(scan[0], (np.cumsum(v) - v) & M32), f"{what}: block_excl_scan<16>"
        assert int(misc[0]) == int(v.sum()) & M32, f"{what}: block_excl_scan<16>'s total"
        assert np.array_equal(scan[1], np.repeat(v.reshape(16, 64).sum(axis=1) & M32, 64)), f"{what}: wave_last of the inclusive scan"


def _float_lanes():
    rng = np.random.default_rng(34)
    f = np.float32
    fmax, tiny = np.finfo(f).max, np.float32(1e-45)                       # (the smallest denormal)
    spread = lambda a: rng.permutation(np.resize(np.asarray(a, f), 64))
    return {
        "negatives": (-rng.uniform(0.5, 4000.0, 64)).astype(f),
        "mixed signs": rng.uniform(-4000.0, 4000.0, 64).astype(f),
        "FLT_MAX both ways": spread([fmax, -fmax, 1.0, -1.0, 3.5]),
        "denormals": spread([tiny, -tiny, tiny * 3, -tiny * 7, np.float32(1e-39), np.float32(-1e-39)]),
        "denormals and normals": spread([tiny, np.float32(1.1754944e-38), -tiny, np.float32(-1.1754944e-38)]),
        "all equal": np.full(64, -12.625, f),
        "one differs, lane 0": np.concatenate([[f(-3.0)], np.full(63, 2.0, f)]),
        "one differs, lane 63": np.concatenate([np.full(63, 2.0, f), [f(-3.0)]]),
        "zeros of both signs": spread([0.0, -0.0]),
        "zeros among positives": spread([0.0, -0.0, 1.0, 2.0]),
        "zeros among negatives": spread([0.0, -0.0, -1.0, -2.0]),
    }


@pytest.mark.parametrize("name", list(_float_lanes()))
def test_wave_reductions_on_float_and_int(lp, name):
    lanes = _float_lanes()[name]
    words = lanes.view(np.uint32)
    _, red, _ = lp.selftest_wave_wide([], words, 1)
    fmin, fmax = red[0].view(np.float32), red[1].view(np.float32)
    if "zero" in name:                                                   # -0 and +0 are one number: compared as numbers
        assert np.array_equal(fmin, np.full(64, lanes.min())) and np.array_equal(fmax, np.full(64, lanes.max())), name
    else:
        assert np.array_equal(red[0], np.full(64, lanes.min().view(np.uint32))), f"{name}: wave_min float"
        assert np.array_equal(red[1], np.full(64, lanes.max().view(np.uint32))), f"{name}: wave_max float"
    ints = words.view(np.int32)                                          # the same words as int: both signs, the extremes
    assert np.array_equal(red[2].view(np.int32), np.full(64, ints.min())), f"{name}: wave_min int"
    assert np.array_equal(red[3].view(np.int32), np.full(64, ints.max())), f"{name}: wave_max int"


def test_wave_reductions_on_int_extremes(lp):
    rng = np.random.default_rng(35)
    for ints in (rng.integers(-(1 << 31), 1 << 31, 64).astype(np.int32), np.array([-(1 << 31), (1 << 31) - 1, 0, -1] * 16, np.int32),
                 np.full(64, -7, np.int32)):
        _, red, _ = lp.selftest_wave_wide([], ints.view(np.uint32), 1)
        assert np.array_equal(red[2].view(np.int32), np.full(64, ints.min())) and np.array_equal(red[3].view(np.int32), np.full(64, ints.max()))


@pytest.mark.parametrize("groups", [1, 2, 64, 257, 2090])
def test_last_block_names_one_workgroup_that_sees_every_word(lp, groups):
    """one launch per size, no repetition: exactly one workgroup is named, and it reads what all the others stored"""
    _, _, misc = lp.selftest_wave_wide([], LANES, groups)
    i = np.arange(4 * groups, dtype=np.uint64)
    want = int(((groups * 0x9E3779B1 + i * i + 1) & M32).sum()) & M32
    assert int(misc[1]) == 1, f"{int(misc[1])} workgroups were named the last"
    assert int(misc[2]) == want and int(misc[3]) == 0


def test_wave_wide_refuses_what_it_cannot_hold(lp):
    for values, groups in ((np.zeros(1025, np.uint32), 1), ([], 0), ([], 4097)):
        with pytest.raises(RolloutError):
            lp.selftest_wave_wide(values, LANES, groups)
