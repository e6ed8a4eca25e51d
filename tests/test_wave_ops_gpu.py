"""The wave and workgroup primitives of csrc/wave_ops.hip.h, through their one entry point (selftest_wave_ops: a single
workgroup of 256 lanes, the lanes at or past n taking part with value 0 and a clear flag), against NumPy bit for bit.
Sums wrap as their integer type does.  The four waves race for the append's counter, so of the append only what is
guaranteed is asserted: inside a wave the keeping lanes hold consecutive ascending indices, the waves' ranges are
disjoint and tile [base, base + count), the final counter is base + count; a lane that does not keep is not looked at.

Sizes: one lane, a wave less one, a wave, a wave and one, the workgroup less one, the workgroup, and nothing at all."""
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
