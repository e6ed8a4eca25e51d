"""Cases for tests/test_sweep_association_cpu.py and tests/test_sweep_association_gpu.py, on top of lidar_sweep_cases and
lidar_features_cases: hand-made range images at the smallest shapes at which each rule of the association can go wrong,
and two of the existing scene sweeps (ground, picks of every kind, outliers).  It imports nothing from the library under
test.

Conditions, asserted in tests/test_sweep_association_cpu.py on the restatements alone.  Every case has no fragile
decision of the sweep (lidar_sweep_ref), no tie-sensitive feature list (lidar_features_ref) and min_margin >= MARGIN
(sweep_association_ref): every comparison an atan2f feeds -- findStartEndAngle's two corrections, the two wrap tests and
the flip of the first branch for the points up to i0, the two wrap tests of the second branch behind it -- holds at least
1e-5 rad from its threshold, lidar_sweep_ref's margin with its argument (a device atan2f within an ulp or two of the C
library's, 4.8e-7 rad at 2 pi).  A hand-made case is drawn again, seed by seed, until that holds and until the shape it
is made for has come out (`want`); a scene case is fixed by lidar_sweep_cases and only checked.  Voxel keys need no
margin: the coordinates are the inputs' own bits.

A wall of constant range has curvature ~0: no picks, so a ring of m points has m - 10 candidates when no sixth is
skipped (the sixths cover [start, end - 1]).  ori = -atan2f(y, x) falls as the column rises, by 2 pi / H per column.
"""
import functools

import numpy as np

import lidar_features_cases as FC
import lidar_features_ref as FR
import lidar_sweep_cases as Cs
import lidar_sweep_ref as R
import sweep_association_ref as AR

MARGIN = AR.MARGIN
PERIODS = (0.0, 0.1)


def _wall(V, H, rows, rng=5.0):
    """rows: per row an iterable of present columns"""
    img = np.zeros((V, H))
    for r, cols in enumerate(rows):
        img[r, list(cols)] = rng
    return img


def _small():
    """4 x 64: ring 0 has 8 points (fewer than 11: every sixth skipped), ring 1 has 21 (end - start = 11: exactly one sixth
    with sp >= ep), rings 2 and 3 are full"""
    return R.Config(4, 64, -15.0, 15.0, 0), _wall(4, 64, [range(10, 18), range(0, 21), range(64), range(64)])


def _counts():
    """8 x 512: rings of 73 / 74 / 75 and 265 / 266 / 267 points (63 / 64 / 65 and 255 / 256 / 257 candidates), an empty
    ring, and a ring of 30 points at 0.4 m that lies inside one voxel"""
    img = _wall(8, 512, [range(73), range(74), range(75), range(265), range(266), range(267), (), ()])
    img[7, 220:250] = 0.4
    return R.Config(8, 512, -15.0, 15.0, 0), img


def _wide():
    """2 x 4096, no ground: two full rings (4086 slots in the sixths, beyond the features' sort width) with 2 mm of range
    noise (neighbours stay connected; points flip between voxels from one index to the next) and small tents that are picked
    at the case's own edge threshold"""
    rng = np.random.default_rng(11)
    img = np.stack([5.0 + rng.uniform(-0.002, 0.002, 4096), 6.0 + rng.uniform(-0.002, 0.002, 4096)])
    for at in (300, 1111, 2500, 3900):
        img += FC.tent(4096, at, 0.004, 8)[None, :]
    return R.Config(2, 4096, -15.0, 15.0, 0), img


def _overflow():
    """4 x 64 with a maximum range of 100 km: 43 columns at 5 m but three in their middle at 40 km (12 points in 4 rows: a
    valid segment at valid_point_num 5, valid_line_num 3; at most one of a ring's three is picked as an edge, its neighbours
    are suppressed, not labelled), so every ring's voxel index overflows and VoxelGrid hands it through"""
    img = _wall(4, 64, [range(43)] * 4)
    img[:, 20:23] = 40000.0
    return R.Config(4, 64, -15.0, 15.0, 0, valid_point_num=5, valid_line_num=3, max_range=1.0e5), img


def _flip_last():
    """rings 0 .. 2 hold columns 0 .. 16, ring 3 column 17 as well; the sweep starts at (0, 1), a quarter turn (16 columns)
    before (3, 17): whether that point flips the flag depends on the two beams' places inside their pixels"""
    return R.Config(4, 64, -15.0, 15.0, 0), _wall(4, 64, [range(17), range(17), range(17), range(18)])


def _never():
    """a quarter of a turn, started at its first column: nothing is ever more than pi behind the start"""
    return R.Config(4, 64, -15.0, 15.0, 0), _wall(4, 64, [range(15)] * 4)


# name -> (image maker, edge, surf, (row, col) of the first raw record or None = raster order, junk records at both ends,
#          what the association must show for the draw to be accepted)
HAND = {
    "small": (_small, FC.EDGE, FC.SURF, None, False, lambda a, n: a["ring_skipped"][:2] == [6, 1] and 0 < a["i0"] < n),
    "small-junk-ends": (_small, FC.EDGE, FC.SURF, None, True, lambda a, n: True),
    "counts": (_counts, FC.EDGE, FC.SURF, None, False,
               lambda a, n: a["ring_candidates"][:6] == [63, 64, 65, 255, 256, 257] and a["ring_voxels"][7] == 1 and a["ring_candidates"][7] >= 19),
    "wide": (_wide, 0.005, FC.SURF, None, False, lambda a, n: min(a["ring_candidates"]) > 4000 and a["n_scattered"] > 0),
    "overflow": (_overflow, FC.EDGE, FC.SURF, None, False, lambda a, n: all(a["ring_overflow"]) and min(a["ring_candidates"]) > 20),
    # ring 0 is columns 10 .. 17, segment indices 0 .. 7; started at column 60, column 13 is the first one more than a
    # quarter turn (16 columns) on: the flag flips inside ring 0, the rest of it and every later ring take the second branch
    "flip-in-ring-0": (_small, FC.EDGE, FC.SURF, (2, 60), False, lambda a, n: 0 < a["i0"] < 7),
    "flip-at-the-last-point": (_flip_last, FC.EDGE, FC.SURF, (0, 1), False, lambda a, n: a["i0"] == n - 1),
    "never-flips": (_never, FC.EDGE, FC.SURF, (0, 0), False, lambda a, n: a["i0"] == n),
}
SCENES = ("16x64-g7-m0.0", "16x440-g7-m0.0")
EMPTY = "empty"
NAMES = tuple(HAND) + SCENES + (EMPTY,)


def _ordered(c, img, seed, first, junk):
    raw = Cs.image_sweep(c, img, seed)                     # one beam per pixel, raster order
    if first is not None:
        rows, cols = np.nonzero(np.asarray(img) > 0)
        at = int(np.nonzero((rows == first[0]) & (cols == first[1]))[0][0])
        order = [at] + [i for i in range(len(raw)) if i != at]
        raw = raw[order]
    if junk:
        nan, inf = np.float32(np.nan), np.float32(np.inf)
        raw = np.concatenate([[[nan, 1.0, 1.0], [0.5, inf, 0.5]], raw[: len(raw) // 2], [[1.0, 1.0, -inf]], raw[len(raw) // 2:],
                              [[nan, nan, nan]]]).astype(np.float32)
    return np.ascontiguousarray(raw, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(config, raw, ref = stage one, f = features, edge, surf): computed once and shared: read-only"""
    if name == EMPTY:
        c = R.Config(4, 64, -15.0, 15.0, 0)
        raw = np.zeros((0, 3), np.float32)
        ref = R.stage_one(raw, c)
        return dict(config=c, raw=raw, ref=ref, f=FR.features(ref, c, FC.EDGE, FC.SURF), edge=FC.EDGE, surf=FC.SURF)
    if name in SCENES:
        c, raw, ref, f = FC.case(name)
        return dict(config=c, raw=raw, ref=ref, f=f, edge=FC.EDGE, surf=FC.SURF)
    make, edge, surf, first, junk, want = HAND[name]
    c, img = make()
    for seed in range(40):
        raw = _ordered(c, img, seed, first, junk)
        ref = R.stage_one(raw, c)
        f = FR.features(ref, c, edge, surf)
        n = len(f["seg"]["range"])
        if ref["n_fragile"] or f["n_tie_sensitive"]:
            continue
        a = [AR.association(raw, c, ref, f, p) for p in PERIODS]
        if min(x["min_margin"] for x in a) >= MARGIN and want(a[0], n):
            raw.setflags(write=False)
            return dict(config=c, raw=raw, ref=ref, f=f, edge=edge, surf=surf)
    raise AssertionError(f"{name}: no draw in 40 seeds keeps the margins and shows its shape")


@functools.lru_cache(maxsize=None)
def expected(name, scan_period, node_T=False):
    k = case(name)
    return AR.association(k["raw"], k["config"], k["ref"], k["f"], scan_period, FR.node_T() if node_T else None)
