"""Cases for tests/test_lidar_features_cpu.py and tests/test_lidar_features_gpu.py, on top of lidar_sweep_cases: the existing
sweeps by name, one 16 x 2000 hand-made range image (the shipped mcl_c16_config.yaml shape) and small hand-made images
whose feature lists are derived below by reading the reference (featureAssociation.cpp:318-491), not by running anything.
It imports nothing from the library under test.

Conditions, asserted in tests/test_lidar_features_cpu.py on the restatements alone: every case used for parity has
n_tie_sensitive == 0 and n_fragile == 0; over the set both breaks (21st edge, 4th flat) are taken, and there are
occlusion marks, a pick at slot ep and the slot-4 pick of index 0.

How the hand cases are built.  A tent of slope a and half width w >= 6 in an otherwise constant range profile gives, by
calculateSmoothness's sum (ten neighbours minus ten times the centre), d = -30 a at its apex, -20 a one index beside it,
-11 a (w = 6) or -12 a two beside it, and +15 a at each foot (+-w): curvatures 900 a^2, 400 a^2, <= 144 a^2, 225 a^2.  With
the edge threshold at 1.0 a strong tent (a = 0.06) has three candidates, apex 3.24 and its two neighbours 1.44, a weak one
(|a| = 0.04) only its apex, 1.44; feet stay below (0.81, 0.36).  All slopes stay under the occlusion limits (0.3 m between
neighbours; 2 % of the range on both sides).  The wall cases repeat one profile on rows 8 .. 15 of a 16 x 128 image with
no ground (ground_scan_index 0), so every ring holds the same points and gives the same picks; rows 0 .. 7 are empty
rings (start > end).  The floor cases put one range pattern on the ground points of rows 0 .. 5.
"""
import functools
import math

import numpy as np

import lidar_features_ref as FR
import lidar_sweep_cases as Cs
import lidar_sweep_ref as R

EDGE, SURF = 0.1, 0.1                       # mcl_c16_config.yaml: featureAssociation.edge_threshold / surf_threshold
SWEEP_NAMES = ("4x8-g1", "16x64-g0-m0.0", "16x64-g7-m0.0", "16x64-g15-m0.0", "16x64-g7-m0.2", "16x440-g7-m0.0", "16x1000-g7-m0.0",
               "16x1000-g7-m0.2-b", "64x2048-g7-m0.2")
BIG = "16x2000-floor-wall"


def big_image(seed=5):
    """16 x 2000: rows 0-5 a floor 0.6 m below with +-2 mm height noise, rows 6-15 a wall at 8 m with +-6 cm range noise,
    a 40-column hole in rows 10-15 (column jumps above 10)."""
    rng = np.random.default_rng(seed)
    img = np.zeros((16, 2000))
    for r in range(6):
        img[r] = (0.6 + rng.uniform(-0.002, 0.002, 2000)) / math.sin((15.0 - 2.0 * (r + 0.25)) * Cs.DEG)
    img[6:] = 8.0 + rng.uniform(-0.06, 0.06, (10, 2000))
    img[10:, 700:740] = 0.0
    return img


def big_config():
    return R.Config(16, 2000, -15.0, 15.0, 7, valid_point_num=5, valid_line_num=2, max_range=50.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """(Config, raw sweep, stage-one restatement, feature restatement at EDGE / SURF); computed once: read-only"""
    if name == BIG:
        c = big_config()
        raw = Cs.image_sweep(c, big_image())
        raw.setflags(write=False)
        ref = R.stage_one(raw, c)
    else:
        c, raw, ref = Cs.case(name)
    return c, raw, ref, FR.features(ref, c, EDGE, SURF)


PARITY = SWEEP_NAMES + (BIG,)

# ---- hand-derived known answers ------------------------------------------------------------------------------------------
H = 128
WALL_ROWS = range(8, 16)
HAND_EDGE, HAND_SURF = 1.0, 0.1


def tent(n, at, a, w):
    m = np.abs(np.arange(n) - at)
    return a * np.maximum(0, w - m)


def wall_case(profile, missing=(), short_first_row=None):
    """rows 8 .. 15 carry 5 m + profile over the PRESENT columns in order (the profile is indexed by position in the ring,
    which is what calculateSmoothness sees); `missing` columns give no return; short_first_row: row 8 keeps only these columns"""
    c = R.Config(16, H, -15.0, 15.0, 0)
    present = [j for j in range(H) if j not in set(missing)]
    img = np.zeros((16, H))
    for r in WALL_ROWS:
        img[r, present] = 5.0 + np.asarray(profile)[: len(present)]
    if short_first_row is not None:
        keep = np.zeros(H, bool)
        keep[list(short_first_row)] = True
        img[8, ~keep] = 0.0
    return c, img


def floor_case(raised_head=0.0):
    """rows 0 .. 5 a floor; the 34 ground points a ring keeps (columns 0-5, 10, 15 .. 120, 123-127) carry base + pattern:
    +-u alternating (d = -+12 u with u = 0.04, curvature 0.23, between 0.13 and 0.36 beside a lowered point: never flat,
    and with the edge threshold at 0.1 above it, so only the ground flag keeps them from being edges), except the even positions 6, 14 and 22, lowered by 1.2 u + d / 10 so that their
    own d is 0.10, 0.05 and 0.15 (curvatures 0.01, 0.0025, 0.0225) while their neighbours move by 0.05 only."""
    c = R.Config(16, H, -15.0, 15.0, 7)
    cols = list(range(6)) + list(range(10, 121, 5)) + list(range(123, 128))
    u = 0.04
    pattern = np.where(np.arange(34) % 2 == 0, u, -u)
    for pos, d in ((6, 0.10), (14, 0.05), (22, 0.15)):
        pattern[pos] = u - 1.2 * u - d / 10.0
    pattern[:6] += raised_head
    img = np.zeros((16, H))
    for r in range(6):
        base = 0.6 / math.sin((15.0 - 2.0 * (r + 0.25)) * Cs.DEG)
        img[r] = base
        img[r, cols] = base + pattern
    return c, img, cols


def _wall_expect(cnt, rings, picks):
    """segment indices of ring positions `picks` in each of `rings` (ring k of the wall holds indices k cnt .. k cnt + cnt - 1)"""
    return [k * cnt + p for k in rings for p in picks]


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> dict(config, image or None, edge, surf, expect = (sharp, less_sharp, flat) as segment indices, n_seg)"""
    k = {}

    def add(name, c, img, expect, n_seg, edge=HAND_EDGE, surf=HAND_SURF):
        k[name] = dict(config=c, image=img, edge=edge, surf=surf, expect=tuple(list(e) for e in expect), n_seg=n_seg)

    # a full ring of 128: s = first + 4, e = first + 122; sp = 4, 23, 43, 63, 82, 102 and ep = 22, 42, 62, 81, 101, 121 (positions)
    strong, weak = 0.06, -0.04
    # A strong at 20 (sixth 0, not its ep), B weak and inverted at 25 (sixth 1): d(20) = -1.8 - 0.4, d(25) = +1.2 + 0: A is
    # picked in sixth 0 and suppresses 15 .. 25, B with it; nothing else of sixth 1 passes 1.0 (26: 0.8^2)
    c, img = wall_case(tent(H, 20, strong, 16) + tent(H, 25, weak, 6))
    add("next_sixth_best_removed", c, img, (_wall_expect(H, range(8), [20]), _wall_expect(H, range(8), [20]), []), 8 * H)
    # the same with B at 26: out of A's reach, picked in sixth 1
    c, img = wall_case(tent(H, 20, strong, 16) + tent(H, 26, weak, 6))
    add("next_sixth_best_kept", c, img, (_wall_expect(H, range(8), [20, 26]), _wall_expect(H, range(8), [20, 26]), []), 8 * H)
    # columns 31 .. 40 missing: positions 30 | 31 are columns 30 | 41, a jump of 11.  The apex at 30 is picked, its forward
    # suppression stops at once, position 31 (1.44) is the next candidate; its backward suppression stops at once too
    c, img = wall_case(tent(H, 30, strong, 16), missing=range(31, 41))
    add("column_jump_11_stops_suppression", c, img, (_wall_expect(118, range(8), [30, 31]), _wall_expect(118, range(8), [30, 31]), []), 8 * 118)
    # columns 31 .. 39 missing: a jump of 10 does not stop it
    c, img = wall_case(tent(H, 30, strong, 16), missing=range(31, 40))
    add("column_jump_10_does_not", c, img, (_wall_expect(119, range(8), [30]), _wall_expect(119, range(8), [30]), []), 8 * 119)
    # apex at 41, its neighbour 42 is slot ep of sixth 1: the walk starts at k = ep, whose slot is unsorted, so 42 (1.44) is
    # taken before the larger 41 (3.24) and suppresses it
    c, img = wall_case(tent(H, 41, strong, 16))
    add("candidate_at_slot_ep", c, img, (_wall_expect(H, range(8), [42]), _wall_expect(H, range(8), [42]), []), 8 * H)
    # row 8 keeps 8 points (fewer than 12: s = 4, e = 2, every sixth skipped); the rings after it start at index 8
    c, img = wall_case(tent(H, 60, strong, 16), short_first_row=range(20, 28))
    exp = [8 + (r - 1) * H + 60 for r in range(1, 8)]
    add("short_ring_beside_full_ones", c, img, (exp, exp, []), 8 + 7 * H)
    # 3 x 3 points: a valid segment of 9, fewer than 11 points: no loop of calculateSmoothness runs, no sixth is walked
    c = R.Config(16, H, -15.0, 15.0, 0)
    img = np.zeros((16, H))
    img[8:11, 50:53] = 5.0
    add("fewer_than_11_points", c, img, ([], [], []), 9)
    add("empty_sweep", c, None, ([], [], []), 0)
    # floor: ring k holds indices 34 k .. 34 k + 33; s = first + 4, e = first + 28: sp = 4, 8, .. 24, ep = 7, 11, .. 27.
    # ring 0, sixth 0: slots 4 5 6 sorted are {0, ind 0}, position 6 (0.01), position 5 (0.23): index 0 is flat (curvature
    # 0 of a fresh node, ground, not marked) and suppresses 1 .. 5; 6 is next and suppresses 1 .. 11; sixth 2 picks 14
    # (suppresses 9 .. 19), sixth 4 picks 22.  The other rings have no slot 4.  Edge threshold 0.1: the rough points'
    # 0.23 is above it, they are ground, no edge.
    c, img, cols = floor_case()
    flat = [0, 6, 14, 22] + [34 * r + p for r in range(1, 6) for p in (6, 14, 22)]
    add("slot_4_picks_index_0", c, img, ([], [], flat), 6 * 34, edge=0.1)
    # positions 0 .. 5 a metre further: range[5] - range[6] > 0.3 with a column step of 5 marks 0 .. 5 (markOccludedPoints,
    # i = 5), so index 0 is not picked; positions 6 .. 10 have five .. one raised neighbours (|d| >= 0.52) and are no
    # candidates either
    c, img, cols = floor_case(raised_head=1.0)
    flat = [34 * r + p for r in range(6) for p in (14, 22)]
    add("slot_4_not_when_marked", c, img, ([], [], flat), 6 * 34, edge=0.1)
    return k


@functools.lru_cache(maxsize=None)
def hand_sweep(name):
    """(Config, raw sweep, stage-one restatement) of a hand case"""
    h = hand_cases()[name]
    c = h["config"]
    raw = np.zeros((0, 3), np.float32) if h["image"] is None else Cs.image_sweep(c, h["image"])
    raw.setflags(write=False)
    return c, raw, R.stage_one(raw, c)
