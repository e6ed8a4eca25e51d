"""Deterministic synthetic lidar sweeps for tests/test_lidar_sweep_cpu.py and tests/test_lidar_sweep_gpu.py: a floor (flat
or falling away from the sensor), the walls of a room, poles, a ramp, range noise, dropouts, duplicate returns, junk
records.  A beam is drawn inside its pixel, its range comes from casting the ray into the scene, and the point is taken
back to the tilted sensor's frame.

The generator draws a beam again until the restatement (lidar_sweep_ref.py) reports NO fragile decision for the sweep.
That is a condition, not a tolerance: every case handed out has zero fragile decisions, and tests/test_lidar_sweep_cpu.py
asserts so on the restatement alone.  It imports nothing from the library under test.
"""
import functools
import math

import numpy as np

import lidar_sweep_ref as R

f32, f64 = np.float32, np.float64
DEG = math.pi / 180.0


def directions(c, rows, cols, row_frac, col_frac):
    """Beam angles inside the pixels (rows, cols): vertical angle bottom + (row + row_frac) * resolution, so the row
    quotient is row + 0.1 deg / resolution + row_frac; the column angle -(col - H / 2 + col_frac) * 2 pi / H."""
    res = (c.top - c.bottom) / (c.V - 1)
    va = (c.bottom + (np.asarray(rows, f64) + row_frac) * res) * DEG
    ha = -(np.asarray(cols, f64) - c.H / 2 + col_frac) * (2 * math.pi / c.H)
    return va, ha


def points(va, ha, rng):
    """points of the pitch-removed frame: horizonAngle = atan2(x, y)"""
    rho = rng * np.cos(va)
    return np.stack([rho * np.sin(ha), rho * np.cos(ha), rng * np.sin(va)], axis=1)


def to_raw(pts, mount):
    """back into the tilted sensor's frame: the inverse of q.setRPY(0, mount, 0), float32 records"""
    cm, sm = math.cos(mount), math.sin(mount)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([cm * x - sm * z, y, sm * x + cm * z], axis=1).astype(f32)


class Scene:
    def __init__(self, height=0.6, slope_deg=0.0, walls=(9.0, 14.0), poles=(), ramp=None):
        self.h, self.slope, self.walls, self.poles, self.ramp = height, math.tan(slope_deg * DEG), walls, poles, ramp

    def cast(self, va, ha):
        """range of every beam; inf where nothing is hit"""
        tv, su, cu = np.tan(va), np.sin(ha), np.cos(ha)
        with np.errstate(all="ignore"):
            # floor: z = -h - slope * rho
            den = -tv - self.slope
            rho = np.where(den > 1e-9, self.h / den, np.inf)
            # walls of the room |x| <= wx, |y| <= wy
            wall = np.minimum(self.walls[0] / np.abs(su), self.walls[1] / np.abs(cu))
            rho = np.minimum(rho, wall)
            for (px, py, pr, top) in self.poles:                   # vertical cylinders from the floor up to z = top
                b = su * px + cu * py
                disc = b * b - (px * px + py * py - pr * pr)
                hit = b - np.sqrt(np.where(disc > 0, disc, np.nan))
                ok = (disc > 0) & (hit > 0) & (hit * tv <= top)
                rho = np.where(ok & (hit < rho), hit, rho)
            if self.ramp is not None:                              # z = -h + t * (x - x0) for x0 <= x <= x1, |y| <= w
                x0, x1, w, t = self.ramp
                r = (-self.h - t * x0) / (tv - t * su)
                ok = (r > 0) & (r * su >= x0) & (r * su <= x1) & (np.abs(r * cu) <= w)
                rho = np.where(ok & (r < rho), r, rho)
        return rho / np.cos(va)


def _draw(c, scene, rng, rows, cols):
    row_frac = np.where(np.asarray(rows) == 0, rng.uniform(-0.4, 0.5, len(rows)), rng.uniform(0.0, 0.5, len(rows)))
    col_frac = rng.uniform(-0.4, 0.4, len(rows))
    va, ha = directions(c, rows, cols, row_frac, col_frac)
    r = scene.cast(va, ha) * (1.0 + rng.normal(0.0, 0.002, len(rows)))
    return va, ha, r


def scene_sweep(c, scene, seed, dropout=0.03, duplicates=0.05):
    """One sweep of the scene: a beam per pixel in a shuffled order, dropouts as missing, NaN, infinite or all-zero
    records, second returns of some beams later in the input (the later one must win), beams out of range."""
    rng = np.random.default_rng(seed)
    rows, cols = (a.reshape(-1) for a in np.meshgrid(np.arange(c.V), np.arange(c.H), indexing="ij"))
    dup = rng.random(len(rows)) < duplicates
    rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
    order = rng.permutation(len(rows))
    rows, cols = rows[order], cols[order]
    va, ha, r = _draw(c, scene, rng, rows, cols)
    kind = rng.random(len(rows))
    for attempt in range(50):
        pts = points(va, ha, np.where(np.isfinite(r), r, 1.0))
        raw = to_raw(pts, c.mount)
        gone = kind < dropout
        raw[~np.isfinite(r) | (gone & (kind < dropout * 0.25))] = np.nan
        raw[gone & (kind >= dropout * 0.25) & (kind < dropout * 0.5)] = 0.0
        raw[gone & (kind >= dropout * 0.5) & (kind < dropout * 0.75), 0] = np.inf
        keep = ~(gone & (kind >= dropout * 0.75))
        ref = R.stage_one(raw[keep], c, segments=False)
        if ref["n_fragile"] == 0:
            return np.ascontiguousarray(raw[keep])
        bad = np.nonzero(keep)[0][ref["fragile_points"]]           # draw those beams again
        va[bad], ha[bad], r[bad] = _draw(c, scene, rng, rows[bad], cols[bad])
    raise AssertionError("no sweep without a fragile decision in 50 rounds")


def image_sweep(c, range_img, seed=0):
    """A sweep with one beam per pixel of a hand-made range image (0 = no return), in raster order."""
    rng = np.random.default_rng(seed)
    rows, cols = np.nonzero(np.asarray(range_img) > 0)
    r = np.asarray(range_img, f64)[rows, cols]
    for attempt in range(50):
        va, ha = directions(c, rows, cols, rng.uniform(0.1, 0.4, len(rows)), rng.uniform(-0.3, 0.3, len(rows)))
        raw = to_raw(points(va, ha, r), c.mount)
        if R.stage_one(raw, c, segments=False)["n_fragile"] == 0:
            return raw
    raise AssertionError("no sweep without a fragile decision in 50 rounds")


ROOM = dict(poles=((2.0, 3.0, 0.15, 0.4), (-3.0, 1.5, 0.2, 5.0), (4.0, -2.5, 0.1, 5.0), (-1.5, -4.0, 0.03, -0.2), (0.5, 6.0, 0.25, 5.0)),
            ramp=(1.5, 4.0, 1.0, 0.25))


def tiny_image():
    """4 x 8, the smallest image with a wrap, a ground pair and a segment: rows 0 and 1 see the floor (0.25 m below), rows
    2 and 3 an object across the wrap (columns 7, 0, 1), a second one (columns 3, 4) and a lone far return."""
    img = np.zeros((4, 8))
    img[0], img[1] = 0.25 / math.sin(12.0 * DEG), 0.25 / math.sin(3.0 * DEG)
    img[2:, [7, 0, 1]] = 5.0
    img[2:, [3, 4]] = 6.5
    img[3, 5] = 50.0
    return img


# name -> (Config, how to make the sweep).  The mount of 0.2 rad puts a flat floor above the node's 10 degree limit
# ((angle + mount) <= 10 deg), so those scenes have a floor that falls away from the sensor by 5 degrees.
def _specs():
    C = R.Config
    s = {}
    for gsi in (0, 1, 3):
        s[f"4x8-g{gsi}"] = (C(4, 8, -15.0, 15.0, gsi, valid_point_num=3, valid_line_num=2), ("image", tiny_image()))
    for gsi in (0, 7, 15):
        for mount in (0.0, 0.2):
            s[f"16x64-g{gsi}-m{mount}"] = (C(16, 64, -15.0, 15.0, gsi, max_range=30.0, mount=mount),
                                           ("scene", Scene(slope_deg=5.0 if mount else 0.0, walls=(7.0, 40.0), **ROOM), 100 + gsi))
    s["16x440-g7-m0.0"] = (C(16, 440, -15.0, 15.0, 7, max_range=30.0), ("scene", Scene(walls=(7.0, 40.0), **ROOM), 201))
    s["16x440-g15-m0.2"] = (C(16, 440, -15.0, 15.0, 15, max_range=30.0, mount=0.2), ("scene", Scene(slope_deg=5.0, walls=(7.0, 40.0), **ROOM), 202))
    s["16x1000-g7-m0.0"] = (C(16, 1000, -15.0, 15.0, 7, max_range=30.0), ("scene", Scene(walls=(7.0, 40.0), **ROOM), 301))
    s["16x1000-g7-m0.2"] = (C(16, 1000, -15.0, 15.0, 7, max_range=30.0, mount=0.2), ("scene", Scene(slope_deg=5.0, walls=(7.0, 40.0), **ROOM), 302))
    s["16x1000-g7-m0.2-b"] = (C(16, 1000, -15.0, 15.0, 7, max_range=30.0, mount=0.2), ("scene", Scene(slope_deg=5.0, walls=(6.0, 40.0), **ROOM), 303))
    s["64x2048-g7-m0.2"] = (C(64, 2048, -24.9, 2.0, 7, max_range=30.0, mount=0.2), ("scene", Scene(height=1.7, slope_deg=5.0, walls=(7.0, 40.0), **ROOM), 401))
    return s


SPECS = _specs()
NAMES = tuple(SPECS)
SMALL = tuple(n for n in NAMES if not n.startswith("64x"))


@functools.lru_cache(maxsize=None)
def case(name):
    """(Config, raw sweep [N,3] float32, the restatement's answer); computed once and shared: treat it as read-only"""
    c, how = SPECS[name]
    raw = image_sweep(c, how[1]) if how[0] == "image" else scene_sweep(c, how[1], how[2])
    raw.setflags(write=False)
    return c, raw, R.stage_one(raw, c)


# ---- hand-derivable known answers --------------------------------------------------------------------------------------
def _beams(c, triples, row_frac=0.25, col_frac=0.0):
    rows, cols, r = (np.asarray(v, f64) for v in zip(*triples))
    va, ha = directions(c, rows, cols, row_frac, col_frac)
    return to_raw(points(va, ha, r), c.mount)


def known_answers():
    """name -> (Config, raw sweep); what each must give is asserted in tests/test_lidar_sweep_cpu.py"""
    C = R.Config
    k = {}
    c = C(16, 64, -15.0, 15.0, 7)
    k["two_points_one_pixel"] = (c, _beams(c, [(9, 10, 5.0), (9, 10, 6.0)]))
    k["row_quotient_minus_half"] = (c, _beams(c, [(0, 20, 4.0)], row_frac=-0.55))          # quotient -0.55 + 0.05 = -0.5
    k["column_on_the_wrap"] = (c, _beams(c, [(9, 0, 5.0), (10, 64, 5.0)], col_frac=[0.1, -0.1]))   # angles pi - and -pi +
    k["segment_across_the_wrap"] = (c, _beams(c, [(r, col, 5.0) for r in (9, 10, 11) for col in (62, 63, 0, 1)]))
    c2 = C(16, 64, -15.0, 15.0, 7, valid_point_num=5, valid_line_num=2)
    k["row_of_29_beside_row_of_30"] = (c2, _beams(c2, [(9, col, 5.0) for col in range(0, 29)] + [(9, col, 5.0) for col in range(32, 62)]))
    pole = [(r, 30, 5.0) for r in range(8, 13)]
    for lines in (5, 4):                                   # 5 pixels in 5 rows: 4 lines, the seed's row is not counted
        cp = C(16, 64, -15.0, 15.0, 7, valid_point_num=5, valid_line_num=lines)
        k[f"pole_of_5_needs_{lines}_lines"] = (cp, _beams(cp, pole))
    floor = lambda row: 0.7 / math.sin((15.0 - 2.0 * (row + 0.25)) * DEG)          # a floor 0.7 m below, rows 2 degrees apart
    k["empty_lower_pixel"] = (c, _beams(c, [(1, 5, floor(1)), (1, 6, floor(1)), (0, 6, floor(0))]))
    c3 = C(16, 64, -15.0, 15.0, 0, valid_point_num=4, valid_line_num=2)
    k["labels_in_seed_order"] = (c3, _beams(c3, [(r, col, 5.0) for r in (2, 3) for col in (40, 41)] +      # valid, seed (2, 40)
                                      [(4, 10, 5.0), (4, 11, 5.0)] +                                         # invalid, seed (4, 10)
                                      [(r, col, 8.0) for r in (5, 6) for col in (3, 4, 5)]))                 # valid, seed (5, 3)
    return k
