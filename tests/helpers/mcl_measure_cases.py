"""Named inputs for the particle-measure tests: a scene (map, ground, normals), an observation (flat, less sharp) and
a batch of states, with the restatement's answer (mcl_measure_ref.measure).  A case is drawn again, with the next seed,
until the restatement reports no fragile decision of the double chain and no tie between ground neighbours with
different normals; after 100 draws it fails loudly.  Answers are computed once per process and must not be modified.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import mcl_measure_ref as R

F = np.float32
SHIFT = np.array([3000.0, -7000.0, 40.0], F)


def quat_rpy(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(yaw / 2), math.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def rot_matrix(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def room(rng):
    """a 12 m room: a jittered floor with near-vertical normals (some pointing down), four walls and a few boxes"""
    g = np.arange(-6.0, 6.01, 0.25)
    gx, gy = np.meshgrid(g, g)
    ground = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)
    ground[:, :2] += rng.uniform(-0.08, 0.08, (len(ground), 2))
    ground[:, 2] = 0.02 * np.sin(ground[:, 0]) + rng.uniform(-0.01, 0.01, len(ground))
    nrm = np.concatenate([rng.normal(0, 0.05, (len(ground), 2)), np.ones((len(ground), 1))], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[rng.random(len(ground)) < 0.1] *= -1.0
    walls = []
    t, z = np.meshgrid(np.arange(-6.0, 6.01, 0.15), np.arange(0.0, 2.01, 0.15))
    for a, s in ((0, -6.0), (0, 6.0), (1, -6.0), (1, 6.0)):
        w = np.zeros((t.size, 3))
        w[:, a], w[:, 1 - a], w[:, 2] = s, t.ravel(), z.ravel()
        walls.append(w + rng.uniform(-0.02, 0.02, w.shape))
    for c in ((2.5, 1.0), (-1.5, 3.0), (1.0, -3.5)):
        b = rng.uniform(-0.4, 0.4, (400, 3)) + np.array([c[0], c[1], 0.5])
        walls.append(b)
    structure = np.concatenate(walls)
    static_map = np.concatenate([ground, structure])
    assert len(static_map) <= 20000
    return static_map.astype(F), ground.astype(F), nrm.astype(F), structure


def room_case(seed, n_states, n_flat, n_ls, shift=None):
    rng = np.random.default_rng(seed)
    static_map, ground, nrm, structure = room(rng)
    true_pos, true_q = np.array([0.5, -0.3, 0.0]), quat_rpy(0.0, 0.0, 0.4)
    Rt = rot_matrix(true_q)
    near = ground[np.linalg.norm(ground[:, :2] - true_pos[:2], axis=1) < 4.0].astype(np.float64)
    flat = (near[rng.choice(len(near), n_flat, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.02, (n_flat, 3))
    ls = (structure[rng.choice(len(structure), n_ls, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.03, (n_ls, 3))
    ls = np.concatenate([ls, rng.uniform(0.5, 3.0, (n_ls, 1))], axis=1)
    states = np.zeros((n_states, 7))
    for i in range(n_states):
        kind = rng.random() if n_states > 1 else 0.0
        pos = true_pos + rng.normal(0, [0.15, 0.15, 0.05])
        rpy = np.array([rng.normal(0, 0.03), rng.normal(0, 0.03), 0.4 + rng.normal(0, 0.05)])
        if 0.70 <= kind < 0.78:
            rpy[0] = rng.uniform(2.65, 3.1) * rng.choice([-1, 1])          # the first roll band
        elif 0.78 <= kind < 0.84:
            rpy[0] = rng.uniform(0.6, 2.4) * rng.choice([-1, 1])           # neither band
        elif 0.84 <= kind < 0.90:
            pos = np.array([rng.choice([-1, 1]) * rng.uniform(6.3, 6.9), rng.uniform(-5, 5), rng.uniform(0, 0.5)])   # off the floor, by a wall
        elif 0.90 <= kind < 0.94:
            pos = rng.uniform(-40, 40, 3) + np.array([60.0, 0, 0])        # nowhere
        elif 0.94 <= kind:
            pos[2] += rng.uniform(0.5, 1.3)                                # above the floor: few or no ground neighbours
        states[i, :3] = pos
        states[i, 3:] = quat_rpy(*rpy) * rng.uniform(0.5, 2.0)             # raw, not normalised
    parts = dict(map=static_map, ground=ground, normals=nrm, flat=flat.astype(F), ls=ls.astype(F), states=states.astype(F))
    if shift is not None:
        for k in ("map", "ground"):
            parts[k] = (parts[k] + shift).astype(F)
        parts["states"][:, :3] = (parts["states"][:, :3] + shift).astype(F)
    return parts


GROUND_COUNTS = (0, 5, 6, 64, 65, 300)


def ground_counts_case(seed):
    """one particle per entry of GROUND_COUNTS with exactly that many ground points inside the search radius"""
    rng = np.random.default_rng(seed)
    ground, states, extra = [], [], []
    for j, k in enumerate(GROUND_COUNTS):
        c = np.array([25.0 * j, 3.0 * j, 0.0])
        d = rng.normal(size=(k, 3))
        d[:, 2] *= 0.1
        d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.05, 0.9, (k, 1))
        ground.append(c + d)
        ground.append(c + np.array([1.6, 0, 0]) + rng.uniform(-0.3, 0.3, (20, 3)))      # outside the radius
        extra.append(c + np.array([0.0, 0.5, 0.2]) + rng.uniform(-0.1, 0.1, (30, 3)))
        states.append(np.concatenate([c + np.array([0, 0, 0.05]), quat_rpy(0.02 * j, -0.01 * j, 0.3 * j) * (1.0 + 0.1 * j)]))
    ground = np.concatenate(ground)
    nrm = np.concatenate([rng.normal(0, 0.08, (len(ground), 2)), np.ones((len(ground), 1))], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    static_map = np.concatenate([ground, np.concatenate(extra)])
    flat = rng.uniform(-0.8, 0.8, (3, 3)) * np.array([1, 1, 0.05])
    ls = np.concatenate([rng.uniform(-0.3, 0.3, (130, 3)) + np.array([0.0, 0.5, 0.15]), rng.uniform(0.5, 3.0, (130, 1))], axis=1)
    return dict(map=static_map.astype(F), ground=ground.astype(F), normals=nrm.astype(F), flat=flat.astype(F), ls=ls.astype(F),
                states=np.array(states).astype(F))


def small_map_case(seed, n_map):
    """a map of one point, or none: no ground either, so every particle takes the unhealthy branch"""
    rng = np.random.default_rng(seed)
    static_map = np.array([[0.3, 0.1, 0.0]], F)[:n_map]
    states = np.zeros((5, 7), F)
    states[:, :3] = np.array([[0, 0, 0], [0.2, 0.1, 0.05], [0.9, 0.2, 0], [1.4, 0, 0], [5, 5, 5]], F)
    states[:, 3:] = np.array([quat_rpy(0, 0, a) * s for a, s in ((0, 1), (0.3, 2), (1.0, 0.5), (2.0, 1), (3.0, 3))], F)
    ls = np.concatenate([rng.uniform(-0.25, 0.25, (4, 3)), rng.uniform(0.5, 3.0, (4, 1))], axis=1).astype(F)
    return dict(map=static_map, ground=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), flat=rng.uniform(-0.2, 0.2, (2, 3)).astype(F), ls=ls,
                states=states)


NEEDLE_DIRS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


PAD = F(1e-3)                      # the device's widening of its search boxes (kMclPad)
NEEDLE_LO, NEEDLE_HI = np.array([-5, -5, -2], F), np.array([45, 35, 13], F)      # two filler points fix the map's box


def device_grid(map_xyz, match_dist_min=0.3):
    """The uniform grid the device builds over a cloud (mcl_upload / grid_shape, float32 like there): origin at the
    cloud's minimum, cubic cells 2.02 * (match_dist_min + pad) wide -> (origin [3], cell, 1 / cell)"""
    cell = F(2.02) * F(F(match_dist_min) + PAD)
    lo, hi = map_xyz.min(axis=0).astype(F), map_xyz.max(axis=0).astype(F)
    n = np.ceil((hi - lo) / cell).astype(np.int64) + 1
    assert n.prod() <= 1 << 21                                      # (beyond that the device coarsens the cells)
    return lo, cell, F(1.0) / cell


def device_cells(grid, p, d=F(0)):
    """grid_cx / grid_cy / grid_cz of ((p - origin) + d), unclamped"""
    lo, cell, inv = grid
    return np.floor(((np.asarray(p, F) - lo) + F(d)) * inv).astype(np.int64)


def needle_case(seed):
    """26 identity-rotation particles and one less-sharp point.  Each particle's single match is one map point, placed
    by CELL of the device's grid: along every axis the query sits 0.08 m on one side of a cell boundary and the needle
    0.08 m on the other (direction +1 / -1), or both sit mid-cell (direction 0).  Over the 26 directions the needle
    takes every cell of the query's 2 x 2 x 2 box of candidates, the far corner (all three axes crossed, 0.277 m away)
    from both sides.  needle_cells() gives the indices; tests/test_mcl_measure_cpu.py asserts them."""
    rng = np.random.default_rng(seed)
    o = np.array([0.11, 0.23, 0.31])
    cell = float(F(2.02) * F(F(CFG.match_dist_min) + PAD))
    states = np.zeros((len(NEEDLE_DIRS), 7))
    needles = []
    for i, d in enumerate(NEEDLE_DIRS):
        k = np.array([4 + 4 * (i % 6), 4 + 4 * (i // 6), 3 + 3 * (i % 5)])
        bound = NEEDLE_LO.astype(np.float64) + k * cell
        u = np.array(d, np.float64)
        q = bound - 0.08 * u + 0.3 * (u == 0)
        needles.append(bound + 0.08 * u + 0.3 * (u == 0))
        states[i, :3], states[i, 6] = q - o, 1.0
    perm = rng.permutation(len(needles))                              # (the order in the map is not the particles')
    static_map = np.concatenate([np.array(needles)[perm], [NEEDLE_LO, NEEDLE_HI]]).astype(F)
    return dict(map=static_map, ground=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), flat=np.zeros((0, 3), F),
                ls=np.array([[*o, 2.0]], F), states=states.astype(F), needle_of=np.argsort(perm))


def needle_cells(parts):
    """per particle of the needle case, as the device computes them: the query's cell, the first and last cell of its
    candidate box, and its needle's cell -> four [N,3] integer arrays"""
    grid = device_grid(parts["map"])
    r = F(F(CFG.match_dist_min) + PAD)
    q = (parts["ls"][0, :3][None, :] + parts["states"][:, :3]).astype(F)       # identity rotation: o + pos_, one float add
    return (device_cells(grid, q), device_cells(grid, q, -r), device_cells(grid, q, r),
            device_cells(grid, parts["map"][parts["needle_of"]]))


CFG = R.Config()
_BUILDERS = {
    "n1-o0x1": lambda s: room_case(s, 1, 0, 1),
    "n64-o1x0": lambda s: room_case(s, 64, 1, 0),
    "n65-o1x1": lambda s: room_case(s, 65, 1, 1),
    "n300-o64x65": lambda s: room_case(s, 300, 64, 65),
    "n64-o3x130": lambda s: room_case(s, 64, 3, 130),
    "n65-o40x200": lambda s: room_case(s, 65, 40, 200),
    "n5-o600x1400": lambda s: room_case(s, 5, 600, 1400),           # the largest observation the library takes (2000 points)
    "n65-o40x200-shifted": lambda s: room_case(s, 65, 40, 200, shift=SHIFT),
    "ground-counts": ground_counts_case,
    "map-of-one": lambda s: small_map_case(s, 1),
    "map-empty": lambda s: small_map_case(s, 0),
    "needles": needle_case,
}
NAMES = tuple(_BUILDERS)
SMOKE = "n1-o0x1"          # the smallest: what __graft_entry__.smoke() runs


def answer(parts, cfg=CFG):
    return R.measure(cfg, parts["map"], parts["ground"], parts["normals"], parts["flat"], parts["ls"], parts["states"])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (parts, ref, draws)"""
    base = 1000 * (NAMES.index(name.replace("-shifted", "")) + 1)         # the shifted scene is its namesake's, moved
    for attempt in range(100):
        parts = _BUILDERS[name](base + attempt)
        ref = answer(parts)
        if int(ref["n_fragile"].sum()) == 0 and int(ref["n_tied"].sum()) == 0:
            for v in list(parts.values()) + [v for v in ref.values() if isinstance(v, np.ndarray)]:
                v.setflags(write=False)
            return parts, ref, attempt + 1
    raise AssertionError(f"case {name}: 100 draws and still a fragile decision or a tie")


# ---- hand-derived known answers: (name, cfg, parts, expected per-particle values) --------------------------------------

def _parts(static_map, ground, normals, flat, ls, states):
    a = lambda v, c: np.asarray(v, F).reshape(-1, c)
    return dict(map=a(static_map, 3), ground=a(ground, 3), normals=a(normals, 3), flat=a(flat, 3), ls=a(ls, 4), states=a(states, 7))


IDENT = [0, 0, 0, 0, 0, 0, 1]


def _lattice(h, normal, n=5, step=0.3):
    """a (2n+1)^2 lattice floor at z = -h below the origin, every normal the same"""
    g = np.arange(-n, n + 1) * step
    gx, gy = np.meshgrid(g, g)
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -h)], axis=1).astype(F)
    return ground, np.tile(np.asarray(normal, F), (len(ground), 1))


def known_answers():
    out = []
    mdm, mdf = F(0.3), F(0.05)
    below, above = np.nextafter(mdm, F(0)), np.nextafter(mdm, F(1))
    # one identity particle, one map point at distance d along x, one less-sharp point at the origin
    for d, matched in ((F(0.0), 1), (F(0.04), 1), (F(0.2), 1), (below, 1), (mdm, 0), (above, 0)):
        d2 = F(d * d)
        dist = F(mdm - max(np.sqrt(d2), mdf))
        intensity = F(1.7)
        score = F(F(dist * dist) / intensity) if matched else F(0)
        w = F(1.0 - float(np.sqrt(d2)))                                 # no ground: the map's nearest point decides the weight
        out.append((f"one-point-d{float(d):.9g}", CFG, _parts([[d, 0, 0]], [], [], [], [[0, 0, 0, intensity]], [IDENT]),
                    dict(score=[score], n_match=[matched], pos_weight=[w], healthy=[False], likelihood=[F(score * w)], quality=[F(matched)])))
    # a floor whose normals are exactly up: right_vector is zero, roll is NaN, roll_diff = 0.55
    ground, nrm = _lattice(0.2, (0, 0, 1))
    w = F((1.0 - float(np.sqrt(F(F(0.2) * F(0.2))))) * (1 - 0.55))
    out.append(("flat-floor-nan-roll", CFG, _parts(ground, ground, nrm, [[0, 0, -0.2]], [], [IDENT]),
                dict(pos_weight=[w], healthy=[True], n_ground=[37], n_match=[1], score=[F(F(mdm - mdf) * F(mdm - mdf))])))
    # five against six ground neighbours at threshold 6
    ring = [[0.5 * math.cos(a), 0.5 * math.sin(a), 0.0] for a in np.arange(6) * 1.0471975512]
    far = [[50 + 0.5 * math.cos(a), 0.5 * math.sin(a), 0.0] for a in np.arange(5) * 1.0471975512]
    gr = np.array(ring + far, F)
    out.append(("five-against-six", CFG, _parts(gr, gr, np.tile(np.array([0.1, 0, 0.99498744], F), (11, 1)), [[0.5, 0, 0]], [],
                                                [IDENT, [50, 0, 0, 0, 0, 0, 1]]),
                dict(healthy=[True, False], n_ground=[6, 5])))
    # the pose's nearest map point at d2 = 1 exactly, one float above, clearly beyond
    up = F(3.4e-4)
    assert F(F(1) + F(up * up)) == np.nextafter(F(1), F(2))
    for name, pt, w in (("nn-at-one", [1, 0, 0], F(0.0)), ("nn-one-ulp-above", [1, up, 0], F(0.0)), ("nn-beyond", [1.5, 0, 0], F(0.01))):
        out.append((name, CFG, _parts([pt], [], [], [], [[0, 0, 0, 1]], [IDENT]),
                    dict(pos_weight=[w], healthy=[False], n_match=[0], likelihood=[F(0.0)], score=[F(0.0)])))
    # a normal tilted past the 3x test
    t = np.array([0.9, 0.0, 0.2]) / math.hypot(0.9, 0.2)
    ground, nrm = _lattice(0.1, t)
    out.append(("tilted-normal", CFG, _parts(ground, ground, nrm, [[0, 0, -0.1]], [], [IDENT]), dict(pos_weight=[F(0.2)], healthy=[True])))
    return out
