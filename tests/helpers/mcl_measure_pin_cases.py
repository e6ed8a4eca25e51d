"""Inputs of the particle-measure pin (tests/test_mcl_measure_pin_cpu.py, tests/test_mcl_measure_pin_gpu.py,
tests/golden/make_ref_mcl_golden.py) beyond mcl_measure_cases: small scenes aimed at one decision of mcl_3dl's measure()
each, and random rooms of at most 3000 map points.  Every input is chosen from the restatement's own reports
(mcl_measure_ref.measure: avg, roll, roll_diff, n_fragile, n_tied), never from the compiled reference; a scene is drawn
again with the next seed until the restatement reports no fragile decision and no tie, as mcl_measure_cases.case does.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import mcl_measure_ref as R
import mcl_measure_cases as Cs

F = np.float32
ROLL_EDGES = (2.6, 0.5, 3.1415926)
ROLL_MARGIN = 1e-6
N_ROOMS, ROOM_PARTICLES = 8, 250


def step(v, k):
    """the float32 k steps above (below for negative k) v"""
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return v


def _parts(static_map, ground, normals, flat, ls, states):
    return Cs._parts(static_map, ground, normals, flat, ls, states)


def _ring(rng, centre, k, radius, z=0.0):
    a = rng.uniform(0, 2 * math.pi, k)
    r = rng.uniform(radius[0], radius[1], k)
    return np.asarray(centre, np.float64) + np.stack([r * np.cos(a), r * np.sin(a), np.full(k, z)], axis=1)


def _observation(rng, n_flat=3, n_ls=5):
    """a few points around a particle standing 5 cm above a cluster's floor"""
    flat = np.concatenate([rng.uniform(-0.6, 0.6, (n_flat, 2)), rng.uniform(-0.1, 0.0, (n_flat, 1))], axis=1)
    ls = np.concatenate([rng.uniform(-0.6, 0.6, (n_ls, 2)), rng.uniform(-0.1, 0.0, (n_ls, 1)), rng.uniform(0.5, 3.0, (n_ls, 1))], axis=1)
    return flat, ls


def _clusters(rng, normals_of, radius=(0.15, 0.7), k=6):
    """one particle per entry of normals_of, each 5 cm above a floor patch of its own (k ground points, 8 m from the
    next patch) whose normals are normals_of[i] ([3] for all the same, or [k,3])"""
    ground, nrm, states = [], [], []
    for i, n in enumerate(normals_of):
        c = np.array([8.0 * (i % 6), 8.0 * (i // 6), 0.0])
        ground.append(_ring(rng, c, k, radius))
        nrm.append(np.broadcast_to(np.asarray(n, F), (k, 3)))
        q = Cs.quat_rpy(0.01 * (i % 5), -0.02 * (i % 3), 0.3 * i) * (0.5 + 0.1 * (i % 15))
        states.append(np.concatenate([c + np.array([0, 0, 0.05]), q]))
    ground = np.concatenate(ground)
    flat, ls = _observation(rng)
    return _parts(ground, ground, np.concatenate(nrm), flat, ls, states)


def counts_scene(seed, counts):
    """one particle per entry of counts with exactly that many ground points inside the 1 m search radius"""
    rng = np.random.default_rng(seed)
    ground, states = [], []
    for j, k in enumerate(counts):
        c = np.array([8.0 * j, 0.0, 0.0])
        ground.append(_ring(rng, c, k, (0.1, 0.85)))
        ground.append(_ring(rng, c, 9, (1.3, 1.8)))                    # outside the radius
        states.append(np.concatenate([c + np.array([0, 0, 0.05]), Cs.quat_rpy(0.02 * j, -0.01, 0.4 * j) * (0.7 + 0.2 * j)]))
    ground = np.concatenate(ground)
    nrm = np.concatenate([rng.normal(0, 0.08, (len(ground), 2)), np.ones((len(ground), 1))], axis=1)
    flat, ls = _observation(rng)
    return _parts(ground, ground, nrm, flat, ls, states)


def three_times_scene(seed):
    """the averaged normal a few float steps on either side of |n| >= 3 |nz|, on x and on y, both signs"""
    rng = np.random.default_rng(seed)
    nz = F(0.3 + 0.003 * rng.random())
    edge = F(3.0 * float(nz))
    normals = []
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            for k in (-3, -2, -1, 1, 2, 3):
                n = np.array([0.05, 0.05, nz], F)
                n[axis] = F(sign) * step(edge, k)
                normals.append(n)
    return _clusters(rng, normals)


def negative_z_scene(seed):
    """normals whose z is negative: all of a patch's, every other one's (without the fabs the average would fail the 3x
    test), and one of six"""
    rng = np.random.default_rng(seed)
    down = np.array([0.05, -0.03, -0.99], F)
    mixed = np.array([[0.3, 0.02, 0.95 * (-1) ** i] for i in range(6)], F)
    one = np.array([[0.02, 0.1, -0.98 if i == 2 else 0.98] for i in range(6)], F)
    return _clusters(rng, [down, mixed, one])


def up_normal_scene(seed):
    """exactly-up (and exactly-down) normals: right_vector is zero, the roll is NaN and roll_diff 0.55"""
    rng = np.random.default_rng(seed)
    return _clusters(rng, [np.array([0, 0, 1], F), np.array([0, 0, -1], F)])


def roll_targets():
    out = [2.9, 0.2, 1.5, -2.9, -0.2, -1.5, 0.0]
    for e in ROLL_EDGES:
        for side in (-3.0, 3.0):
            t = e + side * ROLL_MARGIN
            if t < math.pi - 1e-6:                                   # (3.1415926 is 5e-8 below pi: nothing fits above it)
                out += [t, -t]
    return out


def rolls_scene(seed):
    """one floor patch with one slightly tilted normal, and a particle per roll target: each state's roll is adjusted
    until the restatement's own roll sits within 5e-7 of the target (3e-6 from an edge of a band, or mid-band)"""
    rng = np.random.default_rng(seed)
    n = np.array([0.02, 0.01, 1.0]) / np.linalg.norm([0.02, 0.01, 1.0])
    ground = _ring(rng, np.zeros(3), 7, (0.2, 0.7))
    flat, ls = _observation(rng)
    pos = np.array([0, 0, 0.05])
    probe = _parts(ground, ground, np.tile(n, (7, 1)), flat, ls, [np.concatenate([pos, [0, 0, 0, 1]])])
    avg = Cs.answer(probe)["avg"][0]
    states = []
    for j, target in enumerate(roll_targets()):
        r, scale = target, 0.5 + 0.1 * (j % 15)
        for _ in range(12):
            rot = (Cs.quat_rpy(r, 0.01, 0.3) * scale).astype(F)
            rep = {}
            R.weight_healthy(avg, rot, F(0.01), rep)
            if abs(rep["roll"] - target) < 5e-7:
                break
            r += target - rep["roll"]
        assert abs(rep["roll"] - target) < 5e-7, (target, rep)
        states.append(np.concatenate([pos, rot]))
    return _parts(ground, ground, np.tile(n, (7, 1)), flat, ls, states)


CFG_WIDE = R.Config(radius_of_ground_search=1.5)
CFG_THR3 = R.Config(threshold_for_trusted_ground=3)
MDM = F(Cs.CFG.match_dist_min)
UP = F(3.4e-4)                     # 1 + UP * UP is the float above 1 (mcl_measure_cases.known_answers asserts it)
TILT = [0.02, 0.01, 0.9997]
# the flat loop's edges, as distances along x from a point at the origin: one float inside the match radius, on it, one
# float outside, below match_dist_flat, mid-range; then a point with no neighbour followed by one with a neighbour
FLAT_EDGES = [[np.nextafter(MDM, F(0)), 0, 0], [MDM, 0, 0], [np.nextafter(MDM, F(1)), 0, 0], [0.04, 0, 0], [0.2, 0, 0],
              [5, 5, 5], [0.1, 0, 0], [5, -5, 5]]
LS_WEIGHTS = [[0.1, 0, 0, 0.5], [0, 0.1, 0, 1.0], [0, 0, 0.1, 3.0], [-0.25, 0, 0, 1.7]]
ORIGIN_STATES = [[0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 2]]          # (the second normalises by an exact 0.5)


def nn_scene(seed, first):
    """a trusted floor (search radius 1.5 m) whose nearest point is `first`, the other six 1.2 m away"""
    rng = np.random.default_rng(seed)
    ground = np.concatenate([np.array([first], np.float64), _ring(rng, np.zeros(3), 6, (1.2, 1.4))])
    flat, ls = _observation(rng)
    return _parts(ground, ground, np.tile(TILT, (7, 1)), flat, ls, [ORIGIN_STATES[0]])


def far_floor_scene(seed):
    """trusted ground whose nearest point is 1.2 m away: (1 - d)(1 - roll_diff) < 0 becomes 0.01"""
    rng = np.random.default_rng(seed)
    ground = _ring(rng, np.zeros(3), 8, (1.2, 1.4))
    flat = ground[:3] + np.array([0.05, 0.0, 0.0])                     # (identity rotation at the origin: matched)
    return _parts(ground, ground, np.tile(TILT, (8, 1)), flat, _observation(rng)[1], [ORIGIN_STATES[0]])


def flat_edges_ground_scene(seed):
    """the flat loop on the ground tree: a ground point at the origin under the particle, six more 0.8 m away"""
    rng = np.random.default_rng(seed)
    ground = np.concatenate([np.zeros((1, 3)), _ring(rng, np.zeros(3), 6, (0.8, 0.95))])
    return _parts(ground, ground, np.tile(TILT, (7, 1)), FLAT_EDGES, LS_WEIGHTS, ORIGIN_STATES)


def flat_edges_map_scene(seed):
    """the flat loop on the map tree (no ground at all), the map's one point at the particle's position: pos_weight is
    exactly 1 and the likelihood is score_like itself"""
    return _parts([[0, 0, 0]], [], [], FLAT_EDGES, LS_WEIGHTS, ORIGIN_STATES)


def just_beyond_scene(seed):
    """untrusted, the nearest map point at 1.0003 m: 1 - sqrt(d2) < 0 becomes 0.01"""
    return _parts([[1.0003, 0, 0]], [], [], [[1.1, 0, 0]], [[1.0, 0.1, 0, 2.0]], [ORIGIN_STATES[0]])


def small_room(rng, half=3.0):
    """a 6 m room of at most 3000 map points: a jittered floor (a strip of it with normals tilted past and around the
    3x test, a tenth pointing down), four walls and two boxes"""
    g = np.arange(-half, half + 0.01, 0.25)
    gx, gy = np.meshgrid(g, g)
    ground = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)
    ground[:, :2] += rng.uniform(-0.08, 0.08, (len(ground), 2))
    ground[:, 2] = 0.02 * np.sin(ground[:, 0]) + rng.uniform(-0.01, 0.01, len(ground))
    nrm = np.concatenate([rng.normal(0, 0.05, (len(ground), 2)), np.ones((len(ground), 1))], axis=1)
    strip = ground[:, 0] > 0.5
    nrm[strip, 0] += rng.uniform(2.5, 6.0, int(strip.sum()))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[rng.random(len(ground)) < 0.1] *= -1.0
    walls = []
    t, z = np.meshgrid(np.arange(-half, half + 0.01, 0.2), np.arange(0.0, 2.01, 0.2))
    for a, s in ((0, -half), (0, half), (1, -half), (1, half)):
        w = np.zeros((t.size, 3))
        w[:, a], w[:, 1 - a], w[:, 2] = s, t.ravel(), z.ravel()
        walls.append(w + rng.uniform(-0.02, 0.02, w.shape))
    for c in ((1.2, 0.8), (-1.0, -1.5)):
        walls.append(rng.uniform(-0.3, 0.3, (200, 3)) + np.array([c[0], c[1], 0.4]))
    structure = np.concatenate(walls)
    static_map = np.concatenate([ground, structure])
    assert len(static_map) <= 3000
    return static_map, ground, nrm, structure


ROOM_CFGS = (Cs.CFG, R.Config(0.25, 0.1, 0.7, 4), R.Config(0.3, 0.05, 1.0, 12), R.Config(0.35, 0.02, 1.5, 30))


def random_room_scene(seed, n_states=ROOM_PARTICLES, n_flat=24, n_ls=40):
    rng = np.random.default_rng(seed)
    static_map, ground, nrm, structure = small_room(rng)
    true_pos, true_yaw = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 0.0]), rng.uniform(-math.pi, math.pi)
    Rt = Cs.rot_matrix(Cs.quat_rpy(0.0, 0.0, true_yaw))
    near = ground[np.linalg.norm(ground[:, :2] - true_pos[:2], axis=1) < 2.5]
    flat = (near[rng.choice(len(near), n_flat, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.02, (n_flat, 3))
    ls = (structure[rng.choice(len(structure), n_ls, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.03, (n_ls, 3))
    ls = np.concatenate([ls, rng.uniform(0.5, 3.0, (n_ls, 1))], axis=1)
    states = np.zeros((n_states, 7))
    for i in range(n_states):
        kind = rng.random()
        pos = true_pos + rng.normal(0, [0.2, 0.2, 0.05])
        rpy = np.array([rng.normal(0, 0.03), rng.normal(0, 0.03), true_yaw + rng.normal(0, 0.05)])
        if kind < 0.25:
            pos = np.array([rng.uniform(-2.8, 2.8), rng.uniform(-2.8, 2.8), rng.uniform(0, 0.1)])      # anywhere on the floor
        elif kind < 0.33:
            rpy[0] = rng.uniform(2.65, 3.1) * rng.choice([-1, 1])
        elif kind < 0.39:
            rpy[0] = rng.uniform(0.6, 2.4) * rng.choice([-1, 1])
        elif kind < 0.45:
            rpy[:2] = rng.uniform(-0.5, 0.5, 2)
        elif kind < 0.51:
            pos = np.array([rng.choice([-1, 1]) * rng.uniform(3.3, 3.9), rng.uniform(-2.5, 2.5), rng.uniform(0, 0.5)])
        elif kind < 0.55:
            pos = rng.uniform(-20, 20, 3) + np.array([30.0, 0, 0])
        elif kind < 0.63:
            pos[2] += rng.uniform(0.4, 1.6)
        states[i, :3] = pos
        states[i, 3:] = Cs.quat_rpy(*rpy) * rng.uniform(0.5, 2.0)
    return _parts(static_map, ground, nrm, flat, ls, states)


def weight_one_scene(seed, n_states=20, n_flat=50, n_ls=100):
    """no ground, so every particle is untrusted, and the map holds a point exactly at each particle's position:
    pos_weight = 1 - sqrt(0) = 1 and the likelihood is score_like, a float sum over up to 150 matches"""
    rng = np.random.default_rng(seed)
    static_map, ground, _, structure = small_room(rng)
    true_pos, Rt = np.array([0.3, -0.2, 0.0]), Cs.rot_matrix(Cs.quat_rpy(0.0, 0.0, 0.7))
    flat = (ground[rng.choice(len(ground), n_flat, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.02, (n_flat, 3))
    ls = (structure[rng.choice(len(structure), n_ls, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.03, (n_ls, 3))
    ls = np.concatenate([ls, rng.uniform(0.5, 3.0, (n_ls, 1))], axis=1)
    states = np.zeros((n_states, 7))
    states[:, :3] = true_pos + rng.normal(0, [0.1, 0.1, 0.03], (n_states, 3))
    states[:, 3:] = [Cs.quat_rpy(rng.normal(0, 0.02), rng.normal(0, 0.02), 0.7 + rng.normal(0, 0.04)) * rng.uniform(0.5, 2.0)
                     for _ in range(n_states)]
    states = states.astype(F)
    return _parts(np.concatenate([static_map.astype(F), states[:, :3]]), [], [], flat, ls, states)


# name -> (config, builder(seed)); the order is the order of the golden file
TARGETED = {
    "counts-5-6-7": (Cs.CFG, lambda s: counts_scene(s, (5, 6, 7))),
    "counts-2-3-4-threshold-3": (CFG_THR3, lambda s: counts_scene(s, (2, 3, 4))),
    "three-times": (Cs.CFG, three_times_scene),
    "negative-z": (Cs.CFG, negative_z_scene),
    "up-normal": (Cs.CFG, up_normal_scene),
    "rolls": (Cs.CFG, rolls_scene),
    "far-floor": (CFG_WIDE, far_floor_scene),
    "trusted-nn-at-one": (CFG_WIDE, lambda s: nn_scene(s, [1, 0, 0])),
    "trusted-nn-one-float-above-one": (CFG_WIDE, lambda s: nn_scene(s, [1, UP, 0])),
    "untrusted-nn-just-beyond-one": (Cs.CFG, just_beyond_scene),
    "flat-edges-on-ground": (Cs.CFG, flat_edges_ground_scene),
    "flat-edges-on-map-weight-one": (Cs.CFG, flat_edges_map_scene),
    "weight-one-room": (Cs.CFG, weight_one_scene),
}
ROOMS = {f"room-{i}": (ROOM_CFGS[i % len(ROOM_CFGS)], random_room_scene) for i in range(N_ROOMS)}
_ALL = dict(TARGETED, **ROOMS)
NAMES = tuple(_ALL)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (cfg, parts, restatement's answer, draws)"""
    cfg, build = _ALL[name]
    base = 50000 + 1000 * NAMES.index(name)
    for attempt in range(100):
        parts = build(base + attempt)
        ref = Cs.answer(parts, cfg)
        if int(ref["n_fragile"].sum()) == 0 and int(ref["n_tied"].sum()) == 0:
            for v in list(parts.values()) + [v for v in ref.values() if isinstance(v, np.ndarray)]:
                v.setflags(write=False)
            return cfg, parts, ref, attempt + 1
    raise AssertionError(f"case {name}: 100 draws and still a fragile decision or a tie")


def branch(ref):
    """the restatement's branch per particle in the compiled reference's code: 0 untrusted, 1 the 3x test took 0.2,
    2 the roll chain ran"""
    return np.where(ref["healthy"], np.where(np.isnan(ref["roll_diff"]), 1, 2), 0).astype(np.int32)
