"""Seeded inputs for the observation tests (mcl_observation_ref.prepare): less-sharp lists that select each branch of
cbLeGoFeatureCloud and lidar-like flat lists.  The shapes are laid out in base_link and carried into the sensor frame
with the inverse of T_B2S, so every case exercises the transform.  A case whose restatement misses the condition its
branch needs (tests/test_mcl_observation_cpu.py states them) is drawn again with the next seed, 50 times at most.
Answers are computed once per process and must not be modified."""
from __future__ import annotations

import functools
import math

import numpy as np

import mcl_observation_ref as R

F = np.float32
TOL, MIN_SIZE = 0.8, 3                      # p2p_move_base_localization.yaml


def _t_b2s():
    cy, sy, cp, sp = math.cos(0.3), math.sin(0.3), math.cos(0.04), math.sin(0.04)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    return np.concatenate([rz @ ry, np.array([[0.2], [-0.05], [0.45]])], axis=1)


T_B2S = _t_b2s()
T_B2S.setflags(write=False)


def to_sensor(p_base):
    p = np.asarray(p_base, np.float64).reshape(-1, 3)
    return ((p - T_B2S[:, 3]) @ T_B2S[:, :3]).astype(F)


def _wall(rng, n, axis, at, half, noise=0.01):
    """n points on the plane <axis> = at: the other horizontal coordinate in +-half, z in [0, 2]"""
    p = np.zeros((n, 3))
    p[:, axis] = at + rng.normal(0, noise, n)
    p[:, 1 - axis] = rng.uniform(-half, half, n)
    p[:, 2] = rng.uniform(0.0, 2.0, n)
    return p


def x_walls(rng):
    return np.concatenate([_wall(rng, 250, 0, 3.0, 8.0), _wall(rng, 250, 0, -3.0, 8.0), _wall(rng, 40, 1, 8.0, 3.0)])


def y_walls(rng):
    return x_walls(rng)[:, [1, 0, 2]]


def mixed(rng, n=600):
    """n points dealt to the four walls of a 6 m room in turn"""
    walls = [(0, 3.0), (1, 3.0), (0, -3.0), (1, -3.0)]
    per = [len(range(w, n, 4)) for w in range(4)]
    parts = [_wall(rng, per[w], a, at, 3.0) for w, (a, at) in enumerate(walls)]
    out = np.zeros((n, 3))
    for w in range(4):
        out[w::4] = parts[w]
    return out


def rings(rng):
    """8 horizontal lines of 64 points on the wall x = 3"""
    y, z = np.meshgrid(-8.0 + 0.25 * np.arange(64), 0.2 + 0.2 * np.arange(8))
    p = np.stack([np.full(y.size, 3.0), y.ravel(), z.ravel()], axis=1)
    return p + rng.normal(0, 0.01, p.shape) * np.array([1.0, 0.2, 0.2])


ISLAND_SIZES = (1,) * 5 + (2,) * 5 + (3,) * 22 + (4,) * 12


def islands(rng, n=725):
    """the mixed walls plus isolated groups of 1, 2, 3 and 4 points, 2 m apart and more than 0.8 m from everything, in a
    shuffled order: 22 groups of 3 and 12 of 4, so that the order inside the runs of equal sizes decides the output"""
    groups = []
    for g, size in enumerate(ISLAND_SIZES):
        c = np.array([-10.0 + 2.0 * (g % 11), 12.0 + 2.0 * (g // 11), 1.0])
        groups.append(c + rng.uniform(-0.15, 0.15, (size, 3)))
    groups = np.concatenate(groups)
    out = np.concatenate([groups, mixed(rng, n - len(groups))])
    return out[rng.permutation(len(out))]


def diagonal(rng, n):
    """n <= 5 points on the plane x + y = 4: one shared normal with |x| = |y|"""
    t, z = rng.uniform(-0.5, 0.5, n), rng.uniform(0.0, 1.0, n)
    return np.stack([2.0 + t, 2.0 - t, z], axis=1)


def flat_list(rng, n):
    """ground points of a sweep: negative coordinates, z values on 0.1 boundaries; the list of 2 shares a voxel"""
    if n == 2:
        return np.array([[-0.25, -0.75, 0.01], [-0.75, -0.25, 0.09]])
    p = np.stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.normal(0, 0.04, n)], axis=1)
    p[::3, 2] = rng.choice([-0.1, 0.0, 0.1, 0.2], len(p[::3]))
    return p


FLAT_COUNTS = (0, 1, 2, 100, 384)
CLUSTER_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 600, 1900)      # 1900 = 2000 - the 100 flat points it is prepared beside

_BUILDERS = {"x-walls": x_walls, "y-walls": y_walls, "rings": rings, "mixed": mixed, "islands": islands}
for _n in CLUSTER_COUNTS:
    if 0 < _n <= 5:
        _BUILDERS[f"mixed-{_n}"] = functools.partial(diagonal, n=_n)
    elif _n:
        _BUILDERS[f"mixed-{_n}"] = functools.partial(mixed, n=_n)
_BUILDERS["mixed-0"] = lambda rng: np.zeros((0, 3))
_BUILDERS["islands-600"] = functools.partial(islands, n=600)
_BUILDERS["islands-1900"] = functools.partial(islands, n=1900)

DOMINANT = ("x-walls", "y-walls", "rings")
CLUSTER = tuple(k for k in _BUILDERS if k not in DOMINANT)
NAMES = tuple(_BUILDERS)
NEAR_HALF = 0.02                          # |r - 0.5| below this: the 0.5 decision is left out of the comparison


def ratio(ref):
    sx, sy = ref["sum_x"], ref["sum_y"]
    return sx / sy if sy else math.inf


def condition(name, ref):
    """what the GPU tests rely on (the device's sums differ from the restatement's by its own float error only)"""
    if name in DOMINANT:
        q = ratio(ref)
        if not (q >= 3.0 or q <= 1.0 / 3.0):
            return False
        near = np.abs(ref["ratio"].astype(np.float64) - 0.5) < NEAR_HALF
        return near.mean() <= 0.02
    if len(ref["pts"]) < 3:
        return ref["branch"] == R.CLUSTERS                          # NaN normals, 0 / 0
    return 0.8 <= ratio(ref) <= 1.25


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (less-sharp list in the sensor frame [n,3], its restatement with no flat points, draws)"""
    base = 100 * (NAMES.index(name) + 1) + 1
    for attempt in range(50):
        ls = to_sensor(_BUILDERS[name](np.random.default_rng(base + attempt)))
        ref = R.prepare(np.zeros((0, 3), F), ls, T_B2S, TOL, MIN_SIZE)
        if condition(name, ref):
            ls.setflags(write=False)
            for v in ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            return ls, ref, attempt + 1
    raise AssertionError(f"case {name}: 50 draws and its condition still fails")


@functools.lru_cache(maxsize=None)
def flat_case(n):
    """-> (flat list in the sensor frame [n,3], the restatement's flat cloud)"""
    f = to_sensor(flat_list(np.random.default_rng(7000 + n), n))
    out = R.voxel_grid(R.transform(f, T_B2S))
    f.setflags(write=False)
    out.setflags(write=False)
    return f, out


@functools.lru_cache(maxsize=None)
def a_ref():
    """the normal bound: the largest angle between the restatement's float32 normal and the float64 eigh answer of the same
    neighbours, over all cases"""
    worst = 0.0
    for name in NAMES:
        _, ref, _ = case(name)
        a = R.angle(ref["normals"], R.normals_f64(ref["pts"], ref["nb"]))
        a = a[~np.isnan(a)]
        if len(a):
            worst = max(worst, float(a.max()))
    return worst
