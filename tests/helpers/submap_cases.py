"""The sub-map cases shared by tests/test_submap_cpu.py and tests/test_submap_gpu.py: seeded keyframe sets, the id list of
the warm-up, and the restatement's answer (computed once per case, read-only).

  a  a jittered floor of overlapping keyframes, 0.25 m spacing, +-1 cm
  b  two floors 3 m apart
  c  a ramp
  d  an exact 0.25 m lattice (many equal d2: the ties go by index)
  e  the same keyframe's points in two keyframes (d2 = 0 ties)
  f  a plus one point 30 m away and one 400 m away
  g  a shifted by (5000, -3000, 40) m
  h-N  ground totals of 0, 1, 2, 3, 19, 20 and 21 points
  i  a keyframe with an empty ground cloud and one with an empty corner cloud
  j  keyframes given in their own frames with a 3x4 transform, roll, pitch and yaw all non-zero
"""
from __future__ import annotations

import functools

import numpy as np

import mcl_measure_cases as MC
import submap_ref as S

F = np.float32
SHIFT = np.array([5000.0, -3000.0, 40.0])
H_TOTALS = (0, 1, 2, 3, 19, 20, 21)
NAMES = ("a", "b", "c", "d", "e", "f", "g") + tuple(f"h-{n}" for n in H_TOTALS) + ("i", "j")
SMOOTH = ("a", "b", "c", "f", "g", "j")          # the cases the excluded share is capped over
EXCLUDED_CAP = 0.02
SEEDS = {n: 4100 + 17 * i for i, n in enumerate(NAMES)}


def patch(rng, x0, y0, nx, ny, z=lambda x, y: 0.0 * x, jitter=0.01, spacing=0.25):
    """nx x ny floor points from (x0, y0), float64"""
    gx, gy = np.meshgrid(x0 + spacing * np.arange(nx), y0 + spacing * np.arange(ny), indexing="ij")
    p = np.stack([gx.ravel(), gy.ravel(), z(gx.ravel(), gy.ravel())], axis=1)
    return p + rng.uniform(-jitter, jitter, p.shape) if jitter else p


def corners(rng, x0, y0, n):
    """n wall-like points beside a patch"""
    return np.stack([x0 + rng.uniform(0, 5, n), y0 + rng.choice([0.0, 5.0], n) + rng.normal(0, 0.02, n), rng.uniform(0, 2, n)], axis=1)


def keyframe(corner, ground, T=None, position=None):
    g = np.asarray(ground, np.float64).reshape(-1, 3)
    c = np.asarray(corner, np.float64).reshape(-1, 3)
    if position is None:
        position = g.mean(axis=0) if len(g) else (c.mean(axis=0) if len(c) else np.zeros(3))
    return dict(corner=c.astype(F), ground=g.astype(F), T=T, position=np.asarray(position, np.float64))


def floor(rng, shift=None, z=lambda x, y: 0.0 * x, origins=((0, 0), (3, 0), (0, 3), (3, 3)), n=20):
    kfs = []
    for (x0, y0) in origins:
        g, c = patch(rng, x0, y0, n, n, z), corners(rng, x0, y0, int(rng.integers(60, 200)))
        if shift is not None:
            g, c = g + shift, c + shift
        kfs.append(keyframe(c, g))
    return kfs


def _a(rng):
    return floor(rng), [2, 0, 3, 1]


def _b(rng):
    lower = floor(rng, origins=((0, 0), (3, 0)), n=18)
    upper = floor(rng, origins=((0, 0), (3, 0)), n=18, z=lambda x, y: 3.0 + 0.0 * x)
    return lower + upper, [0, 2, 1, 3]


def _c(rng):
    return floor(rng, z=lambda x, y: 0.3 * x + 0.05 * y, origins=((0, 0), (3, 0), (6, 0)), n=20), [0, 1, 2]


def _d(rng):
    kfs = [keyframe(corners(rng, x0, 0, 80), patch(rng, x0, 0.0, 16, 20, z=lambda x, y: 0.5 + 0.0 * x, jitter=0.0)) for x0 in (0.0, 4.0, 8.0)]
    return kfs, [1, 0, 2]


def _e(rng):
    g = patch(rng, 0, 0, 18, 18)
    c = corners(rng, 0, 0, 90)
    return [keyframe(c, g), keyframe(corners(rng, 3, 0, 70), patch(rng, 3, 0, 18, 18)), keyframe(c, g)], [0, 1, 2]


def _f(rng):
    kfs, ids = _a(rng)
    last = kfs[-1]
    far = np.array([[36.0, 2.0, 0.1], [405.0, 1.0, 0.3]])
    kfs[-1] = keyframe(last["corner"], np.concatenate([last["ground"].astype(np.float64), far]), position=last["position"])
    return kfs, ids


def _g(rng):
    return floor(rng, shift=SHIFT), [2, 0, 3, 1]


def _h(total):
    def build(rng):
        g = patch(rng, 0, 0, 5, 5)[rng.permutation(25)[:total]] if total else np.zeros((0, 3))
        half = total // 2
        return [keyframe(corners(rng, 0, 0, 50), g[:half], position=(0, 0, 0)), keyframe(corners(rng, 0, 0, 50), g[half:], position=(1, 0, 0))], [0, 1]
    return build


def _i(rng):
    kfs = floor(rng, origins=((0, 0), (3, 0)), n=16)
    kfs.insert(1, keyframe(corners(rng, 1, 1, 120), np.zeros((0, 3))))                 # no ground
    kfs.append(keyframe(np.zeros((0, 3)), patch(rng, 1, 3, 16, 10)))                    # no corner
    return kfs, [0, 1, 2, 3]


def _j(rng):
    kfs = []
    for (x0, y0) in ((0, 0), (3, 1), (1, 4)):
        g, c = patch(rng, x0, y0, 18, 18, z=lambda x, y: 0.1 * y), corners(rng, x0, y0, 100)
        rpy = rng.uniform(0.05, 0.3, 3) * rng.choice([-1, 1], 3) + np.array([0, 0, rng.uniform(0.5, 2.5)])
        Rm = MC.rot_matrix(MC.quat_rpy(*rpy))
        t = np.array([x0 + 2.0, y0 + 2.0, 0.4]) + rng.normal(0, 0.1, 3)
        T = np.concatenate([Rm, t[:, None]], axis=1)
        assert min(abs(rpy)) > 0.04
        kfs.append(keyframe((c - t) @ Rm, (g - t) @ Rm, T=T, position=t))
    return kfs, [2, 0, 1]


_BUILDERS = dict(a=_a, b=_b, c=_c, d=_d, e=_e, f=_f, g=_g, i=_i, j=_j, **{f"h-{n}": _h(n) for n in H_TOTALS})


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (keyframes, ids, ref): ref is submap_ref.warm_up of the list"""
    kfs, ids = _BUILDERS[name](np.random.default_rng(SEEDS[name]))
    ref = S.warm_up(kfs, ids)
    for kf in kfs:
        for v in kf.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    for v in ref.values():
        v.setflags(write=False)
    return kfs, tuple(ids), ref


def restatement_error(name):
    """-> (largest angle of the restatement's float normals to normals_f64 over the compared points, compared, excluded,
    NaN normals)"""
    _, _, ref = case(name)
    nan = np.isnan(ref["normals"][:, 0])
    cmp_ = ~nan & ref["defined"]
    ang = S.R.angle(ref["normals"][cmp_], ref["normals_f64"][cmp_]) if cmp_.any() else np.zeros(0)
    return (float(ang.max()) if len(ang) else 0.0), int(cmp_.sum()), int((~nan & ~ref["defined"]).sum()), int(nan.sum())


def select_case(seed, n=200, radius=50.0):
    """random keyframe positions around a query, none within 1 mm of the sphere -> (positions [n,3], query, radius)"""
    rng = np.random.default_rng(seed)
    for _ in range(100):
        q = rng.uniform(-200, 200, 3) * np.array([1, 1, 0.05])
        k = q + rng.uniform(-90, 90, (n, 3)) * np.array([1, 1, 0.1])
        d = np.linalg.norm(k.astype(F).astype(np.float64) - q.astype(F).astype(np.float64), axis=1)
        if (np.abs(d - radius) >= 1e-3).all():
            return k, q, radius
    raise AssertionError("select_case: 100 draws and still a keyframe within 1 mm of the sphere")
