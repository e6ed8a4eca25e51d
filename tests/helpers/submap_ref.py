"""Serial NumPy restatement of mcl_3dl's SubMaps (dddmr_mcl_3dl/src/sub_maps.cpp): the keyframes' transform
(readPoseGraph, :126-156), the keyframe radius search (:225-235), the concatenation and the ground normals of a warm-up
(:283-298, NormalEstimation with setKSearch(20)).  Built on mcl_observation_ref.py, whose transform, neighbours and
normals are the same third-party steps with k = 5.

UNPINNED, like that file: PCL, FLANN and Eigen cannot be built here.  The normals are restated from memory of PCL 1.15
(DESIGN.md 4e, N1-N7); the order of the radius search's result (the reference asks FLANN for an unsorted one) and its
comparison at the sphere are this library's statement, not the reference's.

A keyframe is a dict: corner [A,3], ground [B,3] float32, T (3x4 float64 or None), position (3 doubles)."""
from __future__ import annotations

import numpy as np

import mcl_observation_ref as R

F = np.float32
D = np.float64
K_SEARCH = 20
# A normal is compared only where the data define it: the two smallest eigenvalues of the neighbours' float64 covariance
# apart by more than this factor, and the middle one not vanishing beside the largest (a collinear neighbourhood).
GAP_FACTOR = 4.0
RANK_FLOOR = 1e-9


def stored(kf):
    """-> (corner, ground) as the store holds them: transformed once, rounded to float once"""
    c, g = np.asarray(kf["corner"], F).reshape(-1, 3), np.asarray(kf["ground"], F).reshape(-1, 3)
    if kf.get("T") is None:
        return c, g
    return R.transform(c, kf["T"]), R.transform(g, kf["T"])


def concatenate(keyframes, ids):
    """-> (map [M,3], ground [G,3]): the listed keyframes' corner clouds and ground clouds, in the list's order"""
    parts = [stored(keyframes[i]) for i in ids]
    cat = lambda v: np.concatenate(v).astype(F) if v else np.zeros((0, 3), F)
    return cat([p[0] for p in parts]), cat([p[1] for p in parts])


def neighbours(p, k=K_SEARCH):
    """-> [n, k] int32, -1 padded: the k nearest by (float d2, index), the point itself included"""
    p = np.asarray(p, F).reshape(-1, 3)
    out = np.full((len(p), k), -1, np.int32)
    nb = R.neighbours(p, k)
    out[:, : nb.shape[1]] = nb
    return out


def _rows(nb):
    nb = np.asarray(nb)
    have = int((nb[0] >= 0).sum()) if len(nb) else 0
    return nb[:, :have].astype(np.int64)


def normals(p, nb):
    return R.normals(np.asarray(p, F).reshape(-1, 3), _rows(nb))


def normals_f64(p, nb):
    return R.normals_f64(np.asarray(p, F).reshape(-1, 3), _rows(nb))


def defined(p, nb):
    """-> [n] bool: where the neighbours' float64 covariance defines a normal (GAP_FACTOR, RANK_FLOOR)"""
    p, rows = np.asarray(p, F).reshape(-1, 3), _rows(nb)
    ok = np.zeros(len(p), bool)
    if rows.shape[1] < 3:
        return ok
    for i in range(len(p)):
        w = np.linalg.eigvalsh(np.cov(p[rows[i]].astype(D).T, bias=True))
        l0, l1, l2 = max(w[0], 0.0), max(w[1], 0.0), max(w[2], 0.0)
        ok[i] = l1 > GAP_FACTOR * l0 and l1 > RANK_FLOOR * l2
    return ok


def select(kf_positions, position, radius):
    """-> ascending ids of the keyframes with float d2 <= float(radius * radius), and every keyframe's float d2"""
    k = np.asarray(kf_positions, D).reshape(-1, 3).astype(F)
    q = np.asarray(position, D).astype(F)
    d = (k[:, 0] - q[0]).astype(F)
    d2 = (d * d).astype(F)
    d = (k[:, 1] - q[1]).astype(F)
    d2 = (d2 + d * d).astype(F)
    d = (k[:, 2] - q[2]).astype(F)
    d2 = (d2 + d * d).astype(F)
    r2 = F(D(radius) * D(radius))
    return np.nonzero(d2 <= r2)[0].astype(np.int32), d2


def warm_up(keyframes, ids, k=K_SEARCH):
    """-> dict(map, ground, neighbours, normals, normals_f64, defined) of the warm-up generation"""
    m, g = concatenate(keyframes, ids)
    nb = neighbours(g, k)
    return dict(map=m, ground=g, neighbours=nb, normals=normals(g, nb), normals_f64=normals_f64(g, nb), defined=defined(g, nb))
