"""NumPy restatement of mcl_3dl's LidarMeasurementModelLikelihood::measure
(dddmr_mcl_3dl/src/lidar_measurement_model_likelihood.cpp:86-252) for a batch of particles, with the lambda around it
(src/mcl_3dl.cpp:476-498): float32 where the reference is float, float64 where it is double.

PINNED to the reference's own code: lidar_measurement_model_likelihood.cpp, with state_6dof.h, quat.h, vec3.h and pf.h,
compiled unmodified against the stand-ins of oracle/ref/shim/ (oracle/ref/ref_mcl_driver.cpp, `make -C oracle ref`).
tests/test_mcl_measure_pin_cpu.py holds this file to it on bits -- quality, counts, branch, the float averages of the
normals, roll and roll_diff as doubles, likelihood, and State6DOF::transform through the reference's Quat and Vec3 -- and
tests/golden/REF_MCL_*.npz carry its answers to machines without the reference.  So the function's logic,
its float / double promotions and the transform are pinned.  Not pinned:
  * what the stand-ins encode of FLANN and tf2 (oracle/ASSUMPTIONS.md rows 1-3, 13, 14, 19):
    pcl::KdTreeFLANN::radiusSearch is FLANN's float L2_Simple distance ((dx*dx + dy*dy) + dz*dz), neighbours with
    d2 < static_cast<float>(radius * radius), sorted by ascending d2, with max_nn = 1 the nearest of them and the
    output vectors sized to the count found; tf2::Quaternion(axis, angle) divides by the axis' length;
    Quaternion::normalize multiplies by 1 / length; Matrix3x3(q).getRPY is setRotation + getEulerYPR "solution 1",
    whose gimbal branch takes roll = atan2(m21, m22) (no case reaches that branch);
  * the order of equal ground distances (ranked by ground index here and in the stand-in: `n_tied` counts where that
    could show, and the cases are drawn until it is 0);
  * the deliberate differences below, which the pin's cases leave out.
State6DOF::transform follows include/mcl_3dl/quat.h:87-93,131-143,175-178 and state_6dof.h:188-198 operation by
operation.

Deliberate differences from the reference: a state with a non-finite component gets likelihood 0 and
quality 0 (bad = True); a non-finite observation point, before or after the transform, matches nothing; with
threshold 0 and no ground neighbour the pose's nearest ground point is searched to d2 < 1.001 only (beyond that the
weight is 0.01 either way) and an empty ground gives 0.01 where the reference has no defined answer.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
from scipy.spatial import cKDTree

F = np.float32
MARGIN = 1e-9          # a decision of the double chain closer than this to its branch value counts as fragile
NN_D2 = F(1.001)


@dataclass
class Config:
    match_dist_min: float = 0.3
    match_dist_flat: float = 0.05
    radius_of_ground_search: float = 1.0
    threshold_for_trusted_ground: int = 6


def rotation(rot: np.ndarray) -> np.ndarray:
    """rot_.normalized() for [N,4] float32 x y z w: q * float(1.0 / double(norm))"""
    x, y, z, w = (rot[:, i] for i in range(4))
    n = np.sqrt(((x * x + y * y) + z * z) + w * w)                     # float32 throughout
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = (1.0 / n.astype(np.float64)).astype(F)
        return rot * s[:, None]


def _qmul(a, b):
    """Quat::operator*: every sum left to right, float32.  a, b: tuples (x, y, z, w) of broadcastable arrays"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz)


def transform(pos: np.ndarray, rot: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """State6DOF::transform of [M,3] points by N states -> [N,M,3] float32"""
    pos, rot, pts = np.asarray(pos, F).reshape(-1, 3), np.asarray(rot, F).reshape(-1, 4), np.asarray(pts, F).reshape(-1, 3)
    r = rotation(rot)
    rq = tuple(r[:, i][:, None] for i in range(4))
    zero = np.zeros((1, len(pts)), F)
    with np.errstate(invalid="ignore", over="ignore"):
        a = _qmul(rq, (pts[None, :, 0], pts[None, :, 1], pts[None, :, 2], zero))
        b = _qmul(a, (-rq[0], -rq[1], -rq[2], rq[3]))
        out = np.stack([b[0] + pos[:, 0][:, None], b[1] + pos[:, 1][:, None], b[2] + pos[:, 2][:, None]], axis=2)
    assert out.dtype == F
    return out


def l2(points: np.ndarray, q: np.ndarray) -> np.ndarray:
    """FLANN L2_Simple<float> of [K,3] points against one query"""
    d = points - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


class Cloud:
    """a kd-tree's stand-in: candidates from a float64 tree with a margin, the decision from FLANN's float distance"""

    def __init__(self, xyz):
        self.xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
        self.tree = cKDTree(self.xyz.astype(np.float64)) if len(self.xyz) else None

    def within(self, q, radius: float, r2):
        """(indices, d2) of the points with d2 < r2, unsorted"""
        if self.tree is None or not np.isfinite(q).all():
            return np.zeros(0, np.int64), np.zeros(0, F)
        idx = np.asarray(self.tree.query_ball_point(q.astype(np.float64), radius * 1.01 + 1e-2), np.int64)
        if len(idx) == 0:
            return idx, np.zeros(0, F)
        d2 = l2(self.xyz[idx], q)
        keep = d2 < r2
        return idx[keep], d2[keep]

    def nearest_many(self, qs, radius: float, r2):
        """per query the smallest d2 < r2, or +inf"""
        out = np.full(len(qs), np.inf, F)
        if self.tree is None:
            return out
        ok = np.isfinite(qs).all(axis=1)
        lists = self.tree.query_ball_point(qs[ok].astype(np.float64), radius * 1.01 + 1e-2)
        for i, idx in zip(np.nonzero(ok)[0], lists):
            if idx:
                d2 = l2(self.xyz[np.asarray(idx)], qs[i])
                m = d2.min()
                if m < r2:
                    out[i] = m
        return out


def weight_healthy(avg, rot, d2_nn, report=None):
    """:133-177 -> (pos_weight float32, n_fragile); report, when given, receives roll and roll_diff (doubles) where
    the 3x test lets the chain run"""
    avg_nx, avg_ny, avg_nz = (float(v) for v in avg)
    fragile = 0
    for a in (avg_nx, avg_ny):
        if abs(abs(a) - 3.0 * abs(avg_nz)) < MARGIN:
            fragile += 1
    if abs(avg_nx) >= 3.0 * abs(avg_nz) or abs(avg_ny) >= 3.0 * abs(avg_nz):
        return F(0.2), fragile
    nan = float("nan")
    ax, ay, az = avg_nx, avg_ny, avg_nz
    rx, ry, rz = ay * 1.0 - az * 0.0, az * 0.0 - ax * 1.0, ax * 0.0 - ay * 0.0       # axis.cross(up)
    dot = ax * 0.0 + ay * 0.0 + az * 1.0
    angle = -1.0 * math.acos(dot) if -1.0 <= dot <= 1.0 else nan
    d = math.sqrt(rx * rx + ry * ry + rz * rz)
    sn = math.sin(angle * 0.5) if math.isfinite(angle) else nan
    s = sn / d if d != 0.0 else (nan if (sn == 0.0 or sn != sn) else math.copysign(math.inf, sn))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.array([rx * s, ry * s, rz * s, math.cos(angle * 0.5) if math.isfinite(angle) else nan], np.float64)
        q = q * (np.float64(1.0) / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
        px, py, pz, pw = (np.float64(v) for v in rot)
        nx, ny, nz, nw = q
        x = pw * nx + px * nw + py * nz - pz * ny
        y = pw * ny + py * nw + pz * nx - px * nz
        z = pw * nz + pz * nw + px * ny - py * nx
        w = pw * nw - px * nx - py * ny - pz * nz
        inv = np.float64(1.0) / np.sqrt(x * x + y * y + z * z + w * w)
        x, y, z, w = x * inv, y * inv, z * inv, w * inv
        dd = x * x + y * y + z * z + w * w
        s2 = np.float64(2.0) / dd
        xs, ys, zs = x * s2, y * s2, z * s2
        wx, wy = w * xs, w * ys
        xx, xz, yy, yz = x * xs, x * zs, y * ys, y * zs
        m20, m21, m22 = float(xz - wy), float(yz + wx), float(1.0 - (xx + yy))
    if m20 != m20:
        roll = nan
    else:
        if abs(abs(m20) - 1.0) < MARGIN:
            fragile += 1
        if abs(m20) >= 1.0:
            roll = math.atan2(m21, m22)
        else:
            pitch = -math.asin(m20)
            roll = math.atan2(m21 / math.cos(pitch), m22 / math.cos(pitch))
    ar = abs(roll)
    for edge in (2.6, 3.1415926, 0.5):
        if abs(ar - edge) < MARGIN:
            fragile += 1
    if ar > 2.6 and ar < 3.1415926:
        roll_diff = 3.1415926 - ar
    elif ar >= 0 and ar < 0.5:
        roll_diff = ar
    else:
        roll_diff = 0.55
    if report is not None:
        report["roll"], report["roll_diff"] = roll, roll_diff
    wd = (1.0 - float(np.sqrt(F(d2_nn)))) * (1 - roll_diff)
    if wd != 0.0 and abs(wd) < MARGIN:
        fragile += 1
    pw_ = F(wd)
    if pw_ < 0:
        pw_ = F(0.01)
    return pw_, fragile


def measure(cfg: Config, map_xyz, ground_xyz, ground_normals, flat_xyz, less_sharp_xyzi, states) -> dict:
    """-> dict of per-particle arrays: likelihood, quality, score, pos_weight (float32), n_match, n_ground (uint32),
    healthy, bad (bool), n_fragile, n_tied (int); the intermediate values the reference logs, NaN where a particle's
    branch has none: avg [N,3] (float32, the averaged normal), roll, roll_diff (float64); and quality_min /
    quality_max, n_bad"""
    mdm, mdf = F(cfg.match_dist_min), F(cfg.match_dist_flat)
    r2_match = F(float(mdm) * float(mdm))
    rg = float(cfg.radius_of_ground_search)
    r2_ground = F(rg * rg)
    cmap, cground = Cloud(map_xyz), Cloud(ground_xyz)
    normals = np.ascontiguousarray(ground_normals, F).reshape(-1, 3)
    flat = np.ascontiguousarray(flat_xyz, F).reshape(-1, 3)
    ls = np.ascontiguousarray(less_sharp_xyzi, F).reshape(-1, 4)
    states = np.ascontiguousarray(states, F).reshape(-1, 7)
    N, n_obs = len(states), len(flat) + len(ls)
    assert n_obs > 0
    out = dict(likelihood=np.zeros(N, F), quality=np.zeros(N, F), score=np.zeros(N, F), pos_weight=np.zeros(N, F),
               n_match=np.zeros(N, np.uint32), n_ground=np.zeros(N, np.uint32), healthy=np.zeros(N, bool), bad=np.zeros(N, bool),
               n_fragile=np.zeros(N, np.int64), n_tied=np.zeros(N, np.int64), avg=np.full((N, 3), np.nan, F),
               roll=np.full(N, np.nan), roll_diff=np.full(N, np.nan))
    good = np.isfinite(states).all(axis=1)
    out["bad"] = ~good
    moved_flat = transform(states[:, :3], states[:, 3:], flat) if len(flat) else np.zeros((N, 0, 3), F)
    moved_ls = transform(states[:, :3], states[:, 3:], ls[:, :3]) if len(ls) else np.zeros((N, 0, 3), F)
    w_ls = ls[:, 3]
    for p in np.nonzero(good)[0]:
        pose = states[p, :3]
        idx, d2 = cground.within(pose, rg, r2_ground)
        cnt = len(idx)
        healthy = cnt >= cfg.threshold_for_trusted_ground
        fragile = tied = 0
        if healthy:
            order = np.lexsort((idx, d2))                            # FLANN's sorted result; ties by ground index
            idx, d2 = idx[order], d2[order]
            same = np.nonzero(d2[1:] == d2[:-1])[0]
            tied = int(sum((normals[idx[i]] != normals[idx[i + 1]]).any() for i in same))
            avg = np.zeros(3, F)
            for i in idx:
                n = normals[i]
                avg = avg + np.array([n[0], n[1], np.abs(n[2])], F)   # float sums in sorted order
            with np.errstate(invalid="ignore", divide="ignore"):
                avg = avg / F(cnt)
            if cnt:
                d2_nn = d2[0]
            else:
                near = cground.nearest_many(pose[None, :], float(np.sqrt(NN_D2)), NN_D2)[0]
                d2_nn = near if np.isfinite(near) else F(4.0)
            report = {}
            pw, fragile = weight_healthy(avg, states[p, 3:], d2_nn, report)
            out["avg"][p] = avg
            if report:
                out["roll"][p], out["roll_diff"][p] = report["roll"], report["roll_diff"]
        else:
            near = cmap.nearest_many(pose[None, :], float(np.sqrt(NN_D2)), NN_D2)[0]
            pw = F(0.01)
            if np.isfinite(near):
                wd = 1.0 - float(np.sqrt(F(near)))
                pw = F(wd)
                if pw < 0:
                    pw = F(0.01)
        score, num = F(0), 0
        near_flat = (cground if healthy else cmap).nearest_many(moved_flat[p], float(mdm), r2_match)
        near_ls = cmap.nearest_many(moved_ls[p], float(mdm), r2_match)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for d2m, w in list(zip(near_flat, [None] * len(near_flat))) + list(zip(near_ls, w_ls)):
                if not np.isfinite(d2m):
                    continue
                dist = F(mdm - max(np.sqrt(F(d2m)), mdf))
                if dist < 0:
                    continue
                score = F(score + (dist * dist if w is None else F(dist * dist) / w))
                num += 1
            out["likelihood"][p] = F(score * pw)
        out["score"][p], out["pos_weight"][p], out["n_match"][p], out["n_ground"][p] = score, pw, num, cnt
        out["healthy"][p], out["n_fragile"][p], out["n_tied"][p] = healthy, fragile, tied
        out["quality"][p] = F(num) / F(n_obs)
    q_min, q_max = F(1.0), F(0.0)
    for q in out["quality"]:                                          # mcl_3dl.cpp:495-498 (a refused state's 0 takes part)
        if q_min > q:
            q_min = q
        if q_max < q:
            q_max = q
    out["quality_min"], out["quality_max"], out["n_bad"] = q_min, q_max, int((~good).sum())
    return out
