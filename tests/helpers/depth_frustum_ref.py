"""NumPy restatement of the depth camera's frustum, its two point tests and selfClear's clearing verdicts: the
yardstick of tests/test_depth_frustum_cpu.py and tests/test_depth_clear_gpu.py.

Written from the reference source (paths relative to dddmr_perception_3d/plugins/depth_camera/), float32 / float64
exactly where the reference's types put them; it imports nothing from the library under test.
  Frustum                     depth_camera_observation_buffer.cpp:148-174, depth_camera_observation.cpp:85-239
  in_frustums / attach        frustum_utils.cpp:124-290
  clear_verdicts              depth_camera_layer.cpp:252-264, :324-422
Every operand of a plane distance, a normal and a `test` dot product is a float, so C++ evaluates them in float (`test`
only widens the finished sum to double); fabs / sqrt on floats are the float overloads (oracle/ASSUMPTIONS.md row 18);
hypot gets (float - double) arguments and is the double one; radiusSearch is FLANN's float L2_Simple against
static_cast<float>(r * r), strict < (oracle/ASSUMPTIONS.md row 1).

Besides its answers every function reports the MARGIN of the comparisons it made, so that a test can draw its inputs by
rejection from this file alone (MARGIN_* below): an input whose comparison sits closer to its threshold than that is not
used, because there a last-ulp difference between two correct implementations (the double hypot, a float division)
could decide.
"""
import math

import numpy as np
from scipy.spatial import cKDTree

import depth_feed_ref as F

MARGIN_TEST = 1e-4        # |test| of every frustum dot product, and |hypot - (max_detect_distance + 0.5)|
MARGIN_DIS = 1e-4         # |dis - 0.12| of every plane distance
MARGIN_D2 = 1e-6          # |d^2 - r^2| / r^2 of every (query, observation point) pair within 2 r
DIS2REJ = np.float32(0.12)

f32 = np.float32
TLN, TRN, BLN, BRN, TLF, TRF, BLF, BRF = range(8)


def _cross(u, w):
    """getCrossProduct (depth_camera_observation.cpp:85-96): float, the y term times -1.0 in double"""
    return np.array([u[1] * w[2] - u[2] * w[1],
                     f32(np.float64(u[0] * w[2] - u[2] * w[0]) * -1.0),
                     u[0] * w[1] - u[1] * w[0]], dtype=f32)


def _plane(p1, p2, p3):
    """getPlaneN (:99-112)"""
    a1, b1, c1 = p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]
    a2, b2, c2 = p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]
    a = b1 * c2 - b2 * c1
    b = a2 * c1 - a1 * c2
    c = a1 * b2 - b1 * a2
    d = (-a * p1[0] - b * p1[1]) - c * p1[2]
    return np.array([a, b, c, d], dtype=f32)


class Frustum:
    """What one DepthCameraObservation holds after bufferCloud: frustum_, frustum_normal_, frustum_plane_equation_,
    BRNear_, TLFar_, origin_ (doubles), max_detect_distance_."""

    def __init__(self, fov_w, fov_v, min_d, max_d, T_gbl_sensor):
        tw, tv = math.tan(float(fov_w) / 2.0), math.tan(float(fov_v) / 2.0)
        v = []
        for d in (float(min_d), float(max_d)):           # findFrustumVertex (:114-127): doubles into PointXYZ floats
            v += [(d, d * tw, d * tv), (d, -d * tw, d * tv), (d, d * tw, -d * tv), (d, -d * tw, -d * tv)]
        self.local = np.array(v, dtype=np.float64).astype(f32)
        self.vtx = F.transform(self.local, T_gbl_sensor)     # pcl::transformPointCloud by the Affine3d of m2s
        V = self.vtx
        vec = lambda a, b: V[b] - V[a]                   # getVec(vec1, vec2) = vec2 - vec1, float
        self.nrm = np.stack([_cross(vec(TLN, TRN), vec(TRN, BRN)),      # findFrustumNormal (:130-200)
                             _cross(vec(TRN, TRF), vec(TRF, BRF)),
                             _cross(vec(BRN, BRF), vec(BRF, BLF)),
                             _cross(vec(BLN, BLF), vec(BLF, TLF)),
                             _cross(vec(BRF, TRF), vec(TRF, TLF)),
                             _cross(vec(TLF, TRF), vec(TRF, TRN))])
        self.pl = np.stack([_plane(V[TLN], V[TLF], V[BLN]), _plane(V[BLN], V[BRN], V[BLF]),   # findFrustumPlane (:202-239)
                            _plane(V[TRN], V[BRN], V[BRF]), _plane(V[TLN], V[TRN], V[TLF]),
                            _plane(V[TLN], V[BLN], V[BRN]), _plane(V[TLF], V[TRF], V[BRF])])
        self.origin = np.asarray(T_gbl_sensor[:3], dtype=np.float64)
        self.max_d = float(max_d)

    def tests(self, P):
        """the six `test` values of every point, [N,6] float64 (float sums widened)"""
        P = np.asarray(P, dtype=f32)
        out = np.empty((len(P), 6), np.float64)
        for i in range(6):
            c = self.vtx[BRN if i < 3 else TLF]
            v = P - c
            n = self.nrm[i]
            out[:, i] = ((v[:, 0] * n[0] + v[:, 1] * n[1]) + v[:, 2] * n[2]).astype(np.float64)
        return out

    def plane_attach(self, P):
        """-> (attaches [N,6] bool, dis [N,6] float32, hyp [N] float64)"""
        P = np.asarray(P, dtype=f32)
        dis = np.empty((len(P), 6), f32)
        for i in range(6):
            a, b, c, d = self.pl[i]
            num = np.abs(((a * P[:, 0] + b * P[:, 1]) + c * P[:, 2]) + d)
            dis[:, i] = num / np.sqrt((a * a + b * b) + c * c)
        hyp = np.hypot(P[:, 0].astype(np.float64) - self.origin[0], P[:, 1].astype(np.float64) - self.origin[1])
        near = hyp < self.max_d + 0.5
        return (dis <= DIS2REJ) & near[:, None], dis, hyp


def point_tests(frustums, P):
    """isinFrustumsObservations and isAttachFRUSTUMs over the cameras in order -> (in_frustums [N], attach [N],
    ok [N]: every comparison made for the point keeps its margin)."""
    P = np.asarray(P, dtype=f32)
    n = len(P)
    inside_s, attach_s, wo_s = [], [], []
    ok = np.ones(n, bool)
    for fr in frustums:
        t = fr.tests(P)
        att, dis, hyp = fr.plane_attach(P)
        ok &= (np.abs(t) >= MARGIN_TEST).all(axis=1)
        ok &= (np.abs(dis.astype(np.float64) - float(DIS2REJ)) >= MARGIN_DIS).all(axis=1)
        ok &= np.abs(hyp - (fr.max_d + 0.5)) >= MARGIN_TEST
        ins = ~(t < 0).any(axis=1)
        inside_s.append(ins)
        attach_s.append(att.any(axis=1))
        wo_s.append(~att.any(axis=1) & ins)              # isInsideFRUSTUMwoAttach
    in_frustums = np.any(inside_s, axis=0)
    # isAttachFRUSTUMs returns at the first plane of the first camera that attaches: true unless ANOTHER camera holds the
    # point inside and unattached.  Which plane it was does not enter the answer, which camera does.
    attach = np.zeros(n, bool)
    decided = np.zeros(n, bool)
    for s in range(len(frustums)):
        first = attach_s[s] & ~decided
        other = np.zeros(n, bool)
        for t in range(len(frustums)):
            if t != s:
                other |= wo_s[t]
        attach[first] = ~other[first]
        decided |= first
    return in_frustums, attach, ok


def radius_any(obs, Q, r):
    """pcl::KdTreeFLANN::radiusSearch(q, r, ..., 1) > 0 for every query -> (hit [N] bool, ok [N] bool: no pair within
    2 r has |d^2 - r^2| < MARGIN_D2 * r^2)."""
    obs = np.asarray(obs, dtype=f32).reshape(-1, 3)
    Q = np.asarray(Q, dtype=f32).reshape(-1, 3)
    hit, ok = np.zeros(len(Q), bool), np.ones(len(Q), bool)
    if not len(obs) or not len(Q):
        return hit, ok
    r2 = f32(float(r) * float(r))                         # static_cast<float>(r * r)
    pairs = cKDTree(Q.astype(np.float64)).sparse_distance_matrix(cKDTree(obs.astype(np.float64)), 2.0 * float(r),
                                                                  output_type="ndarray")
    i, j = pairs["i"], pairs["j"]
    d = obs[j, 0] - Q[i, 0]                               # flann::L2_Simple: float differences squared, summed in order
    d2 = d * d
    d = obs[j, 1] - Q[i, 1]
    d2 = d2 + d * d
    d = obs[j, 2] - Q[i, 2]
    d2 = d2 + d * d
    hit[i[d2 < r2]] = True
    ok[i[np.abs(d2.astype(np.float64) - float(r2)) < MARGIN_D2 * float(r2)]] = False
    return hit, ok


def clear_verdicts(frustums, obs, xy_res, h_res, voxels, offsets, cluster):
    """selfClear's tree for every marking -> (verdict [M] uint8: bit 0 kept, bits 1-2 branch 1 outside / 2 attached /
    3 inside; engaged [M] uint32; ok [M]: every comparison made for the marking keeps its margin, the ratio included)."""
    voxels = np.asarray(voxels, dtype=np.int32).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    cluster = np.asarray(cluster, dtype=f32).reshape(-1, 3)
    obs = np.asarray(obs, dtype=f32).reshape(-1, 3)
    m = len(voxels)
    pt = np.stack([(voxels[:, 0] * np.float64(xy_res)).astype(f32), (voxels[:, 1] * np.float64(xy_res)).astype(f32),
                   (voxels[:, 2] * np.float64(h_res)).astype(f32)], axis=1)          # :325-327
    observation_clear = not (len(obs) > 5)                                          # :258-264
    inside, attach, ok = point_tests(frustums, pt)
    branch = np.where(~inside, 1, np.where(attach, 2, 3)).astype(np.uint8)
    kept = np.zeros(m, bool)
    engaged = np.zeros(m, np.uint32)
    if not observation_clear:
        near, near_ok = radius_any(obs, pt, 0.05)                                    # :336
        out = branch == 1
        kept[out] = near[out]
        ok[out] &= near_ok[out]
        hit, hit_ok = radius_any(obs, cluster, 0.01)                                 # :370, :402
        size = offsets[1:] - offsets[:-1]
        owner = np.repeat(np.arange(m), size)
        eng = np.bincount(owner, weights=hit, minlength=m).astype(np.int64)
        bad = np.bincount(owner, weights=~hit_ok, minlength=m) > 0
        ratio = ~out
        if (size[ratio] == 0).any():
            raise ZeroDivisionError("a marking reaches the engagement ratio with an empty cluster")
        s = np.maximum(size, 1).astype(np.float64)
        k = 1.0 * eng / s > 0.1                                                      # :374, :406
        # the ratio must not sit within one count of 0.1
        k_lo, k_hi = 1.0 * (eng - 1) / s > 0.1, 1.0 * (eng + 1) / s > 0.1
        kept[ratio] = k[ratio]
        engaged[ratio] = eng[ratio]
        ok[ratio] &= ~bad[ratio] & (k_lo == k)[ratio] & (k_hi == k)[ratio]
    verdict = (branch << 1) | kept.astype(np.uint8)
    return verdict.astype(np.uint8), engaged, ok


def ulp_diff(a, b):
    """largest difference of two float32 arrays in units in the last place (of the larger magnitude)"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    if a.size == 0:
        return 0.0
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32)).astype(np.float64)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp))
