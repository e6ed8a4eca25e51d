"""Serial NumPy restatement of mcl_3dl's MCL3dlNode::cbLeGoFeatureCloud (dddmr_mcl_3dl/src/mcl_3dl.cpp:263-464): what
the localiser makes of a sweep's flat and less-sharp lists before measure() sees them.

UNPINNED: PCL, FLANN and Eigen cannot be built here, so the third-party steps are restated from memory of PCL 1.15
(DESIGN.md 4e numbers the assumptions N1-N7; oracle/ASSUMPTIONS.md rows 1, 2, 4, 7-10 for the rest).  float32 where the
reference is float, float64 where it is double, one IEEE operation per NumPy operation, neighbours by (d2, index).

  1 transform   pcl::transformPointCloud(Affine3d): double multiply-add left to right, one rounding to float (:295-296)
  2 flat        VoxelGrid, leaf (1.0f, 1.0f, 0.1f) (:306-309)
  3 normals     NormalEstimation, setKSearch(5), on the transformed less-sharp cloud itself (:320-329)
  4 sums        two double sums in index order, NaN components skipped one by one; the 1.6 rule (:340-360)
  5 dominant    every point in input order with its weight (:362-403)
  6 clusters    EuclideanClusterExtraction, libstdc++'s std::sort(rbegin, rend) over the sizes, weights (:404-443)
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
D = np.float64
CLUSTERS, X_DOMINANT, Y_DOMINANT = 0, 1, 2
LEAF = (F(1.0), F(1.0), F(0.1))


def transform(xyz, T):
    """row 4: x' = float(m00 x + m01 y + m02 z + m03) in double, left to right"""
    p = np.asarray(xyz, F).reshape(-1, 3).astype(D)
    T = np.asarray(T, D).reshape(3, 4)
    out = np.empty((len(p), 3), F)
    for r in range(3):
        out[:, r] = (((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]).astype(F)
    return out


def voxel_grid(pts, leaf=LEAF):
    """rows 7-8 with a per-axis inverse leaf: -> centroids [m,3] in voxel-index order"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    if len(pts) == 0:
        return np.zeros((0, 3), F)
    inv = np.array([F(1.0) / F(l) for l in leaf], F)
    ijk = np.floor(pts * inv[None, :]).astype(np.int64)
    lo, hi = ijk.min(axis=0), ijk.max(axis=0)
    dx, dy = int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)
    key = [int(v[0] - lo[0]) + int(v[1] - lo[1]) * dx + int(v[2] - lo[2]) * dx * dy for v in ijk]
    order = sorted(range(len(pts)), key=lambda i: (key[i], i))
    out = []
    i = 0
    while i < len(order):
        j = i
        s = np.zeros(3, F)
        while j < len(order) and key[order[j]] == key[order[i]]:
            s = (s + pts[order[j]]).astype(F)                       # float running sum, input order
            j += 1
        out.append(s / F(j - i))
        i = j
    return np.array(out, F).reshape(-1, 3)


def l2_matrix(p):
    """row 2: FLANN's L2_Simple in float, x y z order, for every pair"""
    d = (p[:, None, 0] - p[None, :, 0]).astype(F)
    r = d * d
    d = (p[:, None, 1] - p[None, :, 1]).astype(F)
    r = r + d * d
    d = (p[:, None, 2] - p[None, :, 2]).astype(F)
    return (r + d * d).astype(F)


def neighbours(p, k=5):
    """-> [n, min(k, n)] indices: the k nearest by (d2, index), the point itself included"""
    n = len(p)
    if n == 0:
        return np.zeros((0, 0), np.int64)
    d2 = l2_matrix(p)
    return np.argsort(d2, axis=1, kind="stable")[:, : min(k, n)]


def _roots2(b, c):
    d = b * b - F(4.0) * c
    d = np.where(d < 0, F(0.0), d).astype(F)
    sd = np.sqrt(d)
    return np.zeros_like(b), F(0.5) * (b - sd), F(0.5) * (b + sd)


def _roots(m00, m01, m02, m11, m12, m22):
    """N4: pcl::computeRoots, ascending; vectorised over the points"""
    with np.errstate(all="ignore"):
        c0 = m00 * m11 * m22 + F(2.0) * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
        c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12
        c2 = m00 + m11 + m22
        q0, q1, q2 = _roots2(c2, c1)
        s_inv3, s_sqrt3 = F(1.0 / 3.0), np.sqrt(F(3.0))
        c2_over_3 = c2 * s_inv3
        a_over_3 = (c1 - c2 * c2_over_3) * s_inv3
        a_over_3 = np.where(a_over_3 > 0, F(0.0), a_over_3).astype(F)
        half_b = F(0.5) * (c0 + c2_over_3 * (F(2.0) * c2_over_3 * c2_over_3 - c1))
        q = half_b * half_b + a_over_3 * a_over_3 * a_over_3
        q = np.where(q > 0, F(0.0), q).astype(F)
        rho = np.sqrt(-a_over_3)
        theta = (np.arctan2(np.sqrt(-q), half_b) * s_inv3).astype(F)
        ct, st = np.cos(theta).astype(F), np.sin(theta).astype(F)
        r0 = c2_over_3 + F(2.0) * rho * ct
        r1 = c2_over_3 - rho * (ct + s_sqrt3 * st)
        r2 = c2_over_3 - rho * (ct - s_sqrt3 * st)
        sw = r0 >= r1
        r0, r1 = np.where(sw, r1, r0), np.where(sw, r0, r1)
        sw = r1 >= r2
        r1, r2 = np.where(sw, r2, r1), np.where(sw, r1, r2)
        sw2 = sw & (r0 >= r1)
        r0, r1 = np.where(sw2, r1, r0), np.where(sw2, r0, r1)
        use2 = (np.abs(c0) < np.finfo(F).eps) | (r0 <= 0)
        return (np.where(use2, q0, r0).astype(F), np.where(use2, q1, r1).astype(F), np.where(use2, q2, r2).astype(F))


def normals(p, nb):
    """N1-N7: NormalEstimation::computePointNormal per point over its neighbours nb[i] -> [n,3] float32 (NaN rows for
    fewer than 3 neighbours and for a zero cross product)"""
    n = len(p)
    out = np.full((n, 3), np.nan, F)
    if n == 0 or nb.shape[1] < 3:
        return out
    k = nb.shape[1]
    with np.errstate(all="ignore"):
        K = p[nb[:, 0]]
        a = [np.zeros(n, F) for _ in range(9)]
        for q in range(k):
            g = p[nb[:, q]]
            x, y, z = g[:, 0] - K[:, 0], g[:, 1] - K[:, 1], g[:, 2] - K[:, 2]
            for s, v in enumerate((x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
                a[s] = a[s] + v
        a = [v / F(k) for v in a]
        m = [a[0] - a[6] * a[6], a[1] - a[6] * a[7], a[2] - a[6] * a[8], a[3] - a[7] * a[7], a[4] - a[7] * a[8], a[5] - a[8] * a[8]]
        scale = np.max(np.abs(np.stack(m)), axis=0)
        scale = np.where(scale <= np.finfo(F).tiny, F(1.0), scale).astype(F)
        m = [v / scale for v in m]
        r0, _, _ = _roots(*m)
        d0, d1, d2 = m[0] - r0, m[3] - r0, m[5] - r0
        rows = [(d0, m[1], m[2]), (m[1], d1, m[4]), (m[2], m[4], d2)]
        cr, ln = [], []
        for u, v in ((rows[0], rows[1]), (rows[0], rows[2]), (rows[1], rows[2])):
            c = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
            cr.append(c)
            ln.append(np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]))
        best = np.zeros(n, np.int64)
        best = np.where(ln[1] > ln[0], 1, best)
        lbest = np.where(best == 1, ln[1], ln[0])
        best = np.where(ln[2] > lbest, 2, best)
        lbest = np.where(best == 2, ln[2], lbest)
        nrm = np.stack([np.choose(best, [cr[0][c], cr[1][c], cr[2][c]]) / lbest for c in range(3)], axis=1).astype(F)
        vx, vy, vz = F(0.0) - p[:, 0], F(0.0) - p[:, 1], F(0.0) - p[:, 2]
        cos_theta = vx * nrm[:, 0] + vy * nrm[:, 1] + vz * nrm[:, 2]
        nrm = np.where((cos_theta < 0)[:, None], nrm * F(-1.0), nrm).astype(F)
    return nrm


def normals_f64(p, nb):
    """the float64 answer the float32 closed form is measured against: eigh of the neighbours' covariance"""
    out = np.full((len(p), 3), np.nan, D)
    if len(p) == 0 or nb.shape[1] < 3:
        return out
    for i in range(len(p)):
        g = p[nb[i]].astype(D)
        c = np.cov(g.T, bias=True)
        w, v = np.linalg.eigh(c)
        out[i] = v[:, 0]
    return out


def angle(a, b):
    """sign-free angle between unit vectors, rows; NaN where either is NaN"""
    a, b = np.asarray(a, D), np.asarray(b, D)
    with np.errstate(all="ignore"):
        cr = np.linalg.norm(np.cross(a, b), axis=1)
        dt = np.abs(np.sum(a * b, axis=1))
        return np.arctan2(cr, dt)


def sums(nrm):
    """:340-348 -> (sum_normal_x, sum_normal_y), double, index order"""
    sx = sy = 0.0
    for i in range(len(nrm)):
        if not math.isnan(float(nrm[i, 1])):
            sy += abs(float(nrm[i, 1]))
        if not math.isnan(float(nrm[i, 0])):
            sx += abs(float(nrm[i, 0]))
    return sx, sy


def _div(a, b):
    if b == 0.0:
        return math.nan if (a == 0.0 or math.isnan(a)) else math.copysign(math.inf, a)
    return a / b


def branch_of(sx, sy):
    if _div(sx, sy) >= 1.6:
        return X_DOMINANT
    if _div(sy, sx) >= 1.6:
        return Y_DOMINANT
    return CLUSTERS


def dominant_ratio(branch, nrm):
    """the float ratio step 5 compares with 0.5 (NaN where normal_x is NaN)"""
    with np.errstate(all="ignore"):
        r = (nrm[:, 1] / nrm[:, 0]) if branch == X_DOMINANT else (nrm[:, 0] / nrm[:, 1])
    return np.where(np.isnan(nrm[:, 0]), F(np.nan), r).astype(F)


def dominant_intensity(branch, nrm, sx, sy):
    r = dominant_ratio(branch, nrm).astype(D)
    low = F(0.05 * sy / sx) if branch == X_DOMINANT else F(0.05 * sx / sy)
    out = np.ones(len(nrm), F)
    out[(~np.isnan(nrm[:, 0])) & (r >= 0.5)] = low
    return out


# ---- libstdc++'s std::sort, replayed (bits/stl_algo.h: introsort with a threshold of 16, then insertion sort) ----------

def _std_sort(v, less):
    n = len(v)
    if n == 0:
        return

    def move_median_to_first(result, a, b, c):
        if less(v[a], v[b]):
            if less(v[b], v[c]):
                pick = b
            elif less(v[a], v[c]):
                pick = c
            else:
                pick = a
        elif less(v[a], v[c]):
            pick = a
        elif less(v[b], v[c]):
            pick = c
        else:
            pick = b
        v[result], v[pick] = v[pick], v[result]

    def unguarded_partition(first, last, pivot):
        while True:
            while less(v[first], v[pivot]):
                first += 1
            last -= 1
            while less(v[pivot], v[last]):
                last -= 1
            if not first < last:
                return first
            v[first], v[last] = v[last], v[first]
            first += 1

    def adjust_heap(first, hole, length, value):
        top = hole
        child = hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if less(v[first + child], v[first + child - 1]):
                child -= 1
            v[first + hole] = v[first + child]
            hole = child
        if (length & 1) == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            v[first + hole] = v[first + child - 1]
            hole = child - 1
        parent = (hole - 1) // 2
        while hole > top and less(v[first + parent], value):
            v[first + hole] = v[first + parent]
            hole = parent
            parent = (hole - 1) // 2
        v[first + hole] = value

    def heap_sort(first, last):
        length = last - first
        if length >= 2:
            parent = (length - 2) // 2
            while True:
                adjust_heap(first, parent, length, v[first + parent])
                if parent == 0:
                    break
                parent -= 1
        while last - first > 1:
            last -= 1
            value = v[last]
            v[last] = v[first]
            adjust_heap(first, 0, last - first, value)

    def introsort_loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                heap_sort(first, last)
                return
            depth -= 1
            mid = first + (last - first) // 2
            move_median_to_first(first, first + 1, mid, last - 1)
            cut = unguarded_partition(first + 1, last, first)
            introsort_loop(cut, last, depth)
            last = cut

    def unguarded_linear_insert(last):
        val = v[last]
        nxt = last - 1
        while less(val, v[nxt]):
            v[last] = v[nxt]
            last = nxt
            nxt -= 1
        v[last] = val

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if less(v[i], v[first]):
                val = v[i]
                v[first + 1: i + 1] = v[first:i]
                v[first] = val
            else:
                unguarded_linear_insert(i)

    introsort_loop(0, n, 2 * (n.bit_length() - 1))
    if n > 16:
        insertion_sort(0, 16)
        for i in range(16, n):
            unguarded_linear_insert(i)
    else:
        insertion_sort(0, n)


def cluster_order(kept_sizes):
    """row 10: std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters) on the kept clusters in creation order
    -> order[q] = which kept cluster is output q-th"""
    v = [(int(s), c) for c, s in enumerate(kept_sizes)][::-1]          # what the reverse iterators walk
    _std_sort(v, lambda a, b: a[0] < b[0])
    return [c for _, c in v[::-1]]


def cluster_intensity(size, n_points, min_size):
    w = (1.0 * size) / (1.0 * n_points)
    return F(w / 2.0) if size < min_size + 1 else F(w)


def euclidean_clusters(p, tol):
    """rows 1, 9: every cluster (ascending index arrays) in order of its lowest index, before the size filter"""
    n = len(p)
    if n == 0:
        return []
    tol2 = F(D(tol) * D(tol))
    adj = l2_matrix(p) < tol2
    seen = np.zeros(n, bool)
    out = []
    for s in range(n):
        if seen[s]:
            continue
        seen[s] = True
        queue = [s]
        at = 0
        while at < len(queue):
            for j in np.flatnonzero(adj[queue[at]] & ~seen):
                seen[j] = True
                queue.append(int(j))
            at += 1
        out.append(np.array(sorted(queue), np.int64))
    return out


def clusters_output(p, tol, min_size):
    """-> (less sharp [m,4], n_kept, n_small)"""
    n = len(p)
    kept = [c for c in euclidean_clusters(p, tol) if min_size <= len(c) <= n]
    order = cluster_order([len(c) for c in kept])
    rows = []
    for c in (kept[q] for q in order):
        w = cluster_intensity(len(c), n, min_size)
        rows.append(np.concatenate([p[c], np.full((len(c), 1), w, F)], axis=1))
    out = np.concatenate(rows).astype(F) if rows else np.zeros((0, 4), F)
    return out, len(kept), sum(1 for c in kept if len(c) < min_size + 1)


def prepare(flat_xyz, less_sharp_xyz, T_b2s, euc_cluster_distance=0.8, euc_cluster_min_size=3):
    """steps 1-7 -> dict(flat [a,3], ls [b,4], normals [n,3], nb, pts, branch, sum_x, sum_y, n_clusters,
    n_small_clusters, n_nan_normals, ratio)"""
    flat = voxel_grid(transform(np.asarray(flat_xyz, F).reshape(-1, 3 if np.size(flat_xyz) == 0 else np.shape(flat_xyz)[-1])[:, :3], T_b2s))
    p = transform(np.asarray(less_sharp_xyz, F).reshape(-1, 3 if np.size(less_sharp_xyz) == 0 else np.shape(less_sharp_xyz)[-1])[:, :3], T_b2s)
    nb = neighbours(p)
    nrm = normals(p, nb)
    sx, sy = sums(nrm)
    br = branch_of(sx, sy)
    out = dict(flat=flat, normals=nrm, nb=nb, pts=p, branch=br, sum_x=sx, sum_y=sy, n_nan_normals=int(np.isnan(nrm[:, 0]).sum()) if len(p) else 0,
               n_clusters=0, n_small_clusters=0, ratio=None)
    if br != CLUSTERS:
        out["ratio"] = dominant_ratio(br, nrm)
        out["ls"] = np.concatenate([p, dominant_intensity(br, nrm, sx, sy)[:, None]], axis=1).astype(F)
    else:
        out["ls"], out["n_clusters"], out["n_small_clusters"] = clusters_output(p, euc_cluster_distance, int(euc_cluster_min_size))
    return out
