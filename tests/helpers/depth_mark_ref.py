"""NumPy / SciPy restatement of DepthCameraLayer::selfMark from the aggregated observation on: the yardstick of
tests/test_depth_mark_cpu.py and tests/test_depth_mark_gpu.py.

Written from the reference source (dddmr_perception_3d/plugins/depth_camera/depth_camera_layer.cpp:487-601), float32 /
float64 exactly where the reference's types put them; it imports nothing from the library under test.
  1 clustering   pcl::extractEuclideanClusters: FLANN's float L2_Simple against static_cast<float>(tol * tol), strict <
                 (oracle/ASSUMPTIONS.md row 1); clusters in order of their lowest point index, each cluster's indices
                 ascending (rows 2, 9); kept iff min_cluster_size <= size
  2 order        std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters) (row 10): descending size.  Here a
                 STABLE sort: the order inside a run of equal sizes is libstdc++'s introsort's and a test compares such
                 a run as a set
  3 centroid     float running sums in ascending point index, each divided by (float)size (:514-533)
  4 ground       radiusSearch(centroid, 0.1) on the ground cloud (:539)
  5 VoxelGrid    0.2 m (:545-548; rows 7, 8): depth_feed_ref.voxel_centroids
  6 static map   the loop of :552-562, which searches with the CENTROID for every downsampled point
  7 frustums     isinFrustumsObservations(centroid) on the raw float centroid (:591): depth_frustum_ref.point_tests
  8 outputs      addPCPtr's voxel key (int)(c / resolution) (a float divided by a double, truncated); the plane of :568-578
Float sums are sequential: np.cumsum / np.add.at, never np.sum (pairwise).

Every cluster also reports the MARGIN of each comparison that is not plain shared float arithmetic (`margins`): the
nearest ground / map node against 0.1 m, the frustum tests (depth_frustum_ref's own margins), the distance of
c / resolution from an integer (relative to the quotient) and hit against size * ratio.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import depth_feed_ref as F
import depth_frustum_ref as R

f32 = np.float32
BELOW_MIN, GROUND, STATIC, OUTSIDE, ACCEPTED = range(5)
MARGIN_RADIUS = 1e-4      # metres between the nearest ground / map node and the 0.1 m radius
MARGIN_KEY = 1e-6         # |q - nearest integer| / |q| of every voxel-key quotient q = c / resolution


def _l2_simple(a, b):
    d = a[:, 0] - b[:, 0]
    d2 = d * d
    d = a[:, 1] - b[:, 1]
    d2 = d2 + d * d
    d = a[:, 2] - b[:, 2]
    return d2 + d * d


def euclidean_clusters(obs, tol):
    """-> list of index arrays (ascending), in order of their lowest index: every cluster, before the size filter"""
    obs = np.asarray(obs, dtype=f32).reshape(-1, 3)
    n = len(obs)
    pairs = cKDTree(obs.astype(np.float64)).query_pairs(float(tol) * 1.001 + 1e-5, output_type="ndarray")
    if len(pairs):
        keep = _l2_simple(obs[pairs[:, 0]], obs[pairs[:, 1]]) < f32(float(tol) * float(tol))
        pairs = pairs[keep]
    g = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n)) if len(pairs) else coo_matrix((n, n), dtype=np.int8)
    _, lab = connected_components(g, directed=False)
    order = np.argsort(lab, kind="stable")                       # members ascending inside a label
    bounds = np.flatnonzero(np.diff(lab[order])) + 1
    groups = np.split(order, bounds)
    groups.sort(key=lambda idx: int(idx[0]))
    return groups


def _nearest(tree, c):
    if tree is None:
        return np.inf
    return float(tree.query(np.asarray(c, dtype=np.float64))[0])


def plane(T_gbl_base):
    """:568-578: tf2::quatRotate(q, (0, 0, 1)) and d in double, each rounded to float"""
    x, y, z, w = (float(v) for v in T_gbl_base[3:7])
    ax, ay, az, aw = y, -x, w, -z                                 # q * (0, 0, 1, 0)
    bx, by, bz, bw = -x, -y, -z, w                                # q^-1
    n = (aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx)
    d = -float(T_gbl_base[0]) * n[0] - float(T_gbl_base[1]) * n[1] - float(T_gbl_base[2]) * n[2]
    return np.array([n[0], n[1], n[2], d], dtype=np.float64).astype(f32)


def self_mark(frustums, obs, ground, smap, xy_res, h_res, tol, min_size, ratio, T_gbl_base):
    """-> dict: stats (the counts of dddmr_depth_mark_stats), clusters (every kept cluster in the reference's processing
    order: dicts of size, centroid, fate, voxel, points, margins), plane"""
    obs = np.asarray(obs, dtype=f32).reshape(-1, 3)
    ground = np.asarray(ground, dtype=f32).reshape(-1, 3)
    smap = np.asarray(smap, dtype=f32).reshape(-1, 3)
    stats = dict(n_observation=len(obs), n_clusters=0, n_ground_rejected=0, n_static_rejected=0, n_outside_frustums=0,
                 n_accepted=0, n_points=0)
    out = dict(stats=stats, clusters=[], plane=plane(T_gbl_base))
    if len(obs) <= 5:                                              # :491
        return out
    kept = [idx for idx in euclidean_clusters(obs, tol) if len(idx) >= int(min_size)]
    kept.sort(key=lambda idx: -len(idx))                           # stable: descending size, creation order inside a run
    gtree = cKDTree(ground.astype(np.float64)) if len(ground) else None
    mtree = cKDTree(smap.astype(np.float64)) if len(smap) else None
    cents = np.zeros((len(kept), 3), f32)
    for i, idx in enumerate(kept):
        p = obs[idx]
        s = np.array([np.cumsum(p[:, a], dtype=f32)[-1] for a in range(3)], dtype=f32)
        cents[i] = s / f32(len(idx))
    g_hit, _ = R.radius_any(ground, cents, 0.1)
    m_hit, _ = R.radius_any(smap, cents, 0.1)
    inside, _, fr_ok = R.point_tests(frustums, cents)
    for i, idx in enumerate(kept):
        c = cents[i]
        q = np.array([np.float64(c[0]) / np.float64(xy_res), np.float64(c[1]) / np.float64(xy_res), np.float64(c[2]) / np.float64(h_res)])
        key_margin = float(np.min(np.abs(q - np.rint(q)) / np.maximum(np.abs(q), 1e-300)))
        cl = dict(size=len(idx), centroid=c, voxel=np.trunc(q).astype(np.int32), points=np.zeros((0, 3), f32),
                  margins=dict(ground=abs(_nearest(gtree, c) - 0.1), map=abs(_nearest(mtree, c) - 0.1), frustum_ok=bool(fr_ok[i]),
                               key=key_margin, hit=np.inf))
        out["clusters"].append(cl)
        if g_hit[i]:
            cl["fate"] = GROUND
            stats["n_ground_rejected"] += 1
            continue
        ds, _ = F.voxel_centroids(obs[idx], 0.2)
        nds = len(ds)
        hit = 0
        if float(ratio) <= 0.999:
            for _ in range(nds):
                if m_hit[i]:
                    hit += 1
                    cl["margins"]["hit"] = min(cl["margins"]["hit"], abs(hit - nds * float(ratio)))
                    if hit > nds * float(ratio):
                        break
        cl["margins"]["hit"] = min(cl["margins"]["hit"], abs(hit - nds * float(ratio)))
        if not hit <= nds * float(ratio):
            cl["fate"] = STATIC
            stats["n_static_rejected"] += 1
            continue
        if not inside[i]:
            cl["fate"] = OUTSIDE
            stats["n_outside_frustums"] += 1
            continue
        cl["fate"] = ACCEPTED
        cl["points"] = ds
        stats["n_accepted"] += 1
        stats["n_points"] += nds
    stats["n_clusters"] = len(kept)
    return out


def margins_kept(result):
    """every cluster of a result keeps MARGIN_RADIUS from the ground / map radius, the frustum margins and MARGIN_KEY ->
    (bool, the first offender or None)"""
    for cl in result["clusters"]:
        m = cl["margins"]
        if m["ground"] < MARGIN_RADIUS or m["map"] < MARGIN_RADIUS or not m["frustum_ok"] or m["key"] < MARGIN_KEY:
            return False, cl
    return True, None


def packed(result):
    """the accepted clusters as the call returns them -> (centroids, voxels, sizes, offsets, points)"""
    acc = [cl for cl in result["clusters"] if cl["fate"] == ACCEPTED]
    cen = np.array([cl["centroid"] for cl in acc], dtype=f32).reshape(-1, 3)
    vox = np.array([cl["voxel"] for cl in acc], dtype=np.int32).reshape(-1, 3)
    size = np.array([cl["size"] for cl in acc], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum([len(cl["points"]) for cl in acc])]).astype(np.uint32)
    pts = np.concatenate([cl["points"] for cl in acc], axis=0).astype(f32) if acc else np.zeros((0, 3), f32)
    return cen, vox, size, off, pts
