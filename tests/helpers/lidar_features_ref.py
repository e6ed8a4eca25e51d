"""NumPy / Python restatement of the feature half of the reference's mcl_feature_node, on top of lidar_sweep_ref.stage_one's
dictionary: the yardstick of tests/test_lidar_features_cpu.py and tests/test_lidar_features_gpu.py.

Written from the reference source, loop for loop and serially; it imports nothing from the library under test.
  segmented cloud, seg_msg   dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp:542-580
  calculateSmoothness        .../featureAssociation.cpp:318-341
  markOccludedPoints         :343-379
  extractFeatures            :381-491 (without the cloudLabel / less-flat loop and its VoxelGrid)
  adjustDistortion's axes    :281-314 (without relTime), publishCloud's transform :1384-1405
Member types from featureAssociation.h:62-63, :100-103: the thresholds and the curvatures are floats, the ranges are
floats, the literals 0.3 and 0.02 are doubles.

UNPINNED, in DESIGN 5's terms: featureAssociation.cpp needs ROS, PCL and Eigen and cannot be compiled where the tests
run, so nothing checks this file against the reference's binary.  Taken for granted, beyond lidar_sweep_ref's list:
  * std::vector::resize value-initialises, so a fresh node's cloudCurvature, cloudNeighborPicked and cloudSmoothness
    hold zeros: EVERY sweep is treated as the first sweep of a freshly constructed FeatureAssociation.  The reference
    never rewrites slot 4 of cloudSmoothness (ring 0's sp, below calculateSmoothness's range) and carries its sorted
    leftover from sweep to sweep; here slot 4 is {0.0f, ind 0} every time;
  * a float * int product and a float sum are float operations, left to right; a float compared with a double literal is
    promoted; x86-64 without FMA contraction;
  * int division truncates toward zero (it matters only for rings whose sixths are skipped anyway).
std::sort leaves the order of equal curvatures undefined.  extract() therefore runs twice, equal curvatures by ascending
and by descending index; n_tie_sensitive counts the feature lists that differ between the two runs, and a test may use a
sweep for parity only when it is 0.  The library documents ascending.
"""
import math

import numpy as np

import depth_feed_ref as F
import lidar_sweep_ref as R

f32, f64 = np.float32, np.float64
SHARP, LESS_SHARP, FLAT = 0, 1, 2
MAX_PER_RING = (12, 120, 24)          # 6 sixths x (2, 20, 4)


def segmented(ref, c):
    """imageProjection.cpp:542-580 -> dict: xyz [n,3] float32, range [n] float32, col [n] int32, row [n] int32,
    ground [n] bool, start / end [V] int32"""
    V, H = c.V, c.H
    label, ground, rng, full = ref["label"], ref["ground"], ref["range"], ref["full"]
    xyz, r, col, row, gflag = [], [], [], [], []
    start, end = np.zeros(V, np.int32), np.zeros(V, np.int32)
    size = 0
    for i in range(V):
        start[i] = size - 1 + 5
        for j in range(H):
            if label[i, j] > 0 or ground[i, j] == 1:
                if label[i, j] == R.INVALID:
                    continue
                if ground[i, j] == 1:
                    if j % 5 != 0 and j > 5 and j < H - 5:
                        continue
                gflag.append(ground[i, j] == 1)
                col.append(j)
                r.append(rng[i, j])
                xyz.append(full[i, j])
                row.append(i)
                size += 1
        end[i] = size - 1 - 5
    return dict(xyz=np.asarray(xyz, f32).reshape(-1, 3), range=np.asarray(r, f32), col=np.asarray(col, np.int32),
                row=np.asarray(row, np.int32), ground=np.asarray(gflag, bool), start=start, end=end)


def smoothness(seg):
    """:318-341 on fresh arrays: curvature [n] float32 (0 outside 5 <= i < n - 5)"""
    r = seg["range"]
    n = len(r)
    curv = np.zeros(n, f32)
    if n > 10:
        i = np.arange(5, n - 5)
        d = r[i - 5] + r[i - 4]
        d = d + r[i - 3]
        d = d + r[i - 2]
        d = d + r[i - 1]
        d = d - r[i] * f32(10)
        for k in range(1, 6):
            d = d + r[i + k]
        assert d.dtype == f32
        curv[5: n - 5] = d * d
    return curv


def occlusion(seg):
    """:343-379 on fresh arrays: cloudNeighborPicked [n] (list of 0 / 1) after markOccludedPoints"""
    r, col = seg["range"], seg["col"].tolist()
    n = len(r)
    picked = [0] * n
    if n < 12:
        return picked
    fwd = (r[:-1] - r[1:]).astype(f64).tolist()            # depth1 - depth2 at i: a float difference, promoted
    bwd = (r[1:] - r[:-1]).astype(f64).tolist()            # depth2 - depth1
    absd = np.abs(r[1:] - r[:-1]).astype(f64).tolist()     # |range[i + 1] - range[i]| = |range[i] - range[i + 1]|
    lim = (0.02 * r.astype(f64)).tolist()
    for i in range(5, n - 6):
        if abs(col[i + 1] - col[i]) < 10:
            if fwd[i] > 0.3:
                for k in range(i - 5, i + 1):
                    picked[k] = 1
            elif bwd[i] > 0.3:
                for k in range(i + 1, i + 7):
                    picked[k] = 1
        if absd[i - 1] > lim[i] and absd[i] > lim[i]:
            picked[i] = 1
    return picked


def _cdiv(a, b):
    """C's integer division"""
    q = abs(a) // b
    return q if a >= 0 else -q


def extract(seg, curv, picked0, edge_threshold, surf_threshold, V, descending_ties=False):
    """:381-491 -> ([sharp, less_sharp, flat] lists of segment indices in push order, stats)"""
    edge, surf = f32(edge_threshold), f32(surf_threshold)                  # float members
    n = len(curv)
    col, ground = seg["col"].tolist(), seg["ground"].tolist()
    curvature = [float(v) for v in curv]
    picked = list(picked0)
    sm = [(curvature[i], i) if 5 <= i < n - 5 else (0.0, 0) for i in range(max(n, 5))]      # cloudSmoothness, fresh
    out = [[], [], []]
    st = dict(edge_breaks=0, flat_breaks=0, ep_picks=0, slot4_pick=False)
    edge, surf = float(edge), float(surf)

    def suppress(ind):
        picked[ind] = 1
        for l in range(1, 6):
            if abs(col[ind + l] - col[ind + l - 1]) > 10:
                break
            picked[ind + l] = 1
        for l in range(-1, -6, -1):
            if ind + l < 0:
                continue
            if abs(col[ind + l] - col[ind + l + 1]) > 10:
                break
            picked[ind + l] = 1

    for i in range(V):
        s, e = int(seg["start"][i]), int(seg["end"][i])
        for j in range(6):
            sp = _cdiv(s * (6 - j) + e * j, 6)
            ep = _cdiv(s * (5 - j) + e * (j + 1), 6) - 1
            if sp >= ep:
                continue
            sm[sp:ep] = sorted(sm[sp:ep], key=(lambda t: (t[0], -t[1])) if descending_ties else (lambda t: (t[0], t[1])))
            largest = 0
            for k in range(ep, sp - 1, -1):
                ind = sm[k][1]
                if picked[ind] == 0 and curvature[ind] > edge and not ground[ind]:
                    largest += 1
                    if largest <= 2:
                        out[SHARP].append(ind)
                        out[LESS_SHARP].append(ind)
                    elif largest <= 20:
                        out[LESS_SHARP].append(ind)
                    else:
                        st["edge_breaks"] += 1
                        break
                    st["ep_picks"] += k == ep
                    suppress(ind)
            smallest = 0
            for k in range(sp, ep + 1):
                ind = sm[k][1]
                if picked[ind] == 0 and curvature[ind] < surf and ground[ind]:
                    out[FLAT].append(ind)
                    st["ep_picks"] += k == ep
                    if k == 4 and ind == 0:
                        st["slot4_pick"] = True
                    smallest += 1
                    if smallest >= 4:
                        st["flat_breaks"] += 1
                        break
                    suppress(ind)
    return out, st


def features(ref, c, edge_threshold, surf_threshold):
    """Everything of one sweep: the segmented cloud, the three lists (equal curvatures by ascending index) and the report."""
    seg = segmented(ref, c)
    curv = smoothness(seg)
    picked = occlusion(seg)
    lists, st = extract(seg, curv, picked, edge_threshold, surf_threshold, c.V)
    other, _ = extract(seg, curv, picked, edge_threshold, surf_threshold, c.V, descending_ties=True)
    st["n_tie_sensitive"] = sum(a != b for a, b in zip(lists, other))
    st["n_occluded"] = int(sum(picked))
    return dict(seg=seg, curvature=curv, occluded=np.asarray(picked, np.int8), lists=[np.asarray(l, np.int64) for l in lists], **st)


def identity_T():
    return np.hstack([np.eye(3), np.zeros((3, 1))])


def node_T():
    """publishCloud's trans_c2s.inverse() for the node's q.setRPY(0, -1.570795, -1.570795), zero translation, as a caller
    computes it: [3, 4] float64"""
    roll, pitch, yaw = 0.0, -1.570795, -1.570795
    cy, sy, cp, sp, cr, sr = (fn(a / 2) for a in (yaw, pitch, roll) for fn in (math.cos, math.sin))
    q = (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)
    M = np.eye(4)
    M[:3, :3] = F.rotation((0.0, 0.0, 0.0) + q)
    return np.linalg.inv(M)[:3, :]


def output(seg, idx, T_out):
    """:281-314 without relTime, then pcl::transformPointCloud(Affine3d) (:1393): [K, 4] float32 x y z ring"""
    T = np.asarray(T_out, f64).reshape(3, 4)
    p = seg["xyz"][idx].reshape(-1, 3)
    cam = np.stack([p[:, 1], p[:, 2], p[:, 0]], axis=1).astype(f64)
    out = np.empty((len(p), 4), f32)
    for a in range(3):
        out[:, a] = (((T[a, 0] * cam[:, 0] + T[a, 1] * cam[:, 1]) + T[a, 2] * cam[:, 2]) + T[a, 3]).astype(f32)
    out[:, 3] = seg["row"][idx].astype(f32)               # float(int(row + col / 10000.0))
    return out
