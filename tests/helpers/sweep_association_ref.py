"""NumPy restatement of the rest of the front half of LeGO-LOAM's feature node, on top of lidar_sweep_ref.stage_one's and
lidar_features_ref.features' dictionaries: the yardstick of tests/test_sweep_association_cpu.py and
tests/test_sweep_association_gpu.py.  It imports nothing from the library under test.
  findStartEndAngle          dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp:391-406
  adjustDistortion's relTime .../featureAssociation.cpp:281-314
  the cloudLabel loop        :486-490, downSizeFilter (leaf 0.2, :124) :510-514
  outlier_cloud              imageProjection.cpp:548-558, the intensity of :376
float32 where the reference is float (the three orientations are float32 message fields, `ori`, relTime), float64 where
it is double (M_PI, _scan_period); atan2f is the C library's own, called through ctypes.

The serial halfPassed flag is restated WITHOUT the serial walk, as the library does it: the first-branch value of every
point, i0 = the first index whose first-branch value flips the flag, the second branch for the points behind i0.
tests/test_sweep_association_cpu.py holds this against a plain transcription of the reference's loops.

UNPINNED, like the two files it builds on.  Taken for granted beyond their lists:
  * `-atan2(point.x, point.z)` on float arguments is the float overload;
  * cloudLabel of a fresh node is zero (every sweep is the first sweep of a fresh FeatureAssociation);
  * pcl::VoxelGrid as oracle/ASSUMPTIONS.md rows 7 and 8 have it, and -- assumed HERE -- downsample_all_data averages the
    intensity like a coordinate: a float running sum in input order divided by the count;
  * VoxelGrid's leaf-size check: d = int64((max - min) * inverse_leaf) + 1 per axis with a float product, and
    dx * dy * dz > INT32_MAX hands the input through unchanged.
Besides its answers it reports min_margin: how close (rad) any decision that an atan2f feeds comes to its threshold, so a
test can draw its inputs by rejection from this file alone (MARGIN, lidar_sweep_ref's).
"""
import ctypes
import ctypes.util
import math

import numpy as np

import lidar_features_ref as FR
import lidar_sweep_ref as R

f32, f64 = np.float32, np.float64
MARGIN = R.MARGIN
PI = math.pi
LEAF = f32(0.2)
INT32_MAX = 2 ** 31 - 1
SHARP, LESS_SHARP, FLAT, LESS_FLAT = 0, 1, 2, 3

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


def atan2f(y, x):
    """the C library's atan2f, element by element -> float32 array"""
    y, x = np.asarray(y, f32).reshape(-1), np.asarray(x, f32).reshape(-1)
    return np.array([_libm.atan2f(float(a), float(b)) for a, b in zip(y, x)], f32)


def orientation(raw, c):
    """:391-406 on the first and last FINITE record of the pitch-removed cloud -> (start, end, diff as float32, margin)"""
    raw = np.asarray(raw, f32).reshape(-1, 3)
    raw = raw[np.isfinite(raw).all(axis=1)]
    if len(raw) == 0:
        return f32(0), f32(0), f32(0), math.inf
    p = R.pitch_removed(raw[[0, -1]], c.mount)
    a = atan2f(p[:, 1], p[:, 0])
    start = f32(-a[0])
    end = f32(f64(f32(-a[1])) + 2 * PI)
    d = f64(f32(end - start))
    margin = min(abs(d - 3 * PI), abs(d - PI))
    if d > 3 * PI:
        end = f32(f64(end) - 2 * PI)
    elif d < PI:
        end = f32(f64(end) + 2 * PI)
    return start, end, f32(end - start), margin


def point_times(seg, start, end, diff, scan_period):
    """:292-311 for every segmented point -> (intensity [n] float32, relTime [n] float32, i0, margin)"""
    n = len(seg["range"])
    if n == 0:
        return np.zeros(0, f32), np.zeros(0, f32), 0, math.inf
    base = -atan2f(seg["xyz"][:, 1], seg["xyz"][:, 0])               # ori = -atan2(point.x, point.z) = -atan2(seg.y, seg.x)
    b64, s64, e64 = base.astype(f64), f64(start), f64(end)
    lo, hi = b64 < s64 - PI / 2, b64 > s64 + PI * 3 / 2
    first = np.where(lo, (b64 + 2 * PI).astype(f32), np.where(hi, (b64 - 2 * PI).astype(f32), base)).astype(f32)
    d1 = (first - start).astype(f32).astype(f64)
    flips = np.nonzero(d1 > PI)[0]
    i0 = int(flips[0]) if len(flips) else n
    second = (b64 + 2 * PI).astype(f32)
    c64 = second.astype(f64)
    lo2, hi2 = c64 < e64 - PI * 3 / 2, c64 > e64 + PI / 2
    second = np.where(lo2, (c64 + 2 * PI).astype(f32), np.where(hi2, (c64 - 2 * PI).astype(f32), second)).astype(f32)
    idx = np.arange(n)
    ori = np.where(idx <= i0, first, second).astype(f32)
    with np.errstate(all="ignore"):
        rel = ((ori - start).astype(f32) / diff).astype(f32)
    inten = (seg["row"].astype(f64) + f64(scan_period) * rel.astype(f64)).astype(f32)
    m1 = np.minimum(np.minimum(np.abs(b64 - (s64 - PI / 2)), np.abs(b64 - (s64 + PI * 3 / 2))), np.abs(d1 - PI))
    m2 = np.minimum(np.abs(c64 - (e64 - PI * 3 / 2)), np.abs(c64 - (e64 + PI / 2)))
    margin = float(np.where(idx <= i0, m1, m2).min())
    return inten, rel, i0, margin


def voxel_grid(pts, leaf=LEAF):
    """pcl::VoxelGrid with downsample_all_data on [n, 4] float32 x y z intensity -> (centroids [m, 4] in voxel-index order,
    the input indices of each voxel in the order they were summed [m lists], overflow: the input was handed through)"""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    n = len(pts)
    if n == 0:
        return np.zeros((0, 4), f32), [], False
    inv = f32(1.0) / f32(leaf)
    mn, mx = pts[:, :3].min(axis=0), pts[:, :3].max(axis=0)
    prod, over = 1, False
    for a in range(3):
        ext = f32(f32(mx[a] - mn[a]) * inv)
        prod *= int(ext) + 1                                         # (Python integers: no overflow of their own)
    if prod > INT32_MAX:
        return pts.copy(), [[i] for i in range(n)], True
    ijk = np.floor(pts[:, :3] * inv).astype(np.int64)
    lo = np.floor(mn * inv).astype(np.int64)
    hi = np.floor(mx * inv).astype(np.int64)
    dx, dy = int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)
    key = [int(v[0] - lo[0]) + int(v[1] - lo[1]) * dx + int(v[2] - lo[2]) * dx * dy for v in ijk]
    order = sorted(range(n), key=lambda i: (key[i], i))
    out, members = [], []
    i = 0
    while i < n:
        j = i
        s = np.zeros(4, f32)
        while j < n and key[order[j]] == key[order[i]]:
            s = (s + pts[order[j]]).astype(f32)                      # float running sums, input order
            j += 1
        out.append(s / f32(j - i))
        members.append(order[i:j])
        i = j
    return np.array(out, f32).reshape(-1, 4), members, over


def candidates(f, V):
    """:486-490 per ring: the segment indices of the less-flat candidates, ascending, and how many sixths were skipped"""
    seg = f["seg"]
    label = np.zeros(max(len(seg["range"]), 1), np.int8)
    label[f["lists"][FR.FLAT]] = -1
    label[f["lists"][FR.LESS_SHARP]] = 1
    label[f["lists"][FR.SHARP]] = 2
    rings, skipped = [], []
    for i in range(V):
        s, e = int(seg["start"][i]), int(seg["end"][i])
        ks, skip = [], 0
        for j in range(6):
            sp = FR._cdiv(s * (6 - j) + e * j, 6)
            ep = FR._cdiv(s * (5 - j) + e * (j + 1), 6) - 1
            if sp >= ep:
                skip += 1
                continue
            ks += [k for k in range(sp, ep + 1) if label[k] <= 0]
        rings.append(np.asarray(ks, np.int64))
        skipped.append(skip)
    return rings, skipped


def association_frame(seg, idx, inten):
    """:288-290: (y, z, x) of the segmented point and its intensity -> [K, 4] float32"""
    p = seg["xyz"][idx].reshape(-1, 3)
    return np.stack([p[:, 1], p[:, 2], p[:, 0], inten[idx]], axis=1).astype(f32)


def through(T_out, cloud):
    """pcl::transformPointCloud(Affine3d) on an association-frame cloud: the intensity is carried through"""
    T = np.asarray(T_out, f64).reshape(3, 4)
    p = cloud[:, :3].astype(f64)
    out = cloud.copy()
    for a in range(3):
        out[:, a] = (((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3]).astype(f32)
    return out


def outliers(ref, c):
    """imageProjection.cpp:548-558 -> [K, 4] float32, raster order"""
    out = []
    for i in range(c.V):
        for j in range(c.H):
            if ref["label"][i, j] == R.INVALID and i > c.gsi and j % 5 == 0:
                out.append(list(ref["full"][i, j]) + [f32(f64(f32(i)) + f64(f32(j)) / 10000.0)])
    return np.asarray(out, f32).reshape(-1, 4)


def association(raw, c, ref, f, scan_period, T_out=None):
    """Everything of one sweep: dict of start / end / diff, i0, times [n], clouds[frame][which] = ([K, 4], seg index [K]),
    outliers [K, 4], rel [n] (relTime), voxel_members (per less-flat point the segment indices summed into it, in order),
    and the report: min_margin, ring_candidates, ring_voxels, ring_skipped, ring_overflow,
    n_scattered (voxels fed by candidates that are not consecutive), n_single (one-point voxels)"""
    T = FR.identity_T() if T_out is None else T_out
    seg = f["seg"]
    start, end, diff, m0 = orientation(raw, c)
    inten, rel, i0, m1 = point_times(seg, start, end, diff, scan_period)
    rings, skipped = candidates(f, c.V)
    lf, lf_idx, n_vox, over, n_scattered, n_single, voxel_members = [], [], [], [], 0, 0, []
    for ks in rings:
        pts = association_frame(seg, ks, inten)
        cen, members, ov = voxel_grid(pts)
        lf.append(cen)
        lf_idx.append(np.asarray([ks[m[0]] for m in members], np.int64))
        voxel_members += [ks[m] for m in members]
        n_vox.append(len(cen))
        over.append(ov)
        if len(ks) and not ov:
            inv = f32(1.0) / LEAF
            ijk = [tuple(v) for v in np.floor(pts[:, :3] * inv).astype(np.int64)]
            members = {}
            for r, v in enumerate(ijk):
                members.setdefault(v, []).append(r)
            n_scattered += sum(1 for m in members.values() if m[-1] - m[0] + 1 != len(m))
            n_single += sum(1 for m in members.values() if len(m) == 1)
    frame0 = [association_frame(seg, f["lists"][w], inten) for w in range(3)] + [np.concatenate(lf).reshape(-1, 4) if lf else np.zeros((0, 4), f32)]
    idx = [np.asarray(f["lists"][w], np.int64) for w in range(3)] + [np.concatenate(lf_idx) if lf_idx else np.zeros(0, np.int64)]
    frame1 = [through(T, cl) for cl in frame0]
    return dict(start=start, end=end, diff=diff, i0=i0, times=inten, clouds=[list(zip(frame0, idx)), list(zip(frame1, idx))],
                outliers=outliers(ref, c), rel=rel, voxel_members=voxel_members, min_margin=min(m0, m1), ring_candidates=[len(k) for k in rings], ring_voxels=n_vox,
                ring_skipped=skipped, ring_overflow=over, n_scattered=n_scattered, n_single=n_single)
