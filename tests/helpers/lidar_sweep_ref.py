"""NumPy restatement of the front half of ImageProjection::cloudHandler, the node that produces the topic
segmented_cloud_pure the lidar perception plugins subscribe to: the yardstick of tests/test_lidar_sweep_cpu.py and
tests/test_lidar_sweep_gpu.py.

Written from the reference source (dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp, line numbers below; member
types from imageProjection.h:67-107), float32 / float64 exactly where the node's types put them; it imports nothing
from the library under test.
  parameters        :67-125     pitch removal     :297-303     projection        :328-382
  ground            :415-443, :519-526            segments          :538-540, :595-679     output    :582-592
The BFS is written as the reference writes it -- a queue, all_pushed, lineCountFlag -- and NOT as a union-find, so it is
a yardstick for the device's union-find.

UNPINNED: imageProjection.cpp needs ROS, PCL, OpenCV and boost and cannot be compiled where the tests run, so nothing
checks this file against the reference's binary.  Taken for granted:
  * unqualified sin / cos / tan / sqrt on float arguments are the float overloads (as oracle/ASSUMPTIONS.md row 18
    reads sqrt / fabs); std::asin / std::atan2 on floats are the float overloads by the standard.  The configuration's
    constants are taken with the C library's sinf / cosf / tanf, as an x86-64 build of the node would;
  * `round` of a float quotient yields the same integer whichever overload is chosen; halves round away from zero;
  * rclcpp's get_parameter stores a double parameter into a float member by a plain conversion;
  * tf2::Quaternion::setRPY(0, p, 0) = (0, sin(p / 2), 0, cos(p / 2)); tf2::transformToEigen and
    pcl::transformPointCloud(Affine3d) as tests/helpers/depth_feed_ref.py restates them;
  * PointXYZI's intensity starts at 0, so the `intensity == -1` test of groundRemoval never fires;
  * x86-64 without FMA contraction.
Differences from the reference, as the library documents them: a record with any non-finite coordinate is dropped; a
point whose row quotient is not a number (range 0) is dropped; an empty sweep yields an empty cloud.

Besides its answers stage_one reports the sweep's FRAGILE decisions, so that a test can draw its inputs by rejection from
this file alone: points whose row or column quotient lies within MARGIN rad (in angle) of a value where rowIdn or
columnIdn changes, and pixel pairs whose ground angle lies within MARGIN rad of the threshold.  MARGIN = 1e-5 is about
ten times four units in the last place of a float at pi (9.5e-7), well above the <= 1 ulp the project accepts from a
device atan2.  The range, the tang comparison and the pitch removal have no margin: they are the same IEEE operations in
any correct implementation and must agree bit for bit.
"""
import collections
import ctypes
import ctypes.util
import math

import numpy as np

import depth_feed_ref as F

f32, f64 = np.float32, np.float64
MARGIN = 1e-5
DEG_TO_RAD = math.pi / 180.0              # utility.h:51
FLT_MAX = np.finfo(np.float32).max
INVALID = 999999

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")


def _cfloat(name):
    fn = getattr(_libm, name)
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return lambda x: f32(fn(float(x)))


sinf, cosf, tanf = _cfloat("sinf"), _cfloat("cosf"), _cfloat("tanf")


class Config:
    """The fields of dddmr_lidar_sweep_config (angles in degrees, the mount angle in radians)."""

    def __init__(self, V, H, bottom, top, ground_scan_index, segment_theta=60.0, valid_point_num=5, valid_line_num=3,
                 min_range=0.3, max_range=100.0, mount=0.0):
        self.V, self.H, self.bottom, self.top, self.gsi = int(V), int(H), float(bottom), float(top), int(ground_scan_index)
        self.segment_theta, self.valid_point_num, self.valid_line_num = float(segment_theta), int(valid_point_num), int(valid_line_num)
        self.min_range, self.max_range, self.mount = float(min_range), float(max_range), float(mount)

    def planner_args(self):
        """positional and keyword arguments of LocalPlanner.set_lidar_sweep_source after the source id"""
        return (self.V, self.H, self.bottom, self.top, self.gsi), dict(
            segment_theta=self.segment_theta, segment_valid_point_num=self.valid_point_num, segment_valid_line_num=self.valid_line_num,
            minimum_detection_range=self.min_range, maximum_detection_range=self.max_range, sensor_mount_angle=self.mount)


class Derived:
    """The constructor's conversions (:67-125)."""

    def __init__(self, c):
        bottom, top = f32(c.bottom), f32(c.top)                                  # float members / float local
        self.res_x = f32((math.pi * 2) / c.H)                                    # :88
        self.res_y = f32(DEG_TO_RAD * f64(top - bottom) / f64(f32(c.V - 1)))     # :89, float(V - 1)
        self.ang_bottom = f32(-(f64(bottom) - 0.1) * DEG_TO_RAD)                 # :90
        theta = f32(c.segment_theta)
        theta = f32(f64(theta) * DEG_TO_RAD)                                     # :97
        self.tan_theta = tanf(theta)                                             # :597
        self.sin_x, self.cos_x = sinf(self.res_x), cosf(self.res_x)              # :645-646
        self.sin_y, self.cos_y = sinf(self.res_y), cosf(self.res_y)
        self.min_range, self.max_range = f32(c.min_range), f32(c.max_range)
        self.ground_limit = 10 * DEG_TO_RAD                                      # :441


def pitch_removed(raw_f32, mount):
    """:297-303"""
    T = (0.0, 0.0, 0.0, 0.0, math.sin(mount * 0.5), 0.0, math.cos(mount * 0.5))
    return F.transform(raw_f32, T)


def project(pts, c, d):
    """:331-362 for every pitch-removed point: (row, column, range, passes, row angle, column angle); angles in double for
    the fragility report."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        rng = np.sqrt((x * x + y * y) + z * z)
        vertical = np.arcsin(z / rng)
        row_angle = vertical + d.ang_bottom
        rq = row_angle / d.res_y
        ok = (rq > f32(-1.0)) & (rq < f32(c.V))                # int() truncates toward zero; NaN fails
        row = np.where(ok, np.trunc(np.where(ok, rq, 0)), -1).astype(np.int64)
        horizon = np.arctan2(x, y)
        cq = (horizon / d.res_x).astype(f64)
        rounded = np.where(cq >= 0, np.floor(cq + 0.5), -np.floor(-cq + 0.5))
        col = np.trunc(-rounded + c.H * 0.5).astype(np.int64)
        col = np.where(col >= c.H, col - c.H, col)
        ok &= (col >= 0) & (col < c.H)
        ok &= ~((rng < d.min_range) | (rng > d.max_range))
    return row, col, rng, ok, row_angle.astype(f64), horizon.astype(f64)


def label_components(row, col, c, d, range_mat, label_mat, label_count):
    """:595-679, literally; returns the next label count"""
    V, H = c.V, c.H
    line_count_flag = [False] * V
    queue = collections.deque([(row, col)])
    all_pushed = [(row, col)]
    while queue:
        fx, fy = queue.popleft()
        label_mat[fx, fy] = label_count
        for ix, iy in ((0, -1), (-1, 0), (1, 0), (0, 1)):
            tx, ty = fx + ix, fy + iy
            if tx < 0 or tx >= V:
                continue
            if ty < 0:
                ty = H - 1
            if ty >= H:
                ty = 0
            if label_mat[tx, ty] != 0:
                continue
            a, b = range_mat[fx, fy], range_mat[tx, ty]
            d1, d2 = max(a, b), min(a, b)
            sa, ca = (d.sin_x, d.cos_x) if ix == 0 else (d.sin_y, d.cos_y)
            tang = (d2 * sa) / (d1 - d2 * ca)
            if tang > d.tan_theta:
                queue.append((tx, ty))
                label_mat[tx, ty] = label_count
                line_count_flag[tx] = True
                all_pushed.append((tx, ty))
    feasible = False
    if len(all_pushed) >= 30:
        feasible = True
    elif len(all_pushed) >= c.valid_point_num:
        if sum(line_count_flag) >= c.valid_line_num:
            feasible = True
    if feasible:
        return label_count + 1
    for px, py in all_pushed:
        label_mat[px, py] = INVALID
    return label_count


def stage_one(raw_xyz, c, segments=True):
    """segments=False stops before the (slow, serial) segmentation: label then only holds 0 / -1 and cloud is empty.
    -> dict: range [V,H] float32 (FLT_MAX = empty), ground [V,H] int8, label [V,H] int32, cloud [K,4] float32
    (x y z label, raster order), full [V,H,3] float32 (_full_cloud, NaN = empty), owner [V,H] input index or -1,
    fragile_points (input indices), n_fragile."""
    d = Derived(c)
    V, H = c.V, c.H
    raw = np.asarray(raw_xyz, dtype=f32)
    raw = raw.reshape(-1, raw.shape[-1] if raw.ndim == 2 else 3)[:, :3]
    finite = np.isfinite(raw).all(axis=1)
    index = np.nonzero(finite)[0]
    pts = pitch_removed(raw[finite], c.mount)
    row, col, rng, ok, row_angle, horizon = project(pts, c, d)

    range_mat = np.full((V, H), FLT_MAX, f32)
    full = np.full((V, H, 3), np.nan, f32)
    owner = np.full((V, H), -1, np.int64)
    for i in np.nonzero(ok)[0]:                            # input order: the last one stays (:364-381)
        range_mat[row[i], col[i]] = rng[i]
        full[row[i], col[i]] = pts[i]
        owner[row[i], col[i]] = index[i]

    # fragile projections, among the points no other test has dropped for certain (a zero range drops either way)
    live = rng > 0
    res_y, res_x = f64(d.res_y), f64(d.res_x)
    with np.errstate(all="ignore"):
        k = np.clip(np.round(row_angle / res_y), -1, V)
        dist_row = np.where(k == 0, np.minimum(np.abs(row_angle - res_y), np.abs(row_angle + res_y)), np.abs(row_angle - k * res_y))
        cq = horizon / res_x
        dist_col = np.abs(cq - np.floor(cq) - 0.5) * res_x
    fragile = live & ((dist_row < MARGIN) | (dist_col < MARGIN))
    fragile_points = set(index[fragile].tolist())

    # groundRemoval's marks (:415-443): pixel pairs (i, j), (i + 1, j) for i < ground_scan_index
    ground = np.zeros((V, H), np.int8)
    if c.gsi > 0:
        lower, upper = full[: c.gsi], full[1: c.gsi + 1]
        with np.errstate(all="ignore"):
            dX, dY, dZ = (upper[..., a] - lower[..., a] for a in range(3))
            angle = np.arctan2(dZ, np.sqrt((dX * dX + dY * dY) + dZ * dZ))
            total = angle.astype(f64) + f64(c.mount)
            is_ground = total <= d.ground_limit                # NaN (an empty pixel) is not ground
            near = np.abs(total - d.ground_limit) < MARGIN
        ground[: c.gsi][is_ground] = 1
        ground[1: c.gsi + 1][is_ground] = 1
        for i, j in zip(*np.nonzero(near)):
            fragile_points.update((int(owner[i, j]), int(owner[i + 1, j])))
    label = np.zeros((V, H), np.int32)
    label[(ground == 1) | (range_mat == FLT_MAX)] = -1         # :519-526

    count = 1                                                  # cloudSegmentation (:538-540)
    with np.errstate(all="ignore"):
        for i in range(V if segments else 0):
            for j in range(H):
                if label[i, j] == 0:
                    count = label_components(i, j, c, d, range_mat, label, count)

    keep = (label > 0) & (label != INVALID)                    # :582-592, raster order
    cloud = np.concatenate([full[keep], label[keep].astype(f32)[:, None]], axis=1).astype(f32)
    return dict(range=range_mat, ground=ground, label=label, cloud=cloud, full=full, owner=owner,
                fragile_points=sorted(fragile_points), n_fragile=len(fragile_points), n_labels=count - 1)
