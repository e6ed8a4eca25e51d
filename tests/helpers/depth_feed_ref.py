"""NumPy restatement of the depth camera layer's local-mode path, the yardstick of the depth feed tests.

It restates, step by step, DepthCameraObservationBuffer::bufferCloud and purgeStaleObservations
(dddmr_perception_3d/plugins/depth_camera/depth_camera_observation_buffer.cpp:78-187, :203-231) and
DepthCameraLayer::getObservation (depth_camera_layer.cpp:618-663), with float32 / float64 casts where the
reference's types put them.  It imports nothing from the library under test.

Taken for granted (listed in DESIGN.md): pcl_conversions::toPCL = ns // 1000; VoxelGrid with
downsample_all_data and min_points_per_voxel 0; VoxelGrid's index-overflow bail-out is not restated
(voxel_centroids asserts the box stays under 2e9 cells); a record with any non-finite coordinate is
dropped, as the library documents (the reference drops NaN z only).
"""
import numpy as np

VOXELIZE_ABOVE = 20000      # depth_camera_observation_buffer.cpp:124: `if (cloud_size_after_min_max_obstacle > 20000)`
LEAF = 0.05                 # :128 sor.setLeafSize(0.05, 0.05, 0.05)


def rotation(T):
    """Eigen::Quaterniond(w, x, y, z).toRotationMatrix() as tf2::transformToEigen builds it; T = x y z qx qy qz qw."""
    x, y, z, w = (np.float64(v) for v in T[3:7])
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], dtype=np.float64)


def transform(pts_f32, T):
    """pcl::transformPointCloud(cloud, cloud, Affine3d) (:105-107, :177-178): float coordinates promoted to double,
    row times vector summed left to right, plus the translation, rounded to float."""
    p = np.asarray(pts_f32, dtype=np.float32).astype(np.float64)
    R = rotation(T)
    t = np.asarray(T[:3], dtype=np.float64)
    out = np.empty((len(p), 3), dtype=np.float32)
    for a in range(3):
        out[:, a] = (((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a]).astype(np.float32)
    return out


def height_band(base_f32, zmin, zmax):
    """:109-120: `(*it).z <= max_obstacle_height_ && (*it).z >= min_obstacle_height_`: float z against the double
    limits, both ends kept, NaN fails."""
    z = base_f32[:, 2].astype(np.float64)
    return base_f32[(z <= np.float64(zmax)) & (z >= np.float64(zmin))]


def voxel_keys(pts_f32, leaf=LEAF):
    """pcl::VoxelGrid::applyFilter: ijk = floor(p * inverse_leaf_size) per axis in float, inverse_leaf_size =
    1.0f / leaf (20.0f for 0.05f, 10.0f for 0.1f)."""
    inv = np.float32(1.0) / np.float32(leaf)
    return np.floor(np.asarray(pts_f32, dtype=np.float32) * inv).astype(np.int64)


def voxel_centroids(pts_f32, leaf=LEAF):
    """pcl::VoxelGrid centroids (downsample_all_data, min_points_per_voxel 0): voxels in the order of PCL's linear
    index (x fastest), float sums in input order, divided by the float count.  Returns (centroids [K,3] float32,
    member [N] = the output row every input point went to)."""
    pts = np.asarray(pts_f32, dtype=np.float32)
    if len(pts) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int64)
    ijk = voxel_keys(pts, leaf)
    lo, hi = ijk.min(axis=0), ijk.max(axis=0)
    dims = hi - lo + 1
    assert int(dims[0]) * int(dims[1]) * int(dims[2]) < 2_000_000_000, "VoxelGrid would bail out: box too large for the leaf"
    lin = (ijk[:, 0] - lo[0]) + (ijk[:, 1] - lo[1]) * dims[0] + (ijk[:, 2] - lo[2]) * dims[0] * dims[1]
    uniq, member = np.unique(lin, return_inverse=True)
    member = member.reshape(-1)
    sums = np.zeros((len(uniq), 3), dtype=np.float32)
    np.add.at(sums, member, pts)                      # unbuffered: one float add per point, in input order
    counts = np.bincount(member, minlength=len(uniq)).astype(np.float32)
    return (sums / counts[:, None]).astype(np.float32), member


def frame_observation(raw_xyz, T_base_sensor, T_gbl_base, zmin, zmax):
    """bufferCloud's steps for one frame -> the observation in the global frame, [K,3] float32."""
    raw = np.asarray(raw_xyz, dtype=np.float32)[:, :3]
    raw = raw[np.isfinite(raw).all(axis=1)]
    return _frame(raw, T_base_sensor, T_gbl_base, zmin, zmax)[0]


def _frame(raw, T_base_sensor, T_gbl_base, zmin, zmax):
    """-> (observation, whether it went through the VoxelGrid)"""
    band = height_band(transform(raw, T_base_sensor), zmin, zmax)
    voxelised = len(band) > VOXELIZE_ABOVE
    if voxelised:
        band, _ = voxel_centroids(band, LEAF)
    return transform(band, T_gbl_base), voxelised


def n_survivors(raw_xyz, T_base_sensor, zmin, zmax):
    raw = np.asarray(raw_xyz, dtype=np.float32)[:, :3]
    raw = raw[np.isfinite(raw).all(axis=1)]
    return len(height_band(transform(raw, T_base_sensor), zmin, zmax))


def purge(stamps_us, last_updated_ns, persistence_ns):
    """purgeStaleObservations (:203-231) on the observations' stamps (whole microseconds, oldest first): the indices
    that stay.  persistence 0 keeps the newest only; otherwise one leaves when
    last_updated - stamp > persistence, strictly, in integer nanoseconds."""
    if not len(stamps_us):
        return []
    if int(persistence_ns) == 0:
        return [len(stamps_us) - 1]
    return [i for i, us in enumerate(stamps_us) if not (int(last_updated_ns) - int(us) * 1000 > int(persistence_ns))]


class DepthBufferRef:
    """One observation buffer (one camera topic): bufferCloud per frame, getObservations = alive frames oldest first."""

    def __init__(self, zmin, zmax, persistence_ns):
        self.zmin, self.zmax, self.persistence_ns = float(zmin), float(zmax), int(persistence_ns)
        self.frames = []          # (stamp_us, [K,3] float32 global, went through the VoxelGrid)

    def buffer_cloud(self, raw_xyz, T_base_sensor, T_gbl_base, stamp_ns):
        raw = np.asarray(raw_xyz, dtype=np.float32)[:, :3]
        obs, voxelised = _frame(raw[np.isfinite(raw).all(axis=1)], T_base_sensor, T_gbl_base, self.zmin, self.zmax)
        self.frames.append((int(stamp_ns) // 1000, obs, voxelised))                     # pcl_conversions::toPCL(clock_->now(), ...)
        keep = purge([f[0] for f in self.frames], int(stamp_ns), self.persistence_ns)   # last_updated_ = now
        self.frames = [self.frames[i] for i in keep]
        return obs

    def observation(self):
        if not self.frames:
            return np.zeros((0, 3), np.float32)
        return np.concatenate([f[1] for f in self.frames], axis=0)

    def frame_sizes(self):
        return [len(f[1]) for f in self.frames]


def compose(Ta, Tb):
    """Pose product Ta * Tb (x y z qx qy qz qw each), for placing a camera: global<-sensor = global<-base * base<-sensor.
    Used to render test frames only, never on the compared path."""
    ax, ay, az, aw = (float(v) for v in Ta[3:7])
    bx, by, bz, bw = (float(v) for v in Tb[3:7])
    q = (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
         aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)
    t = rotation(Ta) @ np.asarray(Tb[:3], dtype=np.float64) + np.asarray(Ta[:3], dtype=np.float64)
    return (float(t[0]), float(t[1]), float(t[2])) + q
