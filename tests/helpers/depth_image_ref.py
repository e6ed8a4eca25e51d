"""NumPy restatement of the reference's depth image node, the yardstick of the depth image tests.

It restates DepthImg2PointCloud::cbDepthImg (dddmr_perception_3d/utils/depthimg2pointcloud_node.cpp:96-157) with
float32 / float64 casts where the node's types put them, and hands its cloud to depth_feed_ref (bufferCloud) for stage
two.  It imports nothing from the library under test.

Taken for granted (listed in DESIGN.md): cv_bridge::toCvCopy of a 16UC1 image is the image itself, row padding
removed; `at<unsigned short>(v, u) * 0.001` is int -> double, a double product, rounded to float; `1.0f / K[0]` is a
double division rounded to float; `(u - cx)` converts the unsigned u to float; the x86-64 build contracts nothing;
pcl::VoxelGrid<PointXYZ>::setLeafSize(double...) stores floats, inverse_leaf_size = 1.0f / leaf; its index-overflow
bail-out is not restated (depth_feed_ref.voxel_centroids asserts the box stays under 2e9 cells).
"""
import numpy as np

import depth_feed_ref as R

f32, f64 = np.float32, np.float64


def intrinsics(K4):
    """K4 = (fx, fy, cx, cy) = CameraInfo K[0], K[4], K[2], K[5] -> the node's four floats (cx, cy, 1/fx, 1/fy), :111-114"""
    fx, fy, cx, cy = (f64(v) for v in K4)
    return f32(cx), f32(cy), f32(f64(1.0) / fx), f32(f64(1.0) / fy)


def image_rows(buf, width, height, row_stride_bytes):
    """The [height, width] uint16 view of a byte buffer whose rows are row_stride_bytes apart"""
    raw = np.frombuffer(buf, dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(raw.view(np.uint16), shape=(height, width), strides=(row_stride_bytes, 2))


def deproject(img, K4, max_distance=4.0, sample_step=2, drop_zero=False):
    """:127-148 -> [N,3] float32 in the optical frame, in the node's push_back order (rows outer, columns inner).
    A pixel of depth 0 is kept unless drop_zero (the library's flag, not the reference's behaviour)."""
    img = np.asarray(img)
    assert img.dtype == np.uint16 and img.ndim == 2
    cx, cy, fx, fy = intrinsics(K4)
    step = int(sample_step)
    d = img[::step, ::step]
    v, u = np.meshgrid(np.arange(0, img.shape[0], step, dtype=np.uint32), np.arange(0, img.shape[1], step, dtype=np.uint32),
                       indexing="ij")
    z = (d.astype(f64) * f64(0.001)).astype(f32)                # float z = at<unsigned short>(v, u) * 0.001;
    keep = ~(z.astype(f64) > f64(max_distance))                 # if (isnan(z) || z > max_distance_) continue;
    if drop_zero:
        keep &= d != 0
    x = ((u.astype(f32) - cx) * z) * fx                         # pt.x = (u - cx) * z * fx;  float, left to right
    y = ((v.astype(f32) - cy) * z) * fy
    assert x.dtype == f32 and y.dtype == f32
    return np.stack([x[keep], y[keep], z[keep]], axis=1)


def stage_one(img, K4, max_distance=4.0, leaf_size=0.05, sample_step=2, drop_zero=False):
    """What the node publishes: VoxelGrid(leaf) centroids of the deprojected pixels, float sums in input order"""
    return R.voxel_centroids(deproject(img, K4, max_distance, sample_step, drop_zero), leaf_size)[0]


def stage_one_tolerance(img, K4, max_distance=4.0, leaf_size=0.05, sample_step=2, drop_zero=False):
    """PCL sums a voxel's points in float in an order it does not specify.  -> (centroids summed in input order,
    tolerance = max(1e-5, 2 x the largest distance to the centroids summed in reversed order), that largest distance).
    A double sum lies between what float orders produce; 2 x allows for it lying on neither side."""
    pts = deproject(img, K4, max_distance, sample_step, drop_zero)
    fwd = R.voxel_centroids(pts, leaf_size)[0]
    rev = R.voxel_centroids(pts[::-1], leaf_size)[0]            # same voxels, same (linear index) order
    assert fwd.shape == rev.shape
    spread = float(np.linalg.norm(fwd.astype(f64) - rev.astype(f64), axis=1).max()) if len(fwd) else 0.0
    return fwd, max(1e-5, 2.0 * spread), spread


def observation(img, K4, T_base_optical, T_gbl_base, zmin, zmax, **node):
    """image -> the frame's observation in the global frame: stage one, then bufferCloud"""
    return R._frame(stage_one(img, K4, **node), T_base_optical, T_gbl_base, zmin, zmax)[0]


def decided_band(img, K4, T_base_optical, node, nominal=(0.0, 2.0), window=0.02):
    """Height limits at which the reference itself is decided for this image: each nominal limit moves to the middle
    of the widest gap between consecutive base-frame z values of the reference's stage-one centroids within `window`
    of it.  -> ((zmin, zmax), (gap at zmin, gap at zmax))"""
    z = np.sort(R.transform(stage_one(img, K4, **node), T_base_optical)[:, 2].astype(f64))
    limits, gaps = [], []
    for nom in nominal:
        edges = np.concatenate([[nom - window], z[(z > nom - window) & (z < nom + window)], [nom + window]])
        k = int(np.argmax(np.diff(edges)))
        limits.append(float(0.5 * (edges[k] + edges[k + 1])))
        gaps.append(float(edges[k + 1] - edges[k]))
    return tuple(limits), tuple(gaps)
