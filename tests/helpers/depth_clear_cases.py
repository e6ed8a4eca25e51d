"""The inputs tests/test_depth_frustum_cpu.py and tests/test_depth_clear_gpu.py share: camera rigs, rendered frames and
the drawing of markings by rejection from the restatement (depth_frustum_ref) alone.  CPU only."""
import numpy as np

from dddmr_navigation_amd import scenes

import depth_feed_ref as F
import depth_frustum_ref as R

FOV_W, FOV_V, D_MIN, D_MAX = 1.5184, 1.0123, 0.3, 5.0      # multi_depth_camera_3d_ros.yaml
Z_MIN, Z_MAX = 0.1, 2.0
RES = HRES = 0.05
SHIFT_FAR = np.array([1500.0, -800.0, 30.0])               # kilometres from the map origin
T_BASE_CAM = ((0.25, 0.12, 0.35) + tuple(scenes.quat_from_rpy(0.0, 0.05, 0.6)),
              (0.25, -0.12, 0.35) + tuple(scenes.quat_from_rpy(0.0, 0.05, -0.6)))
T_BASE_CAM_ROLLED = ((0.2, 0.1, 0.4) + tuple(scenes.quat_from_rpy(0.3, -0.2, 0.5)),
                     (0.2, -0.1, 0.4) + tuple(scenes.quat_from_rpy(-0.25, 0.15, -0.7)))


def shifted_cloud(shift):
    c = scenes.cloud_c2().copy()
    c[:, :3] = (c[:, :3].astype(np.float64) + np.asarray(shift)).astype(np.float32)
    return c


def base_pose(shift, yaw=0.05, dx=0.0):
    return (float(shift[0]) + dx, float(shift[1]), float(shift[2])) + tuple(scenes.quat_from_rpy(0.0, 0.0, yaw))


def render(cloud, t_gb, t_bc, seed, width=160, height=120):
    return scenes.depth_frame(cloud, F.compose(t_gb, t_bc), width, height, FOV_W, FOV_V, D_MAX, seed=seed)


def frustum(t_gb, t_bc):
    """the restatement's frustum and the m2s it was built from"""
    m2s = F.compose(t_gb, t_bc)
    return R.Frustum(FOV_W, FOV_V, D_MIN, D_MAX, m2s), m2s


def subset(voxels, offsets, cluster, keep):
    """the markings with keep[i], repacked"""
    offsets = np.asarray(offsets, dtype=np.int64)
    size = offsets[1:] - offsets[:-1]
    rows = np.repeat(keep, size)
    off = np.concatenate([[0], np.cumsum(size[keep])]).astype(np.uint32)
    return voxels[keep], off, cluster[rows]


def draw(frustums, obs, centre, n, seed, anchors=None):
    """n markings drawn from the seed, those whose comparisons keep their margins in the restatement kept ->
    (voxels, offsets, cluster, verdict, engaged, share of the draws discarded)"""
    vox, off, cl = scenes.depth_clear_markings(obs, centre, n, seed, RES, HRES, anchors=anchors)
    _, _, ok = R.clear_verdicts(frustums, obs, RES, HRES, vox, off, cl)
    vox, off, cl = subset(vox, off, cl, ok)
    verdict, engaged, ok2 = R.clear_verdicts(frustums, obs, RES, HRES, vox, off, cl)
    assert ok2.all()
    return vox, off, cl, verdict, engaged, 1.0 - float(ok.mean())


def anchors_of(t_gb, cams, seed=40):
    return np.concatenate([scenes.frustum_side_points(F.compose(t_gb, t_bc), FOV_W, FOV_V, D_MIN, D_MAX, 64, seed + i)
                           for i, t_bc in enumerate(cams)], axis=0)


def draw_points(frustums, centre, n, seed, anchors):
    """n test points for the two point tests, around the rig and along its frustum planes, margins kept ->
    (points [K,3] float32, in_frustums, attach, share discarded)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    centre = np.asarray(centre, dtype=np.float64)
    wide = centre + rng.uniform([-7.0, -7.0, -1.0], [7.0, 7.0, 3.0], (n - n // 3, 3))
    near = anchors[rng.integers(0, len(anchors), n // 3)] + rng.normal(0.0, 0.08, (n // 3, 3))
    pts = np.concatenate([wide, near], axis=0).astype(np.float32)
    inside, attach, ok = R.point_tests(frustums, pts)
    return pts[ok], inside[ok], attach[ok], 1.0 - float(ok.mean())


def leaves(verdict):
    """which of the six leaves of the tree (branch 1..3 x kept) a set of verdicts reaches"""
    return set(int(v) for v in np.unique(verdict))
