"""The cases tests/test_depth_mark_cpu.py and tests/test_depth_mark_gpu.py share, built on the depth-clear rigs
(depth_clear_cases): what is fed to which source, the ground and map clouds, the layer's parameters.  CPU only.

A case is a list of feed steps (frames, images, a lidar scan) that the CPU test runs through the feed's restatement
(depth_feed_ref / depth_image_ref) and the GPU test through the library.  The ground cloud is a plane of nodes under the
scene with nodes raised to some clusters' centroids, the map cloud covers the part of the scene ahead of the robot and
some clusters' centroids; both are placed from a first pass of the restatement over the restated observation.  The
committed seeds are such that in the restatement alone every cluster of every case keeps the margins of
depth_mark_ref.margins_kept (tests/test_depth_mark_cpu.py asserts it; find_seed searched them)."""
import numpy as np

from dddmr_navigation_amd import scenes

import depth_clear_cases as dc
import depth_feed_ref as F
import depth_frustum_ref as R
import depth_image_ref as I
import depth_mark_ref as M

MS = 1_000_000
TBS_LIDAR = (0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0)


class Case:
    def __init__(self, name, seed, cams=2, far=False, kind="frame", poses=((0.05, 0.0),), persistence_ns=0, max_frames=1,
                 lidar=False, res=0.05, hres=0.05, tol=0.1, min_size=1, ratio=0.5, with_map=True, width=160, height=120,
                 few=None):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    @property
    def shift(self):
        return dc.SHIFT_FAR if self.far else np.zeros(3)

    @property
    def rig(self):
        return (dc.T_BASE_CAM_ROLLED if self.far else dc.T_BASE_CAM)[: self.cams]

    @property
    def first_source(self):
        return 1 if self.lidar else 0

    @property
    def t_gb(self):
        yaw, dx = self.poses[-1]
        return dc.base_pose(self.shift, yaw=yaw, dx=dx)


CASES = [
    Case("one_camera", seed=200, cams=1, ratio=0.5),
    Case("two_cameras", seed=211, ratio=0.0),
    Case("image_sources", seed=221, kind="image", width=320, height=240, ratio=1.0),
    Case("three_alive_frames", seed=230, cams=1, poses=((0.05, 0.0), (0.45, 0.5), (0.85, 1.0)), persistence_ns=200 * MS, max_frames=4),
    Case("lidar_beside", seed=241, lidar=True),
    Case("far_rolled", seed=251, far=True, res=0.3, min_size=5),
    Case("min_size_5", seed=260, min_size=5),
    Case("no_map", seed=270, with_map=False),
    Case("few_points", seed=280, cams=1, few=5),
    Case("contested_voxels", seed=291, res=0.3, tol=0.05, min_size=4),
    Case("above_20000", seed=300, cams=1, width=320, height=240),
]
BY_NAME = {c.name: c for c in CASES}


def steps(case):
    """the feed steps in order: dicts of sid, kind, data, T_base_sensor (what the feed call takes), T_gbl_base, stamp,
    m2s (the frustum's transform), and for images K4"""
    cloud = dc.shifted_cloud(case.shift)
    out = []
    if case.lidar:
        t_gb = case.t_gb
        out.append(dict(sid=0, kind="lidar", data=scenes.lidar_scan(scenes.cloud_c2()[:, :3], seed=5), t_bs=TBS_LIDAR, t_gb=t_gb))
    for k, (yaw, dx) in enumerate(case.poses):
        t_gb = dc.base_pose(case.shift, yaw=yaw, dx=dx)
        for i, t_bc in enumerate(case.rig):
            m2s = F.compose(t_gb, t_bc)
            st = dict(sid=case.first_source + i, t_gb=t_gb, stamp=10**9 + 50 * MS * k, m2s=m2s)
            seed = case.seed + 10 * k + i
            if case.few is not None:
                ahead = np.array([[2.0 + 0.1 * j, 0.0, 0.0] for j in range(case.few)], np.float32)
                st.update(kind="frame", data=ahead, t_bs=t_bc)
            elif case.kind == "image":
                img, k4 = scenes.depth_image(cloud, m2s, case.width, case.height, dc.FOV_W, dc.FOV_V, dc.D_MAX, seed=seed)
                st.update(kind="image", data=img, K4=k4, t_bs=F.compose(t_bc, scenes.T_LINK_OPTICAL))
            else:
                st.update(kind="frame", data=dc.render(cloud, t_gb, t_bc, seed, case.width, case.height), t_bs=t_bc)
            out.append(st)
    return out


# zero-depth pixels are dropped (the library's flag): the node would turn them into a point AT the camera, whose centroid
# sits on the frustum's side planes, where no margin can be kept
IMAGE_NODE = dict(max_distance=6.0, leaf_size=0.05, sample_step=2, drop_zero=True)


def restated_observation(case, feed_steps):
    """the depth sources' alive frames in source order and the frustums, from the feed's restatement ->
    (obs [N,3] float32, frustums, survivors of the largest frame)"""
    bufs, frs, most = {}, {}, 0
    for st in feed_steps:
        if st["kind"] == "lidar":
            continue
        b = bufs.setdefault(st["sid"], F.DepthBufferRef(dc.Z_MIN, dc.Z_MAX, case.persistence_ns))
        raw = I.stage_one(st["data"], st["K4"], **IMAGE_NODE) if st["kind"] == "image" else st["data"]
        most = max(most, F.n_survivors(raw, st["t_bs"], dc.Z_MIN, dc.Z_MAX))
        b.buffer_cloud(raw, st["t_bs"], st["t_gb"], st["stamp"])
        frs[st["sid"]] = R.Frustum(dc.FOV_W, dc.FOV_V, dc.D_MIN, dc.D_MAX, st["m2s"])
    sids = sorted(bufs)
    return np.concatenate([bufs[s].observation() for s in sids], axis=0), [frs[s] for s in sids], most


def statics(case, obs, frustums):
    """-> (ground [G,3], map [M,3]) float32: a lattice 0.05 m under the scene's floor with a node raised next to the
    centroid of every 6th cluster; the map is every 5th observation point more than 2 m ahead of the robot, moved by
    2 cm, and a point next to the centroid of every 6th cluster (offset by one)"""
    rng = np.random.Generator(np.random.PCG64(case.seed))
    t_gb = case.t_gb
    gx, gy = np.meshgrid(np.arange(-7.0, 7.001, 0.25), np.arange(-7.0, 7.001, 0.25), indexing="ij")
    lattice = np.stack([gx.ravel() + t_gb[0], gy.ravel() + t_gb[1], np.full(gx.size, t_gb[2] - 0.05)], axis=1)
    none = np.zeros((0, 3), np.float32)
    first = M.self_mark(frustums, obs, none, none, case.res, case.hres, case.tol, case.min_size, 1.0, t_gb)
    cents = np.array([cl["centroid"] for cl in first["clusters"]], dtype=np.float64).reshape(-1, 3)
    cents = cents[np.lexsort((cents[:, 2], cents[:, 1], cents[:, 0]))]      # an order that does not depend on cluster order
    raised = cents[0::6] + np.array([0.03, -0.02, -0.04])
    ground = np.concatenate([lattice, raised], axis=0).astype(np.float32)
    if not case.with_map:
        return ground, none
    ahead = obs[(obs[:, 0].astype(np.float64) - t_gb[0]) > 2.0][::5].astype(np.float64)
    ahead = ahead + rng.uniform(-0.02, 0.02, ahead.shape)
    smap = np.concatenate([ahead, cents[1::6] + np.array([-0.04, 0.03, 0.02])], axis=0).astype(np.float32)
    return ground, smap


def restate(case, frustums, obs, ground, smap):
    return M.self_mark(frustums, obs, ground, smap, case.res, case.hres, case.tol, case.min_size, case.ratio, case.t_gb)


_BUILT = {}


def built(name):
    """everything a test needs of a case, computed once: (case, steps, obs, frustums, survivors, ground, map, result)"""
    if name not in _BUILT:
        case = BY_NAME[name]
        st = steps(case)
        obs, frs, most = restated_observation(case, st)
        ground, smap = statics(case, obs, frs)
        _BUILT[name] = (case, st, obs, frs, most, ground, smap, restate(case, frs, obs, ground, smap))
    return _BUILT[name]


def find_seed(name, tries=40):
    """the first seed from the case's own on at which every cluster keeps its margins (how the committed ones were found)"""
    case = BY_NAME[name]
    for seed in range(case.seed, case.seed + tries):
        case.seed = seed
        _BUILT.pop(name, None)
        ok, _ = M.margins_kept(built(name)[7])
        if ok:
            return seed
    return None
