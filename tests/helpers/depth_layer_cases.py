"""The update sequences tests/test_depth_layer_cpu.py and tests/test_depth_layer_gpu.py share, built on the depth-clear
rigs (depth_clear_cases) like depth_mark_cases.  CPU only.

A case is a sequence of 4-6 updates.  Every update renders the rig's 160 x 120 frames (or images) from the two-camera
scene plus the boxes that stand in it at that update -- boxes appear and disappear between updates, so that clearing
really happens -- feeds them, and runs one layer update at the update's pose.  The ground cloud is marking.ground_lattice
under the scene.  The committed seeds are such that in the restatement alone every marking and cluster of every update
keeps the margins of depth_layer_ref.margins_kept (tests/test_depth_layer_cpu.py asserts it; find_seed searched them)."""
import numpy as np

from dddmr_navigation_amd import marking, scenes

import depth_clear_cases as dc
import depth_feed_ref as F
import depth_frustum_ref as R
import depth_image_ref as I
import depth_layer_ref as L
import depth_mark_cases as mc

MS = 1_000_000
OFFSET = np.array([0.0137, 0.0131, 0.0071])       # keeps the poses off the voxel lattice (the window's bounds)


class Up:
    """one update: the robot's yaw and x offset, the boxes standing, `few` = an observation of that many points, `reset` =
    dddmr_rollout_depth_layer_reset before it"""

    def __init__(self, yaw=0.05, dx=0.0, boxes=(), few=None, reset=False):
        self.yaw, self.dx, self.boxes, self.few, self.reset = yaw, dx, tuple(boxes), few, reset


class Case:
    def __init__(self, name, seed, ups, cams=1, far=False, kind="frame", lidar=False, res=0.05, hres=0.05, tol=0.1, min_size=1,
                 ratio=0.5, window=5.0, marking_height=2.0, inscribed=0.4, inflation=0.8, max_markings=1 << 12,
                 max_cluster_points=1 << 16, width=160, height=120, sparse=False):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    @property
    def shift(self):
        return (dc.SHIFT_FAR if self.far else np.zeros(3)) + OFFSET

    @property
    def rig(self):
        return (dc.T_BASE_CAM_ROLLED if self.far else dc.T_BASE_CAM)[: self.cams]

    @property
    def first_source(self):
        return 1 if self.lidar else 0

    def layer_kw(self):
        return dict(xy_resolution=self.res, height_resolution=self.hres, marking_height=self.marking_height,
                    perception_window_size=self.window, euclidean_cluster_extraction_tolerance=self.tol,
                    euclidean_cluster_extraction_min_cluster_size=self.min_size, segmentation_ignore_ratio=self.ratio,
                    inscribed_radius=self.inscribed, inflation_radius=self.inflation, max_obstacle_distance=9999.0)


A, B, C = (0, 1), (1, 2), (0, 2)
CASES = [
    Case("one_camera", 403, [Up(boxes=A), Up(boxes=B), Up(boxes=()), Up(boxes=C), Up(boxes=A)]),
    Case("two_cameras_images", 413, [Up(boxes=A), Up(boxes=B), Up(boxes=C), Up(boxes=())], cams=2, kind="image", tol=0.15, min_size=4),
    Case("lidar_beside", 426, [Up(boxes=A), Up(boxes=()), Up(boxes=B), Up(boxes=A)], cams=2, lidar=True),
    Case("far_rolled", 444, [Up(boxes=A), Up(boxes=B), Up(boxes=()), Up(boxes=C)], cams=2, far=True, res=0.3, min_size=5, sparse=True),
    Case("turning", 451, [Up(yaw=0.05, boxes=A), Up(yaw=0.5, boxes=A), Up(yaw=1.0, boxes=B), Up(yaw=1.6, boxes=()), Up(yaw=0.05, boxes=C)], cams=2),
    Case("out_and_back", 450, [Up(boxes=A), Up(dx=0.4, boxes=B), Up(dx=11.0, boxes=()), Up(dx=11.0, boxes=()), Up(boxes=B)]),
    Case("few_points_in_the_middle", 462, [Up(boxes=A), Up(boxes=A), Up(few=5), Up(boxes=B), Up(boxes=())]),
    Case("contested_voxels", 472, [Up(boxes=A), Up(boxes=B), Up(boxes=()), Up(boxes=C)], cams=2, res=0.3, tol=0.1, min_size=2),
    Case("remarked_while_alive", 480, [Up(boxes=A), Up(boxes=A), Up(boxes=A), Up(boxes=A)]),
    Case("reset_in_the_middle", 490, [Up(boxes=A), Up(boxes=B), Up(boxes=B, reset=True), Up(boxes=C)]),
    Case("housekeeping", 501, [Up(boxes=A), Up(yaw=0.4, boxes=B), Up(yaw=0.8, boxes=()), Up(yaw=0.4, boxes=C), Up(boxes=A), Up(yaw=0.6, boxes=B)],
         max_markings=256, max_cluster_points=4096),
]
BY_NAME = {c.name: c for c in CASES}
# 0.3 m voxels contested by clusters of EQUAL size too (where the reference's order is libstdc++'s introsort's and the
# restatement's stable sort may differ): replayed against the host-split path only, whose order is the library's own replay.
EQUAL = Case("contested_equal_sizes", 470, [Up(boxes=A), Up(boxes=B), Up(boxes=()), Up(boxes=C)], cams=2, res=0.3, tol=0.05, min_size=4)
BY_NAME[EQUAL.name] = EQUAL


def pose(case, up):
    s = case.shift
    return (float(s[0]) + up.dx, float(s[1]), float(s[2])) + tuple(scenes.quat_from_rpy(0.0, 0.0, up.yaw))


def boxes(case, centres=((2.0, 0.5), (2.6, -0.4), (1.6, -0.9))):
    """three boxes of points 1.5 - 3 m ahead of the first pose, 0.3 m wide, standing on the floor"""
    rng = np.random.Generator(np.random.PCG64(case.seed + 7 * len(centres)))
    out = []
    for centre in centres:
        half, top = (0.07, 0.4) if case.sparse else (0.15, 0.9)
        p = rng.uniform([-half, -half, 0.15], [half, half, top], (600, 3)) + np.array([centre[0], centre[1], 0.0])
        out.append((p + case.shift).astype(np.float32))
    return out


def updates(case):
    """-> list of dicts: feeds (the feed steps of depth_mark_cases.steps: sid, kind, data, t_bs, t_gb, stamp, m2s, K4), t_gb, reset"""
    base = dc.shifted_cloud(case.shift)[:, :3]
    if case.sparse:                                     # the boxes alone (and one that always stands): few enough points for the
        base = boxes(case, ((2.3, 0.1),))[0]            # 1e-6 relative key margins to be reachable kilometres from the origin
    bx = boxes(case)
    out = []
    for k, up in enumerate(case.ups):
        t_gb = pose(case, up)
        cloud = np.concatenate([base] + [bx[i] for i in up.boxes], axis=0)
        feeds = []
        if case.lidar and k == 0:
            feeds.append(dict(sid=0, kind="lidar", data=scenes.lidar_scan(scenes.cloud_c2()[:, :3], seed=5), t_bs=mc.TBS_LIDAR, t_gb=t_gb))
        for i, t_bc in enumerate(case.rig):
            m2s = F.compose(t_gb, t_bc)
            st = dict(sid=case.first_source + i, t_gb=t_gb, stamp=10**9 + 50 * MS * k, m2s=m2s)
            seed = case.seed + 10 * k + i
            if up.few is not None:
                ahead = np.array([[2.0 + 0.1 * j, 0.0, 0.0] for j in range(up.few if i == 0 else 0)], np.float32).reshape(-1, 3)
                st.update(kind="frame", data=ahead, t_bs=t_bc)
            elif case.kind == "image":
                img, k4 = scenes.depth_image(cloud, m2s, case.width, case.height, dc.FOV_W, dc.FOV_V, dc.D_MAX, seed=seed)
                st.update(kind="image", data=img, K4=k4, t_bs=F.compose(t_bc, scenes.T_LINK_OPTICAL))
            else:
                st.update(kind="frame", data=dc.render(cloud, t_gb, t_bc, seed, case.width, case.height), t_bs=t_bc)
            feeds.append(st)
        out.append(dict(feeds=feeds, t_gb=t_gb, reset=up.reset))
    return out


def ground_of(case):
    g = marking.ground_lattice(half=8.0, spacing=0.25).astype(np.float64)
    g[:, 2] -= 0.05
    return (g + case.shift).astype(np.float32)


def layer_ref(case, ground):
    return L.LayerRef(ground, np.zeros((0, 3), np.float32), **{
        "xy_resolution": case.res, "height_resolution": case.hres, "marking_height": case.marking_height,
        "perception_window_size": case.window, "tolerance": case.tol, "min_cluster_size": case.min_size,
        "segmentation_ignore_ratio": case.ratio, "inscribed_radius": case.inscribed, "inflation_radius": case.inflation})


_BUILT = {}


def built(name):
    """everything a test needs of a case, computed once and left unchanged: (case, updates, ground, results) where results[k] =
    depth_layer_ref's result of update k on the restated observation, plus obs, frustums and the alive store after it"""
    if name not in _BUILT:
        case = BY_NAME[name]
        ups = updates(case)
        ground = ground_of(case)
        ref = layer_ref(case, ground)
        bufs, frs, results = {}, {}, []
        for u in ups:
            for st in u["feeds"]:
                if st["kind"] == "lidar":
                    continue
                b = bufs.setdefault(st["sid"], F.DepthBufferRef(dc.Z_MIN, dc.Z_MAX, 0))
                raw = I.stage_one(st["data"], st["K4"], **mc.IMAGE_NODE) if st["kind"] == "image" else st["data"]
                b.buffer_cloud(raw, st["t_bs"], st["t_gb"], st["stamp"])
                frs[st["sid"]] = R.Frustum(dc.FOV_W, dc.FOV_V, dc.D_MIN, dc.D_MAX, st["m2s"])
            sids = sorted(bufs)
            obs = np.concatenate([bufs[s].observation() for s in sids], axis=0)
            fr = [frs[s] for s in sids]
            if u["reset"]:
                ref.reset()
            before = set(ref.alive())
            res = ref.update(fr, obs, u["t_gb"])
            res.update(obs=obs, frustums=fr, alive_before=before, alive={v: pc.copy() for v, pc in ref.alive().items()},
                       dgraph=ref.dgraph.copy(), lethal=ref.lethal.copy())
            results.append(res)
        _BUILT[name] = (case, ups, ground, results)
    return _BUILT[name]


def find_seed(name, tries=40):
    """the first seed from the case's own on at which every update keeps its margins (how the committed ones were found)"""
    case = BY_NAME[name]
    for seed in range(case.seed, case.seed + tries):
        case.seed = seed
        _BUILT.pop(name, None)
        if all(L.margins_kept(r) for r in built(name)[3]):
            return seed
    return None
