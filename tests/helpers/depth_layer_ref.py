"""NumPy / SciPy restatement of the global-mode DepthCameraLayer with its Marking store, DynamicGraph and lethal map: the
yardstick of tests/test_depth_layer_cpu.py and tests/test_depth_layer_gpu.py.

Written from the reference source (dddmr_perception_3d/plugins/depth_camera/depth_camera_layer.cpp:252-426, :487-601;
plugins/cluster_marking.cpp:49-138; src/graph/dynamic_graph.cpp:38-61), float32 / float64 exactly where the reference's
types put them; it imports nothing from the library under test.  selfClear's verdicts are depth_frustum_ref.clear_verdicts,
selfMark's clusters are depth_mark_ref.self_mark; this file adds
  the store      dict voxel key -> per_marking(pc_, nodes_of_min_distance_); pc_ None = cleared, the key stays
  the window     [(int)((t -+ window) / res)) per axis, half open because of lower_bound; double division, truncated
  addPCPtr       the slot's pc_ and nodes are REPLACED (no clearValue of the old ones); ProjectInliers on the plane of
                 :568-578 in float32 with Eigen's reduction order (a0 + a2) + (a1 + a3) and the normal normalised; the
                 0.1 m VoxelGrid (depth_feed_ref.voxel_centroids); radiusSearch(inflation_radius) on the ground (FLANN
                 float distance, strict <); nodes[node] = min sqrtf(dx^2 + dy^2); setValue(node, d) = min in double;
                 lethal where d <= inscribed_radius
  removePCPtr    every stored node: clearValue(node, 9999.0) whatever else covers it; erased from the lethal map where
                 the stored distance is <= inscribed_radius
  the dGraph     float64, `initial` fills n + 1 entries with max_obstacle_distance

Every update also reports the MARGINS of the comparisons the new code makes (see margins_kept)."""
import numpy as np
from scipy.spatial import cKDTree

import depth_feed_ref as F
import depth_frustum_ref as R
import depth_mark_ref as M

f32 = np.float32
MARGIN_REL = 1e-6


def window(t_gb, window_size, marking_height, res, hres):
    """-> ((x0, x1), (y0, y1), (z0, z1)) voxel keys, and the smallest relative distance of a bound from an integer"""
    q = [(float(t_gb[0]) - window_size) / res, (float(t_gb[0]) + window_size) / res,
         (float(t_gb[1]) - window_size) / res, (float(t_gb[1]) + window_size) / res,
         (float(t_gb[2]) - marking_height) / hres, (float(t_gb[2]) + marking_height) / hres]
    k = [int(v) for v in q]                                             # C++ double -> int: truncation
    margin = min(abs(v - round(v)) / max(abs(v), 1e-300) for v in q)
    return ((k[0], k[1]), (k[2], k[3]), (k[4], k[5])), margin


def project(points, plane):
    """pcl::ProjectInliers(SACMODEL_PLANE) as Eigen evaluates it: float32, 4-float dot products reduced (a0 + a2) + (a1 + a3)"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    m0, m1, m2, m3 = f32(plane[0]), f32(plane[1]), f32(plane[2]), f32(0.0)
    nrm = np.sqrt((m0 * m0 + m2 * m2) + (m1 * m1 + m3 * m3))
    m0, m1, m2 = m0 / nrm, m1 / nrm, m2 / nrm
    dist = (m0 * p[:, 0] + m2 * p[:, 2]) + (m1 * p[:, 1] + f32(plane[3]) * f32(1.0))
    return np.stack([p[:, 0] - m0 * dist, p[:, 1] - m1 * dist, p[:, 2] - m2 * dist], axis=1).astype(f32)


class LayerRef:
    def __init__(self, ground, smap, xy_resolution, height_resolution, marking_height, perception_window_size, tolerance,
                 min_cluster_size, segmentation_ignore_ratio, inscribed_radius, inflation_radius, max_obstacle_distance=9999.0):
        self.ground = np.asarray(ground, dtype=f32).reshape(-1, 3)
        self.smap = np.asarray(smap, dtype=f32).reshape(-1, 3)
        self.res, self.hres = float(xy_resolution), float(height_resolution)
        self.marking_height, self.window_size = float(marking_height), float(perception_window_size)
        self.tol, self.min_size, self.ratio = float(tolerance), int(min_cluster_size), float(segmentation_ignore_ratio)
        self.inscribed, self.inflation, self.max_d = float(inscribed_radius), float(inflation_radius), float(max_obstacle_distance)
        self.gtree = cKDTree(self.ground.astype(np.float64))
        self.reset()

    def reset(self):
        """resetdGraph"""
        self.store = {}
        self.dgraph = np.full(len(self.ground) + 1, self.max_d, np.float64)
        self.lethal = np.zeros(len(self.ground) + 1, bool)

    # ---- Marking ----
    def nodes_of_min_distance(self, pc, plane, margins):
        gen, _ = F.voxel_centroids(project(pc, plane), 0.1)
        q = project(pc, plane).astype(np.float64) * 10.0
        margins["gen_key"] = min(margins["gen_key"], float(np.min(np.abs(q - np.rint(q)) / np.maximum(np.abs(q), 1e-300))))
        r2 = f32(self.inflation * self.inflation)
        nodes = {}
        for p, near in zip(gen, self.gtree.query_ball_point(gen.astype(np.float64), self.inflation * 1.001 + 1e-4)):
            if not near:
                continue
            g = self.ground[near]
            d = g[:, 0] - p[0]
            d2 = d * d
            d = g[:, 1] - p[1]
            d2 = d2 + d * d
            d = g[:, 2] - p[2]
            d2 = d2 + d * d
            margins["inflation"] = min(margins["inflation"], float(np.min(np.abs(d2.astype(np.float64) - float(r2)) / float(r2))))
            dx, dy = p[0] - g[:, 0], p[1] - g[:, 1]
            dist = np.sqrt(dx * dx + dy * dy)                           # float sqrt: z dropped on purpose (:86-88)
            for node, d2i, di in zip(near, d2, dist):
                if d2i < r2:
                    margins["inscribed"] = min(margins["inscribed"], abs(float(di) - self.inscribed) / self.inscribed)
                    nodes[node] = min(nodes.get(node, di), di)
        return gen, nodes

    def add_pc_ptr(self, voxel, pc, plane, margins):
        gen, nodes = self.nodes_of_min_distance(pc, plane, margins)
        self.store[tuple(int(v) for v in voxel)] = dict(pc=np.asarray(pc, dtype=f32), nodes=nodes, gen=gen)
        for node, d in nodes.items():
            self.dgraph[node] = min(self.dgraph[node], np.float64(d))
            if np.float64(d) <= self.inscribed:
                self.lethal[node] = True

    def remove_pc_ptr(self, voxel):
        mk = self.store[voxel]
        for node, d in mk["nodes"].items():
            self.dgraph[node] = 9999.0
            if np.float64(d) <= self.inscribed:
                self.lethal[node] = False
        mk["pc"] = None

    def verdict_float_margins(self, frustums, obs, vox, verdict, cl):
        """the floating-point margins of depth_frustum_ref.clear_verdicts (frustum dot products, plane distances, hypot,
        every d^2 against r^2) without its integer one (the engagement ratio one count away from 0.1): a stored pc_ has
        fewer than ten points, so a marking that engages no or one point -- every cleared one -- can never keep that one.
        What stands in for it: the count is an integer that is exact as soon as every pair keeps its d^2 margin, and
        1.0 * engaged / n > 0.1 is then decided by integers unless engaged * 10 == n exactly, the one place where the
        rounding of the double quotient could matter; margins["ratio_tie"] reports such a marking and margins_kept
        refuses it"""
        pt = np.stack([(vox[:, 0] * np.float64(self.res)).astype(f32), (vox[:, 1] * np.float64(self.res)).astype(f32),
                       (vox[:, 2] * np.float64(self.hres)).astype(f32)], axis=1)
        ok = bool(R.point_tests(frustums, pt)[2].all())
        if len(obs) > 5:
            out = (verdict >> 1) == 1
            ok = ok and bool(R.radius_any(obs, pt[out], 0.05)[1].all()) and bool(R.radius_any(obs, cl, 0.01)[1].all())
        return ok

    def alive(self):
        return {v: mk["pc"] for v, mk in self.store.items() if mk["pc"] is not None}

    # ---- one doClear_then_Mark pass ----
    def update(self, frustums, obs, t_gb):
        """-> dict(stats, margins, verdicts {voxel: verdict byte}, mark (depth_mark_ref's result))"""
        obs = np.asarray(obs, dtype=f32).reshape(-1, 3)
        margins = dict(gen_key=np.inf, inflation=np.inf, inscribed=np.inf, window=np.inf, verdicts_ok=True, verdict_floats_ok=True, ratio_tie=False, mark_ok=True,
                       equal_size_contest=False)
        ((x0, x1), (y0, y1), (z0, z1)), margins["window"] = window(t_gb, self.window_size, self.marking_height, self.res, self.hres)
        inwin = sorted(v for v, pc in self.alive().items() if x0 <= v[0] < x1 and y0 <= v[1] < y1 and z0 <= v[2] < z1)
        verdicts = {}
        n_cleared = 0
        if inwin:
            vox = np.array(inwin, np.int32)
            off = np.concatenate([[0], np.cumsum([len(self.store[v]["pc"]) for v in inwin])])
            cl = np.concatenate([self.store[v]["pc"] for v in inwin], axis=0)
            verdict, _, ok = R.clear_verdicts(frustums, obs, self.res, self.hres, vox, off, cl)
            margins["verdicts_ok"] = bool(ok.all())
            margins["verdict_floats_ok"] = self.verdict_float_margins(frustums, obs, vox, verdict, cl)
            size = np.diff(off)
            engaged_all = np.zeros(len(inwin), np.int64)
            if len(obs) > 5:
                hit, _ = R.radius_any(obs, cl, 0.01)
                engaged_all = np.bincount(np.repeat(np.arange(len(inwin)), size), weights=hit, minlength=len(inwin)).astype(np.int64)
            ratio = (verdict >> 1) != 1
            margins["ratio_tie"] = bool((engaged_all[ratio] * 10 == size[ratio]).any())
            for v, b in zip(inwin, verdict):
                verdicts[v] = int(b)
                if not b & 1:
                    self.remove_pc_ptr(v)
                    n_cleared += 1
        mark = M.self_mark(frustums, obs, self.ground, self.smap, self.res, self.hres, self.tol, self.min_size, self.ratio, t_gb)
        margins["mark_ok"] = M.margins_kept(mark)[0]
        claimed = {}
        n_accepted = n_contested = 0
        for c in mark["clusters"]:                                      # the reference's processing order
            if c["fate"] != M.ACCEPTED:
                continue
            v = tuple(int(a) for a in c["voxel"])
            n_accepted += 1
            if v in claimed:
                n_contested += 1
                if c["size"] in claimed[v]:
                    margins["equal_size_contest"] = True
            claimed.setdefault(v, []).append(c["size"])
            self.add_pc_ptr(v, c["points"], mark["plane"], margins)
        stats = dict(n_observation=len(obs), n_in_window=len(inwin), n_cleared=n_cleared, n_clusters=mark["stats"]["n_clusters"],
                     n_accepted=n_accepted, n_contested=n_contested, n_alive=len(self.alive()))
        return dict(stats=stats, margins=margins, verdicts=verdicts, mark=mark, contested_sizes=[s for s in claimed.values() if len(s) > 1])


def margins_kept(result):
    """the margins of one update: the two existing slices' own floating-point ones (see verdict_float_margins), and MARGIN_REL (relative) between every (generator point,
    ground node) pair and inflation_radius^2, every xy distance and inscribed_radius, every projected coordinate and a 0.1 m
    voxel-key integer, every window bound and an integer; no voxel contested by two clusters of equal size"""
    m = result["margins"]
    return (m["verdict_floats_ok"] and not m["ratio_tie"] and m["mark_ok"] and not m["equal_size_contest"] and m["gen_key"] >= MARGIN_REL and
            m["inflation"] >= MARGIN_REL and m["inscribed"] >= MARGIN_REL and m["window"] >= MARGIN_REL)
