"""Serial NumPy restatement of the static layer's regeneration (dddmr_perception_3d/plugins/static_layer.cpp:201-285,
:287-420) and of the no-entry layer's inflation (no_entry_layer.cpp:265-283), with exactly the expressions of DESIGN.md
4d-3: FLANN's float L2_Simple, radiusSearch's strict d2 < float(double(r) * double(r)), sqrtf for an edge weight,
double(sqrtf(d2)) for a dGraph value, pcl::PassThrough with float limits and both ends inclusive, setValue as a minimum.

UNPINNED: PCL and FLANN cannot be built here, so nothing below has been compared with the reference's own binaries; the
assumptions are listed in DESIGN.md 4d-3 (S1-S7).

Two versions: build() / zones() propose candidates with SciPy's cKDTree inside a padded radius and decide with the float
expression; build_all_pairs() / zones_all_pairs() need NumPy only and test every pair.  tests/test_static_layer_cpu.py
holds them against each other.

cfg is a dict with the fields of dddmr_static_layer_config that are parameters (see CFG)."""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64
ADAPTIVE_STEPS = 101
MIN_NEIGHBOURS = 5          # static_layer.cpp:343
OVERHANG_COUNT = 10         # :412
OVERHANG_VALUE = 0.25       # :413
PAD = 1e-3                  # the tree's double distance against the float one: candidates only

# p2p_move_base_localization.yaml
CFG = dict(use_adaptive_connection=0, adaptive_connection_number=20, radius_of_ground_connection=1.5, static_imposing_radius=1.5,
           inscribed_radius=0.5, max_obstacle_distance=9999.0, enable_edge_detection=1, generate_static_graph=1)


def config(**kw):
    c = dict(CFG)
    for k, v in kw.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def adaptive_radius(k: int) -> float:
    """search_r + 0.2 * search_cnt with `float search_r = 0.5` (:246-249): a double"""
    return float(D(F(0.5)) + D(0.2) * D(k))


def radius2(r: float) -> np.float32:
    return F(D(r) * D(r))


def adaptive_r2_table() -> np.ndarray:
    """[102] float32, entry 0 unused"""
    return np.array([0.0] + [radius2(adaptive_radius(k)) for k in range(1, ADAPTIVE_STEPS + 1)], F)


def l2_simple(a, b) -> np.ndarray:
    """FLANN L2_Simple<float> between rows of a and b (broadcast): result += diff * diff per dimension, in float"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    d = a - b
    r = d[..., 0] * d[..., 0]
    r = r + d[..., 1] * d[..., 1]
    r = r + d[..., 2] * d[..., 2]
    return r.astype(F)


def _limits(q):
    """the three PassThrough windows of node q (:399-410): float limits from double sums"""
    lo = np.array([F(D(q[0]) - 0.5), F(D(q[1]) - 0.5), F(D(q[2]) + 0.1)], F)
    hi = np.array([F(D(q[0]) + 0.5), F(D(q[1]) + 0.5), F(D(q[2]) + 1.0)], F)
    return lo, hi


def _finish(ground, rows, kidx, counts, qualifying, nearest, cfg):
    """rows: per node (ascending neighbour indices, their d2); qualifying: per node the overhang count of map points;
    nearest: per node the smallest d2 to a map point (inf without a map)"""
    n = len(ground)
    mod = D(cfg["max_obstacle_distance"])
    dgraph = np.full(n + 1, mod, D)
    overhang = np.zeros(n, bool)
    near = np.zeros(n, bool)
    if cfg["enable_edge_detection"]:
        overhang = (counts >= MIN_NEIGHBOURS) & (qualifying > OVERHANG_COUNT)
        dgraph[:n][overhang] = np.minimum(dgraph[:n][overhang], OVERHANG_VALUE)
    if cfg["generate_static_graph"]:
        d = np.sqrt(nearest.astype(F)).astype(D)           # double(sqrtf(d2))
        near = np.isfinite(nearest) & (d < D(cfg["inscribed_radius"]))
        dgraph[:n][near] = np.minimum(dgraph[:n][near], d[near])
    if cfg["generate_static_graph"]:
        deg = np.array([len(r[0]) for r in rows], np.int64)
        row_start = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
        neighbour = np.concatenate([r[0] for r in rows]).astype(np.uint32) if n else np.zeros(0, np.uint32)
        weight = np.sqrt(np.concatenate([r[1] for r in rows]).astype(F)).astype(F) if n else np.zeros(0, F)
    else:
        row_start, neighbour, weight = np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, F)
    return dict(row_start=row_start, neighbour=neighbour, weight=weight, dgraph=dgraph, kidx=np.asarray(kidx, np.int32), counts=np.asarray(counts, np.int64),
                qualifying=np.asarray(qualifying, np.int64), nearest=np.asarray(nearest, F), overhang=overhang, near=near)


def build(ground, map_pts, cfg) -> dict:
    """One selfClear regeneration; candidates from cKDTree, decisions by the float expressions."""
    from scipy.spatial import cKDTree

    ground = np.asarray(ground, F).reshape(-1, 3)
    map_pts = np.asarray(map_pts, F).reshape(-1, 3)
    n = len(ground)
    gtree = cKDTree(ground.astype(D))
    mtree = cKDTree(map_pts.astype(D)) if len(map_pts) else None
    tab = adaptive_r2_table()

    def ball(tree, pts, q, r, r2):
        cand = np.array(sorted(tree.query_ball_point(q.astype(D), float(r) + PAD)), np.int64)
        d2 = l2_simple(pts[cand], q) if len(cand) else np.zeros(0, F)
        keep = d2 < r2
        return cand[keep], d2[keep]

    rows, kidx, counts, qualifying, nearest = [], [], np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, np.inf, F)
    r_fixed = float(cfg["radius_of_ground_connection"])
    for i in range(n):
        q = ground[i]
        if not cfg["use_adaptive_connection"]:
            k, row = 0, ball(gtree, ground, q, r_fixed, radius2(r_fixed))
        else:
            for k in range(1, ADAPTIVE_STEPS + 1):           # the reference's loop with its hard_interrupt_cnt
                row = ball(gtree, ground, q, adaptive_radius(k), tab[k])
                if len(row[0]) >= cfg["adaptive_connection_number"]:
                    break
        rows.append(row)
        kidx.append(k)
        counts[i] = len(row[0])
        if mtree is not None:
            r = float(cfg["static_imposing_radius"])
            idx, _ = ball(mtree, map_pts, q, r, radius2(r))
            lo, hi = _limits(q)
            p = map_pts[idx]
            ok = np.isfinite(p).all(axis=1) & (p >= lo).all(axis=1) & (p <= hi).all(axis=1)
            qualifying[i] = int(ok.sum())
            # the nearest map point: only a distance below inscribed_radius matters, so that far plus a margin is enough
            cand = mtree.query_ball_point(q.astype(D), float(cfg["inscribed_radius"]) + 0.1)
            if len(cand):
                nearest[i] = l2_simple(map_pts[np.array(cand, np.int64)], q).min()
    return _finish(ground, rows, kidx, counts, qualifying, nearest, cfg)


def build_all_pairs(ground, map_pts, cfg) -> dict:
    """The same with every pair tested (NumPy only)."""
    ground = np.asarray(ground, F).reshape(-1, 3)
    map_pts = np.asarray(map_pts, F).reshape(-1, 3)
    n = len(ground)
    tab = adaptive_r2_table()
    d2 = l2_simple(ground[None, :, :], ground[:, None, :])                  # [node, candidate]
    if not cfg["use_adaptive_connection"]:
        kidx = np.zeros(n, np.int32)
        r2 = np.full(n, radius2(float(cfg["radius_of_ground_connection"])), F)
    else:
        srt = np.sort(d2, axis=1)
        kidx = np.full(n, ADAPTIVE_STEPS, np.int32)
        open_ = np.ones(n, bool)
        for k in range(1, ADAPTIVE_STEPS + 1):
            cnt = (srt[:, : cfg["adaptive_connection_number"]] < tab[k]).sum(axis=1)
            hit = open_ & (cnt >= cfg["adaptive_connection_number"])
            kidx[hit] = k
            open_ &= ~hit
        r2 = tab[kidx]
    inside = d2 < r2[:, None]
    rows = [(np.flatnonzero(inside[i]), d2[i][inside[i]]) for i in range(n)]
    counts = inside.sum(axis=1)
    qualifying, nearest = np.zeros(n, np.int64), np.full(n, np.inf, F)
    if len(map_pts):
        m2 = l2_simple(map_pts[None, :, :], ground[:, None, :])             # [node, map point]
        nearest = m2.min(axis=1)
        ri2 = radius2(float(cfg["static_imposing_radius"]))
        for i in range(n):
            lo, hi = _limits(ground[i])
            ok = (m2[i] < ri2) & np.isfinite(map_pts).all(axis=1) & (map_pts >= lo).all(axis=1) & (map_pts <= hi).all(axis=1)
            qualifying[i] = int(ok.sum())
    return _finish(ground, rows, kidx, counts, qualifying, nearest, cfg)


def zones(ground, zone_pts, inflation_distance, max_obstacle_distance) -> np.ndarray:
    """The no-entry dGraph [n + 1] by the reference's loop (no_entry_layer.cpp:265-283): for every zone point, every ground
    node inside radiusSearch(zone point, inflation_distance) takes min(old, double(sqrtf(d2)))."""
    from scipy.spatial import cKDTree

    ground = np.asarray(ground, F).reshape(-1, 3)
    zone_pts = np.asarray(zone_pts, F).reshape(-1, 3)
    out = np.full(len(ground) + 1, D(max_obstacle_distance), D)
    if not len(zone_pts):
        return out
    tree = cKDTree(ground.astype(D))
    r2 = radius2(inflation_distance)
    for z in zone_pts:
        cand = np.array(tree.query_ball_point(z.astype(D), float(inflation_distance) + PAD), np.int64)
        if not len(cand):
            continue
        d2 = l2_simple(ground[cand], z)
        keep = d2 < r2
        idx, d = cand[keep], np.sqrt(d2[keep]).astype(D)
        np.minimum.at(out, idx, d)
    return out


def zones_all_pairs(ground, zone_pts, inflation_distance, max_obstacle_distance) -> np.ndarray:
    ground = np.asarray(ground, F).reshape(-1, 3)
    zone_pts = np.asarray(zone_pts, F).reshape(-1, 3)
    out = np.full(len(ground) + 1, D(max_obstacle_distance), D)
    if not len(zone_pts):
        return out
    d2 = l2_simple(ground[:, None, :], zone_pts[None, :, :])                # [node, zone point]: the zone point is the query
    best = np.where(d2 < radius2(inflation_distance), d2, F(np.inf)).min(axis=1)
    hit = np.isfinite(best)
    out[: len(ground)][hit] = np.minimum(out[: len(ground)][hit], np.sqrt(best[hit]).astype(D))
    return out
