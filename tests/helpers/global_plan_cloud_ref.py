"""Serial Python restatement of the global planner's default A* (dddmr_global_planner/src/a_star_on_pc.cpp:
A_Star_on_Graph::getPath :200-329, isLineOfSightClear :168-198, AstarList :41-100; the kd-tree wrapper
include/global_planner/nanoflann_pcl.hpp:176-213) with brute-force searches in NumPy float32 and global_plan_ref's
containers, and exactly the expressions of DESIGN.md 4d-5: float where the reference has float, double where it has
double, nothing fused.

UNPINNED: nothing here is held to compiled reference code yet (nanoflann is part of the reference, so a later change can
pin it to the real search).  What it assumes beyond the text of the reference: nanoflann's pruned
search returns exactly the points its own float metric admits; a result list is ascending in distance; equal distances
are taken in ascending index (nanoflann orders them by its tree walk).  The deliberate differences are the device's:
NO_PATH on a set emptied by discards; an edge whose march would take more than LOS_MAX_SAMPLES samples is blocked without
a march; a successor list longer than MAX_SUCCESSORS ends the search with ROW_FULL.

plan() takes the ground [n,3] float32, a dGraph [n+1] float64, the aggregate lethal cloud [m,3] float32 (duplicates are
points of their own), the ground's intensity and sGraph's node weights ([n] float32 or None) and cfg (config())."""
from __future__ import annotations

import numpy as np

import global_plan_ref as G
from global_plan_ref import BUDGET, FOUND, NO_PATH, OPEN_FULL, SortedSet, dist  # noqa: F401

F = np.float32
D = np.float64
ROW_FULL = 4
MAX_SUCCESSORS, LOS_MAX_SAMPLES, KNN = 1024, 4096, 8
COUNTERS = ("n_knn_fallbacks", "n_lethal_skipped", "n_los_tested", "n_los_blocked", "n_los_capped", "max_successors")

CFG = dict(turning_weight=0.1, a_star_expanding_radius=0.5, inscribed_radius=0.15, inflation_descending_rate=2.0,
           max_open_entries=1 << 16, max_expansions=4096)


def config(**kw):
    c = dict(CFG)
    for k, v in kw.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def radius2(radius) -> np.float32:
    """nanoflann_pcl.hpp:189, :202: the radius becomes a float at the call and is squared in float"""
    r = F(radius)
    return F(r * r)


def l2_simple(cloud, p) -> np.ndarray:
    """nanoflann's L2_Simple in float: ((dx*dx) + dy*dy) + dz*dz"""
    d = (np.asarray(cloud, F).reshape(-1, 3) - np.asarray(p, F)).astype(F)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)


def successors(ground, cur, radius):
    """:240-245 -> (ids, d2, fallback): radiusSearch keeps d2 < r2 strictly; fewer than 8: the 8 nearest at whatever
    distance.  Ascending in (d2, index)."""
    d2 = l2_simple(ground, ground[cur])
    ids = np.flatnonzero(d2 < radius2(radius))
    fallback = len(ids) < KNN
    if fallback:
        ids = np.arange(len(d2))
    order = np.lexsort((ids, d2[ids]))
    ids = ids[order][:KNN] if fallback else ids[order]
    return ids.astype(np.int64), d2[ids], fallback


def los_dt(pc, pe, inscribed) -> np.float32:
    """:171-180"""
    dX, dY, dZ = F(pe[0] - pc[0]), F(pe[1] - pc[1]), F(pe[2] - pc[2])
    distance = np.sqrt(F(F(dX * dX + dY * dY) + dZ * dZ)).astype(F)
    with np.errstate(divide="ignore", over="ignore"):
        distance = F(D(distance) / D(inscribed))
        return F(F(1) / distance)


def los_ts(dt, cap=LOS_MAX_SAMPLES):
    """:181  the t of every sample the loop visits: accumulated in float, the end test in double.  None beyond `cap`."""
    ts = []
    t = F(0)
    with np.errstate(over="ignore"):
        while D(t) <= 1.0 + D(dt):
            ts.append(t)
            if len(ts) > cap:
                return None
            t = F(t + dt)
    return ts


def los_samples(pc, pe, ts) -> np.ndarray:
    """:182-189  r = t, 1 from t >= 1 on; the sample cur + d * r per coordinate in float"""
    pc, pe = np.asarray(pc, F), np.asarray(pe, F)
    d = (pe - pc).astype(F)
    r = np.array([F(1) if t >= 1.0 else t for t in ts], F)
    return (pc[None, :] + (d[None, :] * r[:, None]).astype(F)).astype(F)


def line_of_sight(pc, pe, inscribed, lethal, stats=None):
    """isLineOfSightClear -> (clear, capped, samples the loop has).  The samples are tested in order and the march stops at
    the first that finds more than one lethal point (:193); the verdict is an OR."""
    dt = los_dt(pc, pe, inscribed)
    ts = los_ts(dt)
    if ts is None:
        return False, True, LOS_MAX_SAMPLES + 1
    if stats is not None:
        stats["longest_march"] = max(stats["longest_march"], len(ts))
    if len(lethal) == 0:                                                       # :226  no cloud in the tree: nothing is found
        return True, False, len(ts)
    r2 = radius2(2.0 * D(inscribed))                                           # :192
    for s in los_samples(pc, pe, ts):
        inside = l2_simple(lethal, s) < r2
        c = int(inside.sum())
        if stats is not None:
            stats["single_point_samples"] += c == 1
            stats["blocked_by_one_node_twice"] += c > 1 and len(np.unique(lethal[inside], axis=0)) == 1
        if c > 1:
            return False, False, len(ts)
    return True, False, len(ts)


def new_g(g, edge, factor, node_weight, theta, turning_weight, avg_intensity) -> np.float32:
    """:288, left to right: the first sum in float, the others in double, the result a float"""
    ge = F(F(g) + F(edge))
    return F((((D(ge) + D(factor) * 1.0) + D(F(node_weight))) + D(theta) * D(turning_weight)) + D(F(avg_intensity)))


def plan(ground, dgraph, lethal, intensity, node_weights, cfg, start, goal, stats=None) -> dict:
    """One getPath.  Returns what global_plan_ref.plan returns (status, path, n_expanded, n_pushed, n_discarded_closed,
    g_goal, ...) and the device's counters (COUNTERS)."""
    ground = np.asarray(ground, F)
    dgraph = np.asarray(dgraph, D)
    lethal = np.zeros((0, 3), F) if lethal is None else np.asarray(lethal, F).reshape(-1, 3)
    inten = None if intensity is None else np.asarray(intensity, F)
    nwt = np.zeros(len(ground), F) if node_weights is None else np.asarray(node_weights, F)
    tw, radius, inscribed, rate = D(cfg["turning_weight"]), D(cfg["a_star_expanding_radius"]), D(cfg["inscribed_radius"]), D(cfg["inflation_descending_rate"])
    assert inscribed > 0 and len(ground) >= KNN
    start, goal = int(start), int(goal)
    st = stats if stats is not None else {}
    for k in ("single_point_samples", "blocked_by_one_node_twice", "longest_march", "fallback_reach_over_1m", "threshold_equal_clear",
              "threshold_equal_blocked", "updates", "popped_behind_discards", "ended_on_emptied_set"):
        st.setdefault(k, 0)
    ctr = {k: 0 for k in COUNTERS}

    rec, closed = {}, set()
    frontier = SortedSet()
    f0 = F(dist(ground[start], ground[goal]))                                 # :212
    rec[start] = (F(0), f0, start)                                            # :213
    frontier.insert((float(f0), start))
    n_expanded = n_discarded = 0
    n_pushed = 1
    status = NO_PATH
    ended_on_emptied_set = False

    while True:
        # getNode_wi_MinimumF (:70-88), as global_plan_ref.plan
        if len(frontier) == 0:
            status = NO_PATH
            break
        if n_expanded >= cfg["max_expansions"]:
            status = BUDGET
            break
        first = frontier.begin()
        cur = None
        if first[1] not in closed:
            frontier.erase(first)                                             # :74
            cur = first[1]
        else:
            while True:                                                       # :81-86
                frontier.erase(first)
                n_discarded += 1
                if len(frontier) == 0:
                    break
                first = frontier.begin()
                if first[1] not in closed:
                    cur = first[1]                                            # (its entry stays in the set)
                    st["popped_behind_discards"] += 1
                    break
            if cur is None:                                                   # :85 reads begin() of the empty set: undefined there
                status = NO_PATH
                ended_on_emptied_set = True
                st["ended_on_emptied_set"] += 1
                break
        g_cur, _, parent = rec[cur]
        pc, pp = ground[cur], ground[parent]

        ids, d2s, fallback = successors(ground, cur, radius)                  # :240-245
        ctr["n_knn_fallbacks"] += fallback
        ctr["max_successors"] = max(ctr["max_successors"], len(ids))
        if fallback and float(np.sqrt(d2s[-1])) > 1.0:
            st["fallback_reach_over_1m"] += 1
        if len(ids) > MAX_SUCCESSORS:
            status = ROW_FULL
            break
        avg = F(0)
        if inten is not None:                                                 # :248-252  a float sum in list order
            s = F(0)
            for n in ids:
                s = F(s + inten[n])
            avg = F(s / F(len(ids)))
        before = len(frontier)
        for n, d2 in zip(ids, d2s):
            n = int(n)
            edge = np.sqrt(F(d2)).astype(F)                                   # :257
            d = dgraph[n]                                                     # :260
            if d < inscribed:                                                 # :263
                ctr["n_lethal_skipped"] += 1
                continue
            pe = ground[n]
            if D(edge) >= 2.0 * inscribed:                                    # :273
                ctr["n_los_tested"] += 1
                clear, capped, _ = line_of_sight(pc, pe, inscribed, lethal, st)
                if D(edge) == 2.0 * inscribed:
                    st["threshold_equal_clear" if clear else "threshold_equal_blocked"] += 1
                if not clear:
                    ctr["n_los_blocked"] += 1
                    ctr["n_los_capped"] += capped
                    continue
            factor = np.exp(-1.0 * rate * (d - inscribed))                    # :278
            theta = G.theta_many(np.array([[pp[0], pp[1], pc[0], pc[1], pe[0], pe[1]]], F))[0]   # :281
            ng = new_g(g_cur, edge, factor, nwt[n], theta, tw, avg)           # :288
            nh = F(dist(pe, ground[goal]))                                    # :289
            nf = F(ng + nh)                                                   # :290
            if n in closed:                                                   # :295
                continue
            if n in rec:                                                      # :298
                if not (rec[n][0] > ng):                                      # :299
                    continue
                st["updates"] += 1
            rec[n] = (ng, nf, cur)                                            # updateNode (:61-68)
            frontier.insert((float(nf), n))
        n_pushed += len(frontier) - before
        if len(frontier) > cfg["max_open_entries"]:
            status = OPEN_FULL
            break
        closed.add(cur)                                                       # :312
        n_expanded += 1
        if goal in closed:                                                    # :315
            status = FOUND
            break

    path = []
    if status == FOUND:                                                       # :316-322
        t = goal
        while rec[t][2] != t:
            path.append(t)
            t = rec[t][2]
        path.append(t)
        path.reverse()
    out = dict(status=status, path=np.array(path, np.uint32), n_expanded=n_expanded, n_pushed=n_pushed, n_discarded_closed=n_discarded,
               g_goal=F(rec[goal][0]) if status == FOUND else F(0), closed=closed, set_size=len(frontier), ended_on_emptied_set=ended_on_emptied_set)
    out.update(ctr)
    return out


def lethal_count_brute(lethal, samples, inscribed) -> np.ndarray:
    """For the CPU test's second opinion: the points of `lethal` inside radiusSearch(s, 2 * inscribed_radius) for every
    sample, as one distance table (written apart from line_of_sight)."""
    a = np.asarray(samples, F)[:, None, :] - np.asarray(lethal, F)[None, :, :]
    d2 = ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]).astype(F) + a[..., 2] * a[..., 2]).astype(F)
    r = F(2.0 * D(inscribed))
    return (d2 < F(r * r)).sum(axis=1)
