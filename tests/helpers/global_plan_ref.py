"""Serial Python restatement of the pre-graph global planner (dddmr_global_planner/src/a_star_on_pre_graph.cpp:
A_Star_on_PreGraph::getPath :191-289, getThetaFromParent2Expanding :133-157, AstarListPreGraph :41-104) with the
reference's containers -- a sorted set of (f, index) pairs and a dict of node records -- and exactly the expressions of
DESIGN.md 4d-4: float where the reference has float, double where it has double, nothing fused.

PINNED: a_star_on_pre_graph.cpp and static_graph.cpp compile unmodified against oracle/ref/shim/ (`make -C oracle ref`),
and tests/test_global_plan_pin_cpu.py holds plan() to those binaries on bits: path, status, every opened node's record,
the closed count, the final set size and theta (the assumptions are DESIGN.md 4d-4's G1-G6).  Two things
differ from the reference on purpose.  (1) The reference's theta is libm's acosf; the default here, like the device, is
the correctly rounded value (acos in double, rounded once), from which glibc 2.35's acosf differs by one float ulp for
about 7 % of arguments; `acosf=` takes libm's.  (2) A search that ends on a set emptied by discards returns NO_PATH here;
the reference reads begin() of the empty set there and has no defined answer (stat `ended_on_emptied_set`).

plan() takes the CSR arrays of static_layer_ref.build, the ground [n,3] float32, a dGraph [n+1] float64, the node weights
[n] float32 (or None) and cfg (config()).  `exp` and `acos` are the two libm calls in double and can be replaced, which
tests/test_global_plan_cpu.py uses to show that the committed cases do not hang on their last bits; `acosf`, a float to
float function over arrays, replaces the rounded double acos altogether."""
from __future__ import annotations

import heapq

import numpy as np

F = np.float32
D = np.float64
FOUND, NO_PATH, BUDGET, OPEN_FULL = 0, 1, 2, 3
NONE = 0xFFFFFFFF

# p2p_move_base_localization.yaml:254-255, :338-340
CFG = dict(turning_weight=0.1, a_star_expanding_radius=0.5, inscribed_radius=0.5, inflation_descending_rate=2.0,
           max_open_entries=1 << 20, max_expansions=1 << 17)


def config(**kw):
    c = dict(CFG)
    for k, v in kw.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


class SortedSet:
    """std::set<std::pair<float, unsigned>>: insert (equal pairs collapse), begin, erase.  A heap with lazy deletion under
    a set of the live pairs; a pair is a tuple (float(f), index), compared like std::pair."""

    def __init__(self):
        self.live = set()
        self.heap = []

    def insert(self, pair) -> bool:
        if pair in self.live:
            return False
        self.live.add(pair)
        heapq.heappush(self.heap, pair)
        return True

    def __len__(self):
        return len(self.live)

    def begin(self):
        while self.heap[0] not in self.live:
            heapq.heappop(self.heap)
        return self.heap[0]

    def erase(self, pair):
        self.live.remove(pair)

    def second(self):
        """the pair behind begin(), None without one (for the tie statistics only)"""
        first = self.begin()
        heapq.heappop(self.heap)
        nxt = None
        while self.heap:
            if self.heap[0] in self.live and self.heap[0] != first:
                nxt = self.heap[0]
                break
            heapq.heappop(self.heap)
        heapq.heappush(self.heap, first)
        return nxt


def dist(a, b) -> np.ndarray:
    """sqrt(pcl::geometry::squaredDistance(a, b)) in float: (dx*dx + dy*dy) + dz*dz"""
    d = np.asarray(a, F) - np.asarray(b, F)
    return np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F)).astype(F)


def cos_raw(vx1, vy1, vx2, vy2) -> np.ndarray:
    """:142: the float cosine before its clamp; NaN where a vector is zero"""
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(F(vx1 * vx1 + vy1 * vy1)).astype(F) * np.sqrt((vx2 * vx2 + vy2 * vy2).astype(F)).astype(F)
        return ((vx1 * vx2 + vy1 * vy2).astype(F) / den).astype(F)


def cos_theta(vx1, vy1, vx2, vy2) -> np.ndarray:
    """:142-144: the float cosine with its clamp; NaN where a vector is zero"""
    with np.errstate(invalid="ignore"):
        c = cos_raw(vx1, vy1, vx2, vy2)
        return np.where(np.abs(c) > F(1), F(1), c).astype(F)


def theta_rules(vx1, vy1, vx2, vy2, acos_double) -> np.ndarray:
    """:145-156 behind the acos: the float overload's value, here the double value rounded once (G3; a float32 array
    handed in is taken as acosf's own result)"""
    with np.errstate(invalid="ignore"):
        th = np.asarray(acos_double).astype(F).astype(D)
        zero = ((np.asarray(vx1) == 0) & (np.asarray(vy1) == 0)) | ((vx2 == 0) & (vy2 == 0)) | (vx_gap(vx1, vx2).astype(D) <= 0.0001)
        th = np.where(zero, 0.0, th)
        return np.where(np.abs(th) <= 0.345, 0.0, th)


def vx_gap(vx1, vx2) -> np.ndarray:
    """:150: fabsf(fabsf(vx1) - fabsf(vx2)), a float"""
    return np.abs(np.abs(F(vx1)) - np.abs(vx2)).astype(F)


def theta_many(xy, acosf=None) -> np.ndarray:
    """getThetaFromParent2Expanding for [n,6] float32 rows (parent x y, current x y, expanding x y) -> [n] float64;
    acosf as in plan()"""
    xy = np.asarray(xy, F).reshape(-1, 6)
    vx1, vy1 = (xy[:, 2] - xy[:, 0]).astype(F), (xy[:, 3] - xy[:, 1]).astype(F)
    vx2, vy2 = (xy[:, 4] - xy[:, 2]).astype(F), (xy[:, 5] - xy[:, 3]).astype(F)
    c = cos_theta(vx1, vy1, vx2, vy2)
    with np.errstate(invalid="ignore"):
        a = np.arccos(c.astype(D)) if acosf is None else np.asarray(acosf(c), F)
    return theta_rules(vx1, vy1, vx2, vy2, a)


def _steps(x, k):
    """the float k floats above (k > 0) or below x"""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def new_g(g, w, factor, theta, turning_weight, intensity) -> np.ndarray:
    """:245-246, left to right: the first sum in float, the others in double, the result a float"""
    gw = (F(g) + np.asarray(w, F)).astype(F)
    return (((gw.astype(D) + np.asarray(factor, D) * 1.0) + np.asarray(theta, D) * D(turning_weight)) + D(F(intensity))).astype(F)


def plan(graph, ground, dgraph, weights, cfg, start, goal, exp=np.exp, acos=np.arccos, stats=None, acosf=None) -> dict:
    """One getPath.  Returns status, path (uint32, start to goal; empty unless FOUND), n_expanded, n_pushed (the set's
    growth, the start's entry included), n_discarded_closed, g_goal, g / f / parent of every node the plan has opened,
    the closed nodes, set_size (what the set holds at the end) and ended_on_emptied_set.
    stats: a dict that collects what tests/helpers/global_plan_cases.check_cases asks of the cases."""
    row_start, neighbour, weight = graph["row_start"].astype(np.int64), graph["neighbour"], graph["weight"].astype(F)
    ground = np.asarray(ground, F)
    dgraph = np.asarray(dgraph, D)
    inten = np.zeros(len(ground), F) if weights is None else np.asarray(weights, F)
    tw, radius, inscribed, rate = D(cfg["turning_weight"]), D(cfg["a_star_expanding_radius"]), D(cfg["inscribed_radius"]), D(cfg["inflation_descending_rate"])
    start, goal = int(start), int(goal)
    st = stats if stats is not None else {}
    for k in ("tie_pops", "updates", "radius_skipped", "radius_equal_kept", "theta_above_cap", "theta_below_cap", "rows_over_256", "collapsed", "ended_on_emptied_set",
              "equal_g_not_filed", "popped_behind_discards", "dgraph_skipped", "dgraph_equal_kept",
              "theta_floats_below_cap", "theta_floats_above_cap", "vx_gap_floats_below", "vx_gap_floats_above", "cos_over_one", "zero_expanding_vector"):
        st.setdefault(k, 0)
    ended_on_emptied_set = False

    # Initial() (:41-50): every node neither opened nor closed; a record is (g, f, parent)
    rec, closed = {}, set()
    frontier = SortedSet()
    f0 = F(dist(ground[start], ground[goal]))                                 # :203
    rec[start] = (F(0), f0, start)                                            # :204
    frontier.insert((float(f0), start))
    n_expanded = n_discarded = 0
    n_pushed = 1
    status = NO_PATH

    while True:
        # getNode_wi_MinimumF (:74-92).  An empty frontier ends the search (:213), also behind discarded entries, where the
        # reference reads begin() of the empty set.
        if len(frontier) == 0:
            status = NO_PATH
            break
        if n_expanded >= cfg["max_expansions"]:
            status = BUDGET
            break
        first = frontier.begin()
        if stats is not None:
            nxt = frontier.second()
            if nxt is not None and nxt[0] == first[0]:
                st["tie_pops"] += 1
        cur = None
        if first[1] not in closed:
            frontier.erase(first)                                             # :78
            cur = first[1]
        else:
            while True:                                                       # :85-90
                frontier.erase(first)
                n_discarded += 1
                if len(frontier) == 0:
                    break
                first = frontier.begin()
                if first[1] not in closed:
                    cur = first[1]                                            # (its entry stays in the set)
                    st["popped_behind_discards"] += 1
                    break
            if cur is None:                                                   # :89 reads begin() of the empty set: undefined there
                status = NO_PATH
                ended_on_emptied_set = True
                st["ended_on_emptied_set"] += 1
                break
        g_cur, _, parent = rec[cur]                                           # current_node: a copy of the record at the pop

        b, e = row_start[cur], row_start[cur + 1]
        if e - b > 256:
            st["rows_over_256"] += 1
        nb, w = neighbour[b:e].astype(np.int64), weight[b:e]
        d = dgraph[nb]
        over = w.astype(D) > radius                                           # :222  float against double
        st["radius_skipped"] += int(over.sum())
        st["radius_equal_kept"] += int((w.astype(D) == radius).sum())
        keep = ~over & ~(d < inscribed)                                       # :229
        st["dgraph_skipped"] += int((~over & (d < inscribed)).sum())
        st["dgraph_equal_kept"] += int((~over & (d == inscribed)).sum())
        nb, w, d = nb[keep], w[keep], d[keep]
        before = len(frontier)
        if len(nb):
            pc, pp, pe = ground[cur], ground[parent], ground[nb]
            factor = np.asarray(exp(-1.0 * rate * (d - inscribed)), D)        # :240
            vx1, vy1 = F(pc[0] - pp[0]), F(pc[1] - pp[1])
            vx2, vy2 = (pe[:, 0] - pc[0]).astype(F), (pe[:, 1] - pc[1]).astype(F)
            c = cos_theta(vx1, vy1, vx2, vy2)
            with np.errstate(invalid="ignore"):
                a = np.asarray(acos(c.astype(D)), D) if acosf is None else np.asarray(acosf(c), F)
            theta = theta_rules(vx1, vy1, vx2, vy2, a)                        # :243
            if stats is not None:
                with np.errstate(invalid="ignore"):
                    raw = np.asarray(a).astype(F).astype(D)
                    st["theta_above_cap"] += int((theta > 0.345).sum())
                    live = ~((vx2 == 0) & (vy2 == 0)) & bool(vx1 != 0 or vy1 != 0) & (vx_gap(vx1, vx2).astype(D) > 0.0001)
                    st["theta_floats_below_cap"] += int((live & (raw <= 0.345) & (raw >= _steps(F(0.345), -16))).sum())
                    st["theta_floats_above_cap"] += int((live & (raw > 0.345) & (raw <= _steps(F(0.345), 16))).sum())
                    gap = vx_gap(vx1, vx2)
                    st["vx_gap_floats_below"] += int(((gap.astype(D) <= 0.0001) & (gap >= _steps(F(0.0001), -3))).sum())
                    st["vx_gap_floats_above"] += int(((gap.astype(D) > 0.0001) & (gap <= _steps(F(0.0001), 3))).sum())
                    st["cos_over_one"] += int((np.abs(cos_raw(vx1, vy1, vx2, vy2)) > F(1)).sum())
                    st["zero_expanding_vector"] += int(((vx2 == 0) & (vy2 == 0) & (nb != cur)).sum())
                    st["theta_below_cap"] += int(((raw > 0) & (raw <= 0.345) & ~((vx2 == 0) & (vy2 == 0)) & (vx1 != 0 or vy1 != 0)).sum())
            ng = new_g(g_cur, w, factor, theta, tw, inten[cur])               # :245
            nh = dist(pe, ground[goal])                                       # :248
            nf = (ng + nh).astype(F)                                          # :249
            for k in range(len(nb)):
                n = int(nb[k])
                if n in closed:                                               # :254
                    continue
                if n in rec:                                                  # :257  opened
                    if not (rec[n][0] > ng[k]):                               # :258
                        st["equal_g_not_filed"] += int(rec[n][0] == ng[k] and n != cur)
                        continue
                    st["updates"] += 1
                rec[n] = (ng[k], nf[k], cur)                                  # updateNode (:65-72)
                if not frontier.insert((float(nf[k]), n)):
                    st["collapsed"] += 1
        n_pushed += len(frontier) - before
        if len(frontier) > cfg["max_open_entries"]:
            status = OPEN_FULL
            break
        closed.add(cur)                                                       # :271
        n_expanded += 1
        if goal in closed:                                                    # :274
            status = FOUND
            break

    path = []
    if status == FOUND:                                                       # :276-282
        t = goal
        while rec[t][2] != t:
            path.append(t)
            t = rec[t][2]
        path.append(t)
        path.reverse()
    return dict(status=status, path=np.array(path, np.uint32), n_expanded=n_expanded, n_pushed=n_pushed, n_discarded_closed=n_discarded,
                g_goal=F(rec[goal][0]) if status == FOUND else F(0), g={k: v[0] for k, v in rec.items()}, parent={k: v[2] for k, v in rec.items()},
                f={k: v[1] for k, v in rec.items()}, closed=closed, set_size=len(frontier), ended_on_emptied_set=ended_on_emptied_set)


def nearest(ground, pts, radius=0.5) -> np.ndarray:
    """getStartGoalID's search (global_planner.cpp:407, :451): element 0 of radiusSearch(p, 0.5), brute force in float32;
    equal distances resolve to the lowest index (G5)"""
    ground, pts = np.asarray(ground, F), np.asarray(pts, F).reshape(-1, 3)
    out = np.full(len(pts), NONE, np.uint32)
    r2 = F(D(radius) * D(radius))
    for i, p in enumerate(pts):
        d = ground - p
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
        j = int(np.argmin(d2))                                                # (argmin: the first of equals)
        if d2[j] < r2:
            out[i] = j
    return out


def probe(ground, dgraph, pts, inscribed_radius, radius=0.25):
    """determineDWAPlan's goal test (dynamic_window_aware_global_planner.cpp:248-270) -> (count, blocked)"""
    ground, pts = np.asarray(ground, F), np.asarray(pts, F).reshape(-1, 3)
    r2 = F(D(radius) * D(radius))
    cnt, blocked = np.zeros(len(pts), np.uint32), np.zeros(len(pts), bool)
    for i, p in enumerate(pts):
        d = ground - p
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
        inside = d2 < r2
        cnt[i] = int(inside.sum())
        blocked[i] = bool((np.asarray(dgraph, D)[: len(ground)][inside] < D(inscribed_radius)).any())
    return cnt, blocked


def dijkstra_cost(graph, ground, dgraph, cfg, start, goal) -> float:
    """An independent best-first search in double for turning_weight 0 and zero weights: the cost of the cheapest path, inf
    without one.  Written apart from plan(): a plain heap, no records, the heuristic only orders."""
    rs, nbr, wt = graph["row_start"].astype(np.int64), graph["neighbour"], graph["weight"].astype(D)
    gp = np.asarray(ground, D)
    best = {int(start): 0.0}
    heap = [(float(np.linalg.norm(gp[start] - gp[goal])), 0.0, int(start))]
    done = set()
    while heap:
        _, g, u = heapq.heappop(heap)
        if u in done:
            continue
        done.add(u)
        if u == goal:
            return g
        for j in range(rs[u], rs[u + 1]):
            v, w = int(nbr[j]), float(wt[j])
            if w > cfg["a_star_expanding_radius"] or dgraph[v] < cfg["inscribed_radius"] or v in done:
                continue
            c = g + w + float(np.exp(-cfg["inflation_descending_rate"] * (dgraph[v] - cfg["inscribed_radius"])))
            if c < best.get(v, np.inf):
                best[v] = c
                heapq.heappush(heap, (c + float(np.linalg.norm(gp[v] - gp[goal])), c, v))
    return float("inf")
