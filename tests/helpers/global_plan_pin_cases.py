"""Cases of the planner pin (tests/test_global_plan_pin_cpu.py): CSR graphs built by hand, CPU only, 2 to 400 nodes, aimed
at the places where tests/helpers/global_plan_ref.py could differ from a_star_on_pre_graph.cpp, and random geometric
graphs.  Hand-built graphs cannot reach the device (the static layer builds its own rows), so these hold the restatement
alone; the device is held to the cloud cases' goldens (tests/test_global_plan_pin_gpu.py).

A pin case is a dict: name, ground [n,3] f32, intensity [n] f32 or None, row_start / neighbour / weight (CSR; a row sorted
by (neighbour, weight), which is std::set<std::pair<unsigned, float>>'s order), order (a shuffled permutation: the order in
which the edges reach StaticGraph::insertNode, so that the rows' order is the set's own -- G6), dgraph [n+1] f64, cfg,
start, goal.  An edge's weight is whatever the case says: the reference takes weights from the graph and the heuristic
from the cloud, so they need not agree.

Every condition a case is built for is asserted here from the restatement's own stats (check()), never from the reference.
A query whose search ends on a set emptied by discards (the reference reads begin() of the empty set there) is flagged
by the restatement and left out of every comparison; check() bounds how many those are."""
from __future__ import annotations

import functools

import numpy as np

import global_plan_cases as Cs
import global_plan_ref as G

F = np.float32
D = np.float64
FAR = Cs.STACK_START


def up(x, k=1):
    """k floats (float32 x) or doubles (float64 x) above x; below for k < 0"""
    x = np.asarray(x)
    inf = x.dtype.type(np.inf if k > 0 else -np.inf)
    for _ in range(abs(k)):
        x = np.nextafter(x, inf)
    return x[()]


def make(name, ground, edges, start, goal, dgraph=None, intensity=None, seed=0, **cfg) -> dict:
    """edges: (a, b, w) directed; duplicates of (a, b, w) collapse as in the set"""
    ground = np.asarray(ground, F).reshape(-1, 3)
    n = len(ground)
    rows = sorted({(int(a), int(b), float(F(w))) for a, b, w in edges})
    src = np.array([r[0] for r in rows], np.int64)
    row_start = np.zeros(n + 1, np.uint32)
    row_start[1:] = np.cumsum(np.bincount(src, minlength=n))
    dg = np.full(n + 1, FAR, D) if dgraph is None else np.asarray(dgraph, D)
    assert len(dg) == n + 1
    return dict(name=name, ground=ground, intensity=None if intensity is None else np.asarray(intensity, F), row_start=row_start,
                neighbour=np.array([r[1] for r in rows], np.uint32), weight=np.array([r[2] for r in rows], F),
                order=np.random.default_rng(1000 + seed).permutation(len(rows)).astype(np.uint32), dgraph=dg,
                cfg=G.config(**cfg), start=int(start), goal=int(goal))


def both(pairs):
    return [(a, b, w) for a, b, w in pairs] + [(b, a, w) for a, b, w in pairs]


def run(case, stats=None, **kw) -> dict:
    return G.plan(case, case["ground"], case["dgraph"], case["intensity"], case["cfg"], case["start"], case["goal"], stats=stats, **kw)


def from_query(q) -> dict:
    """a committed query (global_plan_cases) as a pin case, its rows static_layer_ref.build's"""
    c, g = Cs.case(q[1]), Cs.static_ref(q[1])
    return dict(name=q[0], ground=c["ground"], intensity=c["weights"] if q[5] else None, row_start=g["row_start"], neighbour=g["neighbour"],
                weight=g["weight"], order=np.random.default_rng(7).permutation(len(g["neighbour"])).astype(np.uint32), dgraph=c["dgraph"],
                cfg=Cs.plan_cfg(q), start=q[2], goal=q[3])


# ---- hand-built cases: name -> (case, the stats that must be positive) ----
def _fan(name, mids, goal_xy=(3.0, 0.0), **kw):
    """0 -> 1 (the parent vector), 1 -> every mid node, every mid node -> the goal (the last node)"""
    mids = np.asarray(mids, F).reshape(-1, 2)
    k = len(mids)
    ground = np.zeros((k + 3, 3), F)
    ground[1, :2] = kw.pop("current", (1.0, 0.0))
    ground[2: 2 + k, :2] = mids
    ground[-1, :2] = goal_xy
    e = [(0, 1, 0.3)] + [(1, 2 + i, 0.3) for i in range(k)] + [(2 + i, k + 2, 0.3) for i in range(k)]
    return make(name, ground, e, 0, k + 2, **kw)


def _theta_near_cap():
    """expanding points whose float theta lies beside 0.345 (found by a scan of the angle).  Theta is the acos of a float
    cosine near 0.941, whose floats lie 6e-8 apart: that is 1.8e-7 in theta, six floats of theta, so only every sixth float
    beside the cap can occur at all.  The case holds the three nearest that do on either side (within 16 floats)."""
    hit = {}
    a = np.linspace(0.345 - 6e-7, 0.345 + 6e-7, 6001)
    for r in (0.4, 0.45):
        xy = np.zeros((len(a), 6), F)
        xy[:, 2] = 1.0
        xy[:, 4], xy[:, 5] = F(1.0) + (r * np.cos(a)).astype(F), (r * np.sin(a)).astype(F)
        vx2, vy2 = (xy[:, 4] - xy[:, 2]).astype(F), xy[:, 5]
        th = np.arccos(G.cos_theta(F(1.0), F(0.0), vx2, vy2).astype(D)).astype(F)
        for i, t in enumerate(th.tolist()):
            if float(G._steps(F(0.345), -16)) <= t <= float(G._steps(F(0.345), 16)):
                hit.setdefault(t, xy[i, 4:6].copy())
    assert sum(t <= 0.345 for t in hit) >= 2 and sum(t > 0.345 for t in hit) >= 2, sorted(hit)
    return _fan("theta-near-cap", np.array(list(hit.values())), turning_weight=5.0)


def _vx_gap_near():
    """fabsf(fabsf(vx1) - fabsf(vx2)) one to three floats either side of 0.0001 and on it, at a turn well above the cap:
    current x = 0.0002, expanding x = e beside 0.0001, so vx2 = e - 0.0002 and the gap 0.0002 - (0.0002 - e) = e, both exact"""
    cx = F(0.0002)
    want = {float(G._steps(F(0.0001), k)) for k in range(-3, 4)}
    hit = {}
    for k in range(-3, 4):
        e = G._steps(F(0.0001), k)
        gap = float(G.vx_gap(cx, np.array([e - cx], F))[0])
        if gap in want:
            hit.setdefault(gap, (e, F(0.35)))
    assert len(hit) == 7, sorted(hit)
    return _fan("vx-gap-near", np.array(list(hit.values()), F), current=(float(cx), 0.0), turning_weight=5.0)


def _cos_over_one():
    """collinear vectors whose float cosine rounds above 1 (found by a scan)"""
    rng = np.random.default_rng(5)
    mids, cur = [], None
    for _ in range(4000):
        v = rng.uniform(0.05, 0.9, 2).astype(F)
        k = F(rng.uniform(0.2, 0.5))
        vx2, vy2 = np.array([v[0] * k], F), np.array([v[1] * k], F)
        if abs(float(G.cos_raw(v[0], v[1], vx2, vy2)[0])) > 1.0:
            cur = v
            # (the expanding point is current + v2 in float: the vector read back must still give a cosine over 1)
            e = (v + np.array([vx2[0], vy2[0]], F)).astype(F)
            if abs(float(G.cos_raw(v[0], v[1], np.array([e[0] - v[0]], F), np.array([e[1] - v[1]], F))[0])) > 1.0:
                mids.append(e)
                break
    assert mids, "no cosine over 1 found"
    return _fan("cos-over-one", np.array(mids), current=tuple(float(x) for x in cur), turning_weight=5.0)


def _lattice(name, k=6, shift=(0.0, 0.0, 0.0), reach=0.26, **kw):
    """an exact 0.25 m lattice of k x k nodes with edges to the 4 neighbours (reach 0.36: 8) and to itself, far from every
    obstacle: the factor underflows to 0; with 4 neighbours every g is exact and mirrored nodes have equal f"""
    xs, ys = np.meshgrid(np.arange(k) * 0.25, np.arange(k) * 0.25, indexing="ij")
    ground = (np.stack([xs.ravel(), ys.ravel(), np.zeros(k * k)], axis=1) + np.asarray(shift)).astype(F)
    e = []
    for i in range(k * k):
        for j in range(k * k):
            d = float(G.dist(ground[i], ground[j]))
            if d <= reach:
                e.append((i, j, d))
    return make(name, ground, e, 0, k * k - 1, **kw)


def _diamond(name, w13, w23, ground=None, **kw):
    """0 -> 1, 2 (equal weights: 1 pops first on the index), 1 -> 3, 2 -> 3, 3 -> 4, 4 -> 5 (the goal)"""
    g = np.zeros((6, 3), F) if ground is None else ground
    return make(name, g, [(0, 1, 0.3), (0, 2, 0.3), (1, 3, w13), (2, 3, w23), (3, 4, 0.3), (4, 5, 0.3)], 0, 5, **kw)


@functools.lru_cache(maxsize=None)
def hand_built() -> dict:
    """name -> (case, tuple of stats that must be positive in the restatement's run)"""
    out = {}

    def add(case, *needs):
        assert case["name"] not in out
        out[case["name"]] = (case, needs)

    g5 = np.array([[0, 0, 0], [0.3, 0.1, 0], [0.3, 0, 0], [0.3, -0.1, 0], [0.6, 0, 0]], F)
    half = F(0.5)
    add(make("radius-0.5", g5, [(0, 1, up(half, -1)), (0, 2, half), (0, 3, up(half)), (1, 4, 0.3), (2, 4, 0.3), (3, 4, 0.3)], 0, 4),
        "radius_skipped", "radius_equal_kept")
    # 0.3 is no float: float(0.3) widened is above the double 0.3 and is skipped, the float below is kept
    add(make("radius-0.3", g5, [(0, 1, up(F(0.3), -1)), (0, 2, F(0.3)), (0, 3, up(F(0.3))), (1, 4, 0.2), (2, 4, 0.2), (3, 4, 0.2)], 0, 4,
             a_star_expanding_radius=0.3), "radius_skipped")
    dg = np.array([FAR, up(D(0.5), -1), 0.5, up(D(0.5)), FAR, FAR])
    add(make("dgraph-0.5", g5, [(0, 1, 0.3), (0, 2, 0.3), (0, 3, 0.3), (1, 4, 0.3), (2, 4, 0.3), (3, 4, 0.3)], 0, 4, dgraph=dg),
        "dgraph_skipped", "dgraph_equal_kept")
    dg = np.array([FAR, up(D(0.35), -1), 0.35, up(D(0.35)), FAR, FAR])
    add(make("dgraph-0.35", g5, [(0, 1, 0.3), (0, 2, 0.3), (0, 3, 0.3), (1, 4, 0.3), (2, 4, 0.3), (3, 4, 0.3)], 0, 4, dgraph=dg,
             inscribed_radius=0.35, inflation_descending_rate=10.0), "dgraph_skipped", "dgraph_equal_kept")
    add(_theta_near_cap(), "theta_floats_below_cap", "theta_floats_above_cap")
    add(_vx_gap_near(), "vx_gap_floats_below", "vx_gap_floats_above")
    add(_cos_over_one(), "cos_over_one")
    # two nodes at the same x and y: a zero expanding vector
    gz = np.array([[0, 0, 0], [0.3, 0, 0], [0.3, 0, 0.2], [0.6, 0, 0.2]], F)
    add(make("zero-expanding", gz, both([(0, 1, 0.3), (1, 2, 0.2), (2, 3, 0.3)]), 0, 3, turning_weight=5.0), "zero_expanding_vector")
    add(_lattice("lattice-ties", turning_weight=0.0), "tie_pops", "equal_g_not_filed")
    add(_lattice("lattice-turning", reach=0.36, turning_weight=5.0, inflation_descending_rate=0.5), "updates")
    add(_lattice("lattice-shifted", shift=(4000.25, -3000.5, 100.0), turning_weight=0.1), "tie_pops", "theta_above_cap")
    # the goal 4 km away: an update that lowers g by one float leaves f's bits as they were, and the set collapses it
    far = np.zeros((6, 3), F)
    far[5] = (4000.0, 0.0, 0.0)
    far[4] = (3999.7, 0.0, 0.0)
    add(_diamond("update-same-f", up(F(0.3), 4), F(0.3), ground=far, turning_weight=0.0), "updates", "collapsed")
    # 3's first entry outlives its pop; behind it 4 is reached, and behind 4's own entry the goal
    add(_diamond("popped-behind-discards", 0.45, 0.3, turning_weight=0.0), "updates", "popped_behind_discards")
    add(_diamond("equal-g", 0.3, 0.3, turning_weight=0.0), "equal_g_not_filed")
    chain = np.array([[0.3 * i, 0, 0] for i in range(5)], F)
    ce = both([(i, i + 1, 0.3) for i in range(4)]) + [(i, i, 0.0) for i in range(5)]
    add(make("start-is-goal", chain, ce, 2, 2))
    dl = np.full(6, FAR)
    dl[0] = 0.1
    add(make("start-lethal", chain, ce, 0, 4, dgraph=dl), "dgraph_skipped")
    dl = np.full(6, FAR)
    dl[4] = 0.1
    add(make("goal-lethal", chain, ce, 0, 4, dgraph=dl), "dgraph_skipped")
    add(make("two-nodes", chain[:2], [(0, 1, 0.3)], 0, 1))
    add(make("no-edge", chain[:2], [], 0, 1))
    for lab, inten in (("intensity-0", 0.0), ("intensity-0.3", 0.3), ("intensity-1e-8", 1e-8)):
        add(make(lab, chain, ce, 0, 4, intensity=np.full(5, inten, F), dgraph=np.full(6, 0.9)))
    # a row of 300 successors
    rng = np.random.default_rng(11)
    star = np.zeros((302, 3), F)
    ang = rng.uniform(0, 2 * np.pi, 300)
    rad = rng.uniform(0.1, 0.49, 300)
    star[1:301, 0], star[1:301, 1] = rad * np.cos(ang), rad * np.sin(ang)
    star[301] = (0.9, 0.0, 0.0)
    se = [(0, i, float(G.dist(star[0], star[i]))) for i in range(1, 301)] + [(i, 301, float(G.dist(star[i], star[301]))) for i in range(1, 301)]
    add(make("row-of-300", star, both(se), 1, 301, dgraph=np.concatenate([rng.uniform(0.4, 3.0, 302), [FAR]]), a_star_expanding_radius=1.0),
        "rows_over_256", "dgraph_skipped")
    return out


# ---- random geometric graphs ----
CONFIGS = (dict(turning_weight=0.0, inflation_descending_rate=0.5), dict(turning_weight=0.1, inflation_descending_rate=2.0),
           dict(turning_weight=5.0, inflation_descending_rate=10.0), dict(turning_weight=0.1, inflation_descending_rate=2.0, a_star_expanding_radius=0.7,
                                                                          inscribed_radius=0.3))
N_GRAPHS, QUERIES_PER_GRAPH = 104, 10


@functools.lru_cache(maxsize=None)
def random_graph(i: int):
    """graph i: up to 300 points on a square whose side sets the density (sparse squares fall apart into components), edges
    between points within 0.75 m, a dGraph from a few random obstacle points, random intensities on every other graph;
    every fourth graph lies kilometres from the origin"""
    rng = np.random.default_rng(5000 + i)
    n = int(rng.integers(12, 301))
    side = float(np.sqrt(n) * rng.uniform(0.22, 0.7))
    shift = np.array([rng.uniform(-6000, 6000), rng.uniform(-6000, 6000), rng.uniform(-50, 50)]) if i % 4 == 3 else np.zeros(3)
    ground = (np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n), rng.uniform(0, 0.1, n)], axis=1) + shift).astype(F)
    obstacles = np.stack([rng.uniform(0, side, 3), rng.uniform(0, side, 3)], axis=1) + shift[:2]
    d = np.min(np.hypot(ground[:, None, 0].astype(D) - obstacles[None, :, 0], ground[:, None, 1].astype(D) - obstacles[None, :, 1]), axis=1)
    if i % 3 == 0:
        d = np.full(n, FAR)
    e = [(a, a, 0.0) for a in range(n)]
    for a in range(n):
        w = G.dist(ground[a], ground)
        for b in np.flatnonzero(w <= F(0.75)):
            if b != a:
                e.append((a, int(b), float(w[b])))
    inten = rng.uniform(0, 0.3, n).astype(F) if i % 2 else None
    return ground, e, np.concatenate([d, [FAR]]), inten


@functools.lru_cache(maxsize=None)
def random_cases() -> tuple:
    out = []
    for i in range(N_GRAPHS):
        ground, e, dg, inten = random_graph(i)
        rng = np.random.default_rng(9000 + i)
        base = make(f"random-{i}", ground, e, 0, 0, dgraph=dg, intensity=inten, seed=i, **CONFIGS[i % 4])
        for k in range(QUERIES_PER_GRAPH):
            c = dict(base)
            c["name"] = f"random-{i}-{k}"
            c["start"], c["goal"] = (int(x) for x in rng.integers(0, len(ground), 2))
            out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def restated(name: str) -> dict:
    """the restatement's default run of a pin case (hand-built or random), with its stats; computed once, not to be written"""
    case = all_cases()[name]
    st = {}
    out = run(case, stats=st)
    out["stats"] = st
    return out


@functools.lru_cache(maxsize=None)
def all_cases() -> dict:
    d = {k: v[0] for k, v in hand_built().items()}
    d.update({c["name"]: c for c in random_cases()})
    return d


def check() -> dict:
    """what the pin's cases must hold, from the restatement alone -> the counts found"""
    for name, (case, needs) in hand_built().items():
        n = len(case["ground"])
        assert 2 <= n <= 400, name
        r = restated(name)
        assert not r["ended_on_emptied_set"], name
        for k in needs:
            assert r["stats"][k] > 0, (name, k, r["stats"])
    h = {k: restated(k) for k in hand_built()}
    assert 2 in h["radius-0.5"]["g"] and 1 in h["radius-0.5"]["g"] and 3 not in h["radius-0.5"]["g"]        # equal is kept
    assert 1 in h["radius-0.3"]["g"] and 2 not in h["radius-0.3"]["g"]
    for k in ("dgraph-0.5", "dgraph-0.35"):
        assert 2 in h[k]["g"] and 3 in h[k]["g"] and 1 not in h[k]["g"], k                                   # equal is kept
    assert h["start-is-goal"]["status"] == G.FOUND and h["start-is-goal"]["path"].tolist() == [2]
    assert h["start-lethal"]["status"] == G.FOUND and h["goal-lethal"]["status"] == G.NO_PATH and h["no-edge"]["status"] == G.NO_PATH
    assert h["update-same-f"]["set_size"] == 0 and h["popped-behind-discards"]["set_size"] == 1
    bits = {k: F(h[k]["g_goal"]).view(np.uint32) for k in ("intensity-0", "intensity-0.3", "intensity-1e-8")}
    assert bits["intensity-0"] == bits["intensity-1e-8"] != bits["intensity-0.3"]                             # 1e-8 is lost in the float sum
    found = dict(queries=0, found=0, no_path=0, no_path_defined=0, no_path_on_emptied_set=0, popped_behind_discards=0, updates=0, collapsed=0,
                 tie_pops=0)
    for c in random_cases():
        assert len(c["ground"]) <= 300
        r = restated(c["name"])
        found["queries"] += 1
        found["found"] += r["status"] == G.FOUND
        found["no_path"] += r["status"] == G.NO_PATH
        found["no_path_defined"] += r["status"] == G.NO_PATH and not r["ended_on_emptied_set"]
        found["no_path_on_emptied_set"] += bool(r["ended_on_emptied_set"])
        for k in ("popped_behind_discards", "updates", "collapsed", "tie_pops"):
            found[k] += r["stats"][k]
    assert found["queries"] >= 1000 and found["found"] >= 300, found
    assert found["no_path_defined"] >= 50 and 2 * found["no_path_on_emptied_set"] <= found["no_path"], found
    assert found["popped_behind_discards"] > 0 and found["updates"] > 0, found
    return found
