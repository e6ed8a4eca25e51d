"""What keeps tests/test_point_grid_gpu.py from passing vacuously, checked on the reference alone (tests/helpers/
point_grid_ref.py on the cases of tests/helpers/point_grid_cases.py), and the argument of the search pads.  No GPU.

(a) containment: every point brute force finds inside the radius lies in the query's box of cells -- the grid's
    exactness claim holds on these inputs, so "the walk saw the box population" implies "the walk saw every neighbour";
(b) each case exercises what it is for: enough queries with and without a neighbour, each walk form it names at least 8
    times, ties and points at exactly the radius in the tie case, differing boxes under the historic defect's formula
    in the shifted case, clamped points in the boxed ones, a 4 x 4 x 2 grid in the coarsened one;
(c) the pads.  Three roundings stand between a neighbour and its cell range ((q - origin), (...) + r_box, p - origin),
    and a neighbour can be lost only when p - q > r_box - ulp / 2, ulp that of extent + r_box.  So a pad is safe while it
    is at least half that ulp: 1e-4 m (marking and depth layers) below 2048 m, 1e-3 m (localiser, static layer, planners)
    far past their 4096 m limit.  The search below looks for a lost neighbour at pad 1e-4 with the radii those layers use
    around the cell boundaries next to 1024, 2048 and 4096 m from the origin and in between: it finds them from 2048 m
    on (one is kept as a known answer) and none below, which is why the layers refuse a static cloud wider than
    kSmallPadMaxExtent = 2000 m."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import point_grid_cases as cases  # noqa: E402
import point_grid_ref as R  # noqa: E402

F = np.float32
CASES = {c.name: c for c in cases.cases()}
DESIGNED = [CASES[n] for n in cases.DESIGNED]


@pytest.mark.parametrize("case", [c for c in CASES.values() if c.name != "lost neighbour"], ids=lambda c: c.name)
def test_every_neighbour_lies_in_the_box_of_cells(case):
    e = cases.expected(case)
    assert len(case.queries) <= (704 if case.name == "shifted" else 512) and len(case.pts) <= 20000      # (shifted: 192 edge queries more)
    missed = e["brute"]["inside"] & ~e["box"]["member"]
    assert int(missed.sum()) == 0
    assert np.array_equal(e["brute"]["count"], (e["box"]["member"] & e["brute"]["inside"]).sum(axis=1))
    below = e["brute"]["min_d2"] < case.r2                                   # where a neighbour exists the box holds the nearest
    assert np.array_equal(e["brute"]["min_d2"][below], e["box"]["min_d2"][below])


@pytest.mark.parametrize("case", DESIGNED, ids=lambda c: c.name)
def test_case_exercises_what_it_is_for(case):
    e = cases.expected(case)
    has = e["brute"]["count"] > 0
    m = len(case.queries)
    assert has.sum() * 3 >= m, f"{has.sum()} of {m} queries have a neighbour"
    assert (~has).sum() * 8 >= m, f"{(~has).sum()} of {m} queries have none"
    seen = [cases.form_of(int(a), int(b)) for a, b in e["forms"]]
    for form in case.forms:
        assert seen.count(form) >= 8, f"walk form {form}: {seen.count(form)} queries"
    assert (e["brute"]["count"] > 1).sum() >= 8                              # the early return has something to cut short
    if case.name in ("wide", "extent", "ties"):
        assert (e["brute"]["count"] > 2).sum() >= 8


def test_tie_case_has_ties_and_points_at_exactly_the_radius():
    case = CASES["ties"]
    b = cases.expected(case)["brute"]
    shared = ((b["d2"] == b["id_d2"][:, None]) & b["inside"]).sum(axis=1)
    assert (shared >= 2).sum() >= 32
    at_radius = (b["d2"] == case.r2).any(axis=1)
    assert at_radius.sum() >= 32
    assert (at_radius & (b["id"] == R.GRID_NONE)).sum() >= 32                # ... of which these have nothing nearer: "none", not a hit


def test_shifted_case_tells_the_late_origin_formula():
    """(q + d) - origin, the defect the history found by soak, walks other cells than (q - origin) + d on these queries"""
    case = CASES["shifted"]
    e = cases.expected(case)
    late = R.box_population(e["grid"], case.pts, case.queries, case.r_box, edge=lambda g, a, q, d: R.cell2_late_origin(g, a, q, d))
    differs = (late["visited"] != e["box"]["visited"]) | (late["sum"] != e["box"]["sum"]) | (late["xor"] != e["box"]["xor"])
    assert differs.sum() >= 8
    room = cases.expected(CASES["room"])                                      # ... and near the origin the two agree
    late0 = R.box_population(room["grid"], CASES["room"].pts, CASES["room"].queries, CASES["room"].r_box,
                             edge=lambda g, a, q, d: R.cell2_late_origin(g, a, q, d))
    assert (late0["visited"] != room["box"]["visited"]).sum() <= differs.sum() // 4


def test_grids_have_the_designed_shapes():
    g = cases.expected(CASES["coarsened"])["grid"]
    assert (g.nx, g.ny, g.nz) == (4, 4, 2)
    assert not np.isclose(1.0 / float(g.inv_xy), 0.25 * 1.3, rtol=0.2)            # several 1.3 steps, not one
    assert cases.expected(CASES["flat"])["grid"].nz == 2 and cases.expected(CASES["room"])["grid"].nz == 9
    g = cases.expected(CASES["extent"])["grid"]
    assert g.nx * g.ny * g.nz <= cases.CAP and float(g.inv_xy) < 0.5             # coarsened at scale too
    assert float(CASES["extent"].hi[0] - CASES["extent"].lo[0]) == 4090.0
    for name in ("boxed", "boxed, half a metre in z"):
        c = CASES[name]
        outside = ((c.pts < c.lo) | (c.pts > c.hi)).any(axis=1)
        assert outside.sum() * 5 >= len(c.pts)                                  # a fifth at least is clamped into edge cells
        sides = np.sign(c.queries[:, :2] - c.lo[:2]) * np.sign(c.hi[:2] - c.queries[:, :2])
        assert (sides < 0).any(axis=1).sum() >= 64 and (sides > 0).all(axis=1).sum() >= 64


# ---- (c) the pads ------------------------------------------------------------------------------------------------------
def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


def _search(r, cell, pad, span, n_origins, seed, around=None):
    """Triples (origin, q, p) on one axis, y and z equal: p' = p - origin next to a cell boundary (the first float of a
    cell for the box's upper edge, the last float of the cell below for its lower edge; p up to half an ulp of p' off, so
    that the subtraction rounds onto it), q at every float within +-4 of p -+ r.  The grids are grid_shape's over a box
    `span` long and up to as wide, coarsened under 2^22 cells as the static grids are.  Boundaries: those within r + 1 m
    of `around` metres from the origin, or 24 random ones of the far half.  -> (triples tried, the lost ones)."""
    rng = np.random.default_rng(seed)
    O, INV, K = [], [], []
    for _ in range(n_origins):
        extent = rng.uniform(*span)
        o = F(-extent * rng.uniform(0.0, 1.0))
        g = R.grid_shape([o, 0.0, 0.0], [F(o + F(extent)), F(extent * rng.uniform(0.02, 1.0)), 2.0], cell, cell, 1 << 22)
        inv = float(g.inv_xy)
        if around is None:
            ks = rng.integers(g.nx // 2, g.nx - 1, 24)
        else:
            ks = np.arange(int((around - r - 1.0) * inv), int((around + r + 1.0) * inv) + 1)
        O += [o] * len(ks)
        INV += [g.inv_xy] * len(ks)
        K += list(ks)
    o, inv, k = np.array(O, F), np.array(INV, F), np.array(K, np.float64)
    r_box, r2 = F(F(r) + F(pad)), F(float(r) * float(r))
    first = (k / inv.astype(np.float64)).astype(F)                           # -> the smallest float whose cell is k
    for _ in range(3):
        first = np.where(np.floor(first * inv) < k, np.nextafter(first, F(np.inf)), first)
    for _ in range(3):
        down = np.nextafter(first, F(-np.inf))
        first = np.where(np.floor(down * inv) >= k, down, first)
    assert (np.floor(first * inv) == k).all() and (np.floor(np.nextafter(first, F(-np.inf)) * inv) == k - 1).all()
    ulp = np.spacing(first).astype(np.float64)
    tried, lost = 0, []
    for side in (1, -1):
        target = first if side > 0 else np.nextafter(first, F(-np.inf))
        for half in (0.0, 0.25, 0.5):
            centre = (o.astype(np.float64) + target.astype(np.float64) - side * half * ulp).astype(F)
            for dp in (-1, 0, 1):
                p = _step(centre, dp)
                q0 = (p - F(side) * F(r)).astype(F)
                for dq in range(-4, 5):
                    q = _step(q0, dq)
                    dx = p - q
                    inside = dx * dx < r2
                    cell_p = np.floor((p - o) * inv)
                    edge = np.floor(((q - o) + F(side) * r_box) * inv)
                    miss = inside & ((cell_p > edge) if side > 0 else (cell_p < edge))
                    tried += p.size
                    lost += [(float(o[i]), float(q[i]), float(p[i]), float(inv[i])) for i in np.nonzero(miss)[0]]
    return tried, lost


def _layer_radii():
    from dddmr_navigation_amd import depth_layer, marking
    mk, dl = marking.shipped_config(), depth_layer.shipped_config()
    return sorted({0.05, 0.1, 0.01, float(mk.xy_resolution), float(mk.euclidean_cluster_extraction_tolerance), float(mk.inflation_radius),
                   float(dl.euclidean_cluster_extraction_tolerance), float(dl.inflation_radius)})


def test_search_for_a_lost_neighbour():
    """about 10^7 triples at pad 1e-4: lost neighbours exist from 2048 m on, none below; none at all at pad 1e-3"""
    radii = _layer_radii()
    assert radii == [0.01, 0.05, 0.1, 1.5]
    total, below, beyond, big_pad = 0, [], [], []
    for r in radii:
        for cell in (0.25, 0.5):
            for around, span in ((1024.0, (1100.0, 2000.0)), (None, (1024.0, 2000.0)), (2000.0 - r - 1.0, (2000.0, 2000.0))):
                t, lost = _search(r, cell, 1e-4, span, 100, 21, around)
                total, below = total + t, below + lost
            for around, span in ((2048.0, (2100.0, 4096.0)), (4096.0, (4200.0, 8192.0)), (None, (2048.0, 8192.0))):
                t, lost = _search(r, cell, 1e-4, span, 100, 22, around)
                total, beyond = total + t, beyond + lost
                t, lost = _search(r, cell, 1e-3, span, 100, 22, around)
                total, big_pad = total + t, big_pad + lost
    print(f"{total} triples; lost below 2000 m: {len(below)}, from 2048 m on: {len(beyond)}, at pad 1e-3: {len(big_pad)}")
    assert 5e6 <= total <= 3e7
    assert not below, below[:3]
    assert not big_pad, big_pad[:3]
    assert beyond, "the search no longer finds what it found: lost neighbours past 2048 m at pad 1e-4"
    assert min(float(F(p) - F(o)) for o, q, p, inv in beyond) >= 2047.0


def test_known_lost_neighbour():
    """the kept triple: inside the radius by FLANN's rule, outside the box of cells at pad 1e-4, inside it at pad 1e-3"""
    case = CASES["lost neighbour"]
    e = cases.expected(case)
    assert float(case.hi[0] - case.lo[0]) > 2048.0 and (e["grid"].nx, float(e["grid"].inv_xy)) == (4101, 2.0)
    assert e["brute"]["inside"][0, 0] and not e["box"]["member"][0, 0]
    assert int(R.cell1(e["grid"], 0, case.pts[0, 0])) == 4095 and int(R.query_box(e["grid"], case.queries[:1], case.r_box)[0, 0]) == 4096
    assert e["brute"]["count"][0] == (e["box"]["member"][0] & e["brute"]["inside"][0]).sum() + 1
    wide = cases.lost_neighbour_case(pad=cases.MCL_PAD)
    assert R.box_members(e["grid"], wide.pts, wide.queries, wide.r_box)[0, 0]


def test_half_ulp_rule_on_the_extents_the_layers_accept():
    """pad >= ulp(extent + r_box) / 2 for every extent a layer accepts and every box half width it may search with"""
    src = open(os.path.join(ROOT, "dddmr_navigation_amd", "csrc", "point_grid_plan.hip.h")).read()
    small = float(re.search(r"constexpr float kSmallPadMaxExtent = ([0-9.]+)f;", src).group(1))
    cloud = float(re.search(r"constexpr float kCloudMaxExtent = ([0-9.]+)f;", src).group(1))
    assert (small, cloud) == (2000.0, 4096.0)
    widest = 48.0                                                            # a box half width below this has room under either limit
    assert max(_layer_radii()) + 1e-4 < widest
    assert float(np.spacing(np.nextafter(F(small + widest), F(0)))) / 2 <= float(F(1e-4))
    assert float(np.spacing(np.nextafter(F(2048.0), F(0)))) / 2 <= float(F(1e-4)) < float(np.spacing(F(2048.0))) / 2
    assert float(np.spacing(np.nextafter(F(cloud + widest), F(0)))) / 2 <= float(F(1e-3))
    src = open(os.path.join(ROOT, "dddmr_navigation_amd", "csrc", "marking_host.hip.h")).read()
    assert "small_pad_extent_ok(h.lo, h.hi)" in src                           # upload_static: both layers' static clouds pass through it
