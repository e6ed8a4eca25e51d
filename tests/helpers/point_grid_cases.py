"""The designed inputs of tests/test_point_grid_cpu.py and tests/test_point_grid_gpu.py: point sets, the box and cell
sizes of their grid, and queries, one case per class of input the walks of csrc/point_grid.hip.h can go wrong on.  Fixed
seeds; everything is float32 as the library receives it.  `forms` names the (nys, nzs) shapes of a query's box of cells
the case is there for ("2x3+" is nys = 2 with nzs >= 3, "3+" is nys >= 3: the general path of grid_for_each)."""
from collections import namedtuple

import numpy as np

F = np.float32
Case = namedtuple("Case", "name pts lo hi cell_xy cell_z cap_cells queries r_box r2 forms")

PAD = F(1e-4)          # what the marking and depth layers widen their boxes by
MCL_PAD = F(1e-3)      # kMclPad
CAP = 1 << 22
STOP_ATS = (1, 2, 0x7FFFFFFF)
ROOM = np.array([6.0, 5.0, 2.0])


def _r2(r):
    return F(float(r) * float(r))                 # static_cast<float>(r * r) of a double product, as the callers write it


def _dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _near_points(rng, pts, r, n):
    """a point plus a random direction of length r * {0.5, 0.999, 1, 1.001}, a quarter of the queries each"""
    p = pts[rng.integers(0, len(pts), n)].astype(np.float64)
    scale = np.tile([0.5, 0.999, 1.0, 1.001], (n + 3) // 4)[:n, None]
    return (p + _dirs(rng, n) * scale * float(r)).astype(F)


def _outside_faces(rng, lo, hi, n_per_face, reach, inward=False):
    """queries up to `reach` outside (inward: inside) every face of the box lo .. hi, anywhere across the face"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = []
    for axis in range(3):
        for side in (0, 1):
            q = rng.uniform(lo, hi, (n_per_face, 3))
            off = rng.uniform(0.0, reach, n_per_face) * (-1.0 if inward else 1.0)
            q[:, axis] = lo[axis] - off if side == 0 else hi[axis] + off
            out.append(q)
    return np.concatenate(out).astype(F)


def _far(rng, lo, n):
    return (np.asarray(lo, np.float64) - 100.0 + rng.uniform(-1.0, 1.0, (n, 3))).astype(F)


def _box(pts):
    return pts.min(axis=0).astype(F), pts.max(axis=0).astype(F)


def room_points(seed=1):
    return (np.random.default_rng(seed).uniform(0.0, 1.0, (3000, 3)) * ROOM).astype(F)


def _room_queries(rng, pts, lo, hi, r):
    return np.concatenate([_near_points(rng, pts, r, 384), _outside_faces(rng, lo, hi, 16, 1.0), _far(rng, lo, 32)])


def _room_like(name, seed, r=0.1, cell_xy=0.25, cell_z=0.25, cap=CAP, forms=(), offset=None, extra=None):
    rng = np.random.default_rng(seed)
    pts = room_points()
    if offset is not None:
        pts = (pts + np.asarray(offset, F)).astype(F)
    lo, hi = _box(pts)
    q = _room_queries(rng, pts, lo, hi, r)
    r_box = F(F(r) + PAD)
    if extra is not None:
        q = np.concatenate([q, extra(rng, pts, lo, hi, r_box)])
    return Case(name, pts, lo, hi, F(cell_xy), F(cell_z), cap, q, r_box, _r2(r), tuple(forms))


def _edge_queries(rng, pts, lo, hi, r_box):
    """Queries whose box edges (q - origin) -+ r_box lie within two floats of q of a cell boundary, on every axis and both
    sides: the class of the kilometre defect, where (q -+ r_box) - origin rounds to the float grid of q and can land on
    the other side of the boundary."""
    n = 192
    q = rng.uniform(lo.astype(np.float64), hi.astype(np.float64), (n, 3)).astype(F)
    i = np.arange(n)
    axis, side, steps = i % 3, np.where((i // 3) % 2 == 0, 1.0, -1.0), (i // 6) % 5 - 2
    k = rng.integers(2, 8, n).astype(np.float64)                                 # (the room is 2 m tall: 8 cells)
    x = (lo[axis] + (k * 0.25 - side * float(r_box)).astype(F)).astype(F)
    for j in (-2, -1, 1, 2):
        moved = x.copy()
        for _ in range(abs(j)):
            moved = np.nextafter(moved, F(np.inf if j > 0 else -np.inf))
        x = np.where(steps == j, moved, x)
    q[i, axis] = x
    return q


def tiny_cases():
    lo, hi = np.zeros(3, F), np.ones(3, F)
    q = np.array([[0.55, 0.55, 0.55], [0.6, 0.6, 0.6], [0.5, 0.5, 0.5], [0.9, 0.1, 0.5], [-3.0, 0.5, 0.5], [0.56, 0.56, 0.56]], F)
    one = np.array([[0.55, 0.55, 0.55]], F)
    five = (np.array([0.51, 0.51, 0.51]) + np.random.default_rng(2).uniform(0.0, 0.2, (5, 3))).astype(F)      # all in cell (2, 2, 2)
    twins = np.array([[0.3, 0.3, 0.3], [0.56, 0.56, 0.56], [0.8, 0.2, 0.4], [0.56, 0.56, 0.56]], F)
    mk = lambda name, pts: Case(name, pts, lo, hi, F(0.25), F(0.25), CAP, q, F(F(0.1) + PAD), _r2(0.1), ())
    return [mk("empty", np.zeros((0, 3), F)), mk("one point", one), mk("five in one cell", five), mk("identical pair", twins)]


def boxed(name, shrink, seed):
    rng = np.random.default_rng(seed)
    pts = room_points()
    lo, hi = (np.asarray(shrink, F)).astype(F), (ROOM - np.asarray(shrink)).astype(F)
    q = np.concatenate([_near_points(rng, pts, 0.1, 320), _outside_faces(rng, lo, hi, 16, 0.3),
                        _outside_faces(rng, lo, hi, 16, 0.3, inward=True)])
    return Case(name, pts, lo, hi, F(0.25), F(0.25), CAP, q, F(F(0.1) + PAD), _r2(0.1), ())


def extent_case(seed=9):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-2000.0, -2000.0, -5.0], F), np.array([2090.0, 2090.0, 5.0], F)
    near = lo + rng.uniform(0.0, 1.0, (10000, 3)) * np.array([20.0, 20.0, 10.0])
    far = hi - rng.uniform(0.0, 1.0, (10000, 3)) * np.array([20.0, 20.0, 10.0])
    pts = np.concatenate([near, far]).astype(F)
    q = np.concatenate([_near_points(rng, pts, 1.0, 384), _outside_faces(rng, hi - F(20.0), hi, 8, 1.0),
                        _outside_faces(rng, lo, lo + F(20.0), 8, 1.0), _far(rng, hi, 32)])
    return Case("extent", pts, lo, hi, F(2.0), F(2.0), CAP, q, F(F(1.0) + MCL_PAD), _r2(1.0), ())


def ties_case(seed=10):
    """A lattice of spacing 0.125 (every coordinate and every d2 is an exact float) with 48 points left out and the
    indices shuffled.  Queries: lattice points (six neighbours at exactly d2 == r2), the holes (nothing nearer than that:
    the answer is "none"), edge midpoints (two equal nearest) and face centres (four equal nearest)."""
    rng = np.random.default_rng(seed)
    s = 0.125
    ijk = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    interior = ijk[((ijk > 0) & (ijk < np.array([11, 11, 7]))).all(axis=1) & (ijk.sum(axis=1) % 2 == 0) & (ijk[:, 0] % 3 == 1)]
    holes = interior[rng.permutation(len(interior))[:48]]                           # (no two adjacent: their sum is even)
    keep = np.ones(len(ijk), bool)
    keep[(holes[:, 0] * 12 + holes[:, 1]) * 8 + holes[:, 2]] = False
    kept = ijk[keep]
    pts = (kept[rng.permutation(len(kept))] * s).astype(F)
    on = kept[rng.permutation(len(kept))[:96]] * s
    mid = (ijk[rng.permutation(len(ijk))[:128]] + np.eye(3)[rng.integers(0, 3, 128)] * 0.5) * s
    face = (ijk[rng.permutation(len(ijk))[:128]] + (1.0 - np.eye(3)[rng.integers(0, 3, 128)]) * 0.5) * s
    q = np.concatenate([on, holes * s, mid, face, _far(rng, np.zeros(3), 64), _outside_faces(rng, np.zeros(3), kept.max(axis=0) * s, 8, 1.0)]).astype(F)
    lo, hi = _box(pts)
    return Case("ties", pts, lo, hi, F(0.25), F(0.25), CAP, q, F(F(s) + PAD), F(s * s), ("1x1", "2x1", "1x2", "2x2"))


LOST_ORIGIN, LOST_Q, LOST_P = -1986.9237060546875, 61.126224517822266, 61.07622528076172


def lost_neighbour_case(pad=PAD, seed=13):
    """The known answer of the search for a lost neighbour (tests/test_point_grid_cpu.py): a ground grid of 0.5 m cells
    2050 m long, r = 0.05.  Point 0 and query 0 are the triple: 2047.99994 m and 2048.04993 m from the origin, d2 < r2,
    and with a pad of 1e-4 the point's cell 4095 lies below the box's first cell 4096.  The walks are right to skip it --
    they do what the arithmetic says -- so on the device this case is compared with the box population like any other;
    that the population misses a neighbour is asserted on the CPU alone, and the layers refuse a cloud this wide."""
    rng = np.random.default_rng(seed)
    y, z = 50.0, 0.5
    around = np.array([LOST_P, y, z]) + rng.uniform(-1.0, 1.0, (300, 3)) * np.array([1.0, 1.0, 0.4])
    start = np.array([LOST_ORIGIN, 0.0, 0.0]) + rng.uniform(0.0, 1.0, (100, 3)) * np.array([3.0, 100.0, 1.0])
    pts = np.concatenate([[[LOST_P, y, z]], around, start]).astype(F)
    lo = np.array([LOST_ORIGIN, 0.0, 0.0], F)
    hi = np.array([F(LOST_ORIGIN) + F(2050.0), 100.0, 1.0], F)
    q = np.concatenate([[[LOST_Q, y, z]], _near_points(rng, pts, 0.05, 127)]).astype(F)
    return Case("lost neighbour", pts, lo, hi, F(0.5), F(0.5), CAP, q, F(F(0.05) + F(pad)), _r2(0.05), ())


_EXPECTED = {}


def expected(case):
    """The reference's answers for a case, computed once and shared by the tests (never written to): the grid, what brute
    force finds, the population of each query's box of cells and its (nys, nzs) form."""
    if case.name not in _EXPECTED:
        import point_grid_ref as R
        g = R.grid_shape(case.lo, case.hi, case.cell_xy, case.cell_z, case.cap_cells)
        _EXPECTED[case.name] = dict(grid=g, brute=R.brute_force(case.pts, case.queries, case.r2),
                                    box=R.box_population(g, case.pts, case.queries, case.r_box),
                                    forms=R.walk_form(g, case.queries, case.r_box))
    return _EXPECTED[case.name]


_CASES = []


def cases():
    """all_cases() and the lost neighbour, built once"""
    if not _CASES:
        _CASES.extend(all_cases() + [lost_neighbour_case()])
    return _CASES


def all_cases():
    fast = ("1x1", "2x1", "1x2", "2x2")
    return tiny_cases() + [
        _room_like("room", 3, forms=fast),
        _room_like("shifted", 4, forms=fast, offset=(4000.0, -4000.0, 100.0), extra=_edge_queries),
        _room_like("coarsened", 5, cap=50),
        _room_like("wide", 6, r=0.6, forms=("3+",)),
        _room_like("tall", 7, r=0.12, cell_xy=0.5, cell_z=0.1, forms=("1x3", "1x4", "2x3+")),
        _room_like("flat", 8, cell_z=1e6, forms=("1x1", "2x1")),
        boxed("boxed", (1.0, 1.0, 1.0), 11),
        boxed("boxed, half a metre in z", (1.0, 1.0, 0.5), 12),
        extent_case(),
        ties_case(),
    ]


DESIGNED = ("room", "shifted", "coarsened", "wide", "tall", "flat", "boxed", "boxed, half a metre in z", "extent", "ties")


def form_of(nys, nzs):
    """the name of a box's walk form among those `forms` may list, or None"""
    if nys >= 3:
        return "3+"
    if nys == 2 and nzs >= 3:
        return "2x3+"
    return f"{nys}x{nzs}" if nys * nzs <= 4 else None
