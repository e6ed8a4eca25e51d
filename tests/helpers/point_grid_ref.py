"""The point grid of csrc/point_grid.hip.h and point_grid_plan.hip.h restated in NumPy: every operation in float32 with
every step rounded (NumPy's elementwise float32 operations do not fuse, and the library compiles these lines with
contraction off), and FLANN's L2_Simple in the order of exact_float.hip.h.  Nothing here is read off a kernel: the grid
half is the header's arithmetic, the brute-force half ignores the grid altogether."""
from collections import namedtuple

import numpy as np

F = np.float32
GRID_NONE = 0xFFFFFFFF
INF_BITS = 0x7F800000

Grid = namedtuple("Grid", "nx ny nz ox oy oz inv_xy inv_z")


def f32(x):
    return np.asarray(x, dtype=F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def grid_shape(lo, hi, cell_xy, cell_z, cap_cells) -> Grid:
    """grid_shape(): ceil(extent / cell) + 1 cells an axis, both cell sizes times 1.3f until the product fits the cap."""
    lo, hi, cell_xy, cell_z = f32(lo), f32(hi), F(cell_xy), F(cell_z)
    while True:
        nx = max(1, int(np.ceil((hi[0] - lo[0]) / cell_xy)) + 1)
        ny = max(1, int(np.ceil((hi[1] - lo[1]) / cell_xy)) + 1)
        nz = max(1, int(np.ceil((hi[2] - lo[2]) / cell_z)) + 1)
        if nx * ny * nz <= cap_cells:
            break
        cell_xy = cell_xy * F(1.3)
        cell_z = cell_z * F(1.3)
    return Grid(nx, ny, nz, F(lo[0]), F(lo[1]), F(lo[2]), F(1.0) / cell_xy, F(1.0) / cell_z)


def _axis(g: Grid, axis: int):
    return ((g.ox, g.inv_xy, g.nx), (g.oy, g.inv_xy, g.ny), (g.oz, g.inv_z, g.nz))[axis]


def _clamp(c, n):
    return np.clip(c.astype(np.int64), 0, n - 1)


def cell1(g: Grid, axis: int, x, clamp: bool = True):
    """grid_cx / cy / cz of one argument: floor((x - origin) * inv), clamped into the grid."""
    o, inv, n = _axis(g, axis)
    c = np.floor((f32(x) - o) * inv)
    return _clamp(c, n) if clamp else c.astype(np.int64)


def cell2(g: Grid, axis: int, q, d, clamp: bool = True):
    """grid_cx / cy / cz of two arguments, the cell of a ball's edge: floor(((q - origin) + d) * inv), clamped."""
    o, inv, n = _axis(g, axis)
    c = np.floor(((f32(q) - o) + F(d)) * inv)
    return _clamp(c, n) if clamp else c.astype(np.int64)


def cell2_late_origin(g: Grid, axis: int, q, d):
    """The defect of the history, for the tests that show a case can tell it: floor(((q + d) - origin) * inv), clamped."""
    o, inv, n = _axis(g, axis)
    return _clamp(np.floor(((f32(q) + F(d)) - o) * inv), n)


def point_cells(g: Grid, pts):
    """(cx, cy, cz, linear cell) of every point; cell = (cz * ny + cy) * nx + cx."""
    pts = f32(pts).reshape(-1, 3)
    cx, cy, cz = (cell1(g, a, pts[:, a]) for a in range(3))
    return cx, cy, cz, (cz * g.ny + cy) * g.nx + cx


def histogram(g: Grid, pts):
    return np.bincount(point_cells(g, pts)[3], minlength=g.nx * g.ny * g.nz).astype(np.int64)


def cell_start(g: Grid, pts):
    """The exclusive scan of the histogram, [cells + 1]: its last word is the number of points."""
    return np.concatenate([[0], np.cumsum(histogram(g, pts))]).astype(np.uint32)


def query_box(g: Grid, q, r_box, edge=cell2):
    """(x0, x1, y0, y1, z0, z1) of the box of cells grid_for_each walks for each query, [m, 6]."""
    q = f32(q).reshape(-1, 3)
    cols = []
    for a in range(3):
        cols += [edge(g, a, q[:, a], -F(r_box)), edge(g, a, q[:, a], F(r_box))]
    return np.stack(cols, axis=1)


def box_members(g: Grid, pts, q, r_box, edge=cell2):
    """[m, n] bool: the point lies in a cell of the query's box."""
    cx, cy, cz, _ = point_cells(g, pts)
    b = query_box(g, q, r_box, edge)
    return ((cx[None] >= b[:, 0:1]) & (cx[None] <= b[:, 1:2]) & (cy[None] >= b[:, 2:3]) & (cy[None] <= b[:, 3:4]) &
            (cz[None] >= b[:, 4:5]) & (cz[None] <= b[:, 5:6]))


def walk_form(g: Grid, q, r_box):
    """(nys, nzs) of every query's box, [m, 2]: the fast path of grid_for_each takes nys * nzs <= 4 with nys <= 2."""
    b = query_box(g, q, r_box)
    return np.stack([b[:, 3] - b[:, 2] + 1, b[:, 5] - b[:, 4] + 1], axis=1)


def l2_simple(pts, q):
    """[m, n] float32: dx * dx, then + dy * dy, then + dz * dz, every step rounded (point minus query, as the walks call it)."""
    pts, q = f32(pts).reshape(-1, 3), f32(q).reshape(-1, 3)
    d = pts[None, :, 0] - q[:, 0:1]
    r = d * d
    d = pts[None, :, 1] - q[:, 1:2]
    r = r + d * d
    d = pts[None, :, 2] - q[:, 2:3]
    return r + d * d


def _min_and_id(d2, member, none_d2):
    """Per row: the minimum of d2 over `member`, and the smallest index holding it; (none_d2, GRID_NONE) on an empty row."""
    m = d2.shape[0]
    best = np.full(m, none_d2, F)
    ids = np.full(m, GRID_NONE, np.uint32)
    if d2.shape[1]:
        masked = np.where(member, d2, F(np.inf))
        has = member.any(axis=1)
        best[has] = masked.min(axis=1)[has]
        ids[has] = np.argmax(masked == masked.min(axis=1, keepdims=True), axis=1).astype(np.uint32)[has]
    return best, ids


def brute_force(pts, q, r2):
    """What radiusSearch decides, the grid ignored: per query the number of points with d2 < r2, the minimum d2 over all
    points (+inf without a point), and (id, d2) of the nearest under strict <, the smaller index among equals
    ((GRID_NONE, r2) without one inside)."""
    d2 = l2_simple(pts, q)
    inside = d2 < F(r2)
    dmin, _ = _min_and_id(d2, np.ones_like(inside), F(np.inf))
    best, ids = _min_and_id(d2, inside, F(r2))
    return dict(d2=d2, inside=inside, count=inside.sum(axis=1).astype(np.int64), min_d2=dmin, id=ids, id_d2=best)


def box_population(g: Grid, pts, q, r_box, edge=cell2):
    """What a walk over the query's box of cells must visit: the member matrix, and per query the number of members, the
    sum modulo 2^32 and the xor of their indices, and the minimum d2 among them (+inf without one)."""
    member = box_members(g, pts, q, r_box, edge)
    idx = np.arange(member.shape[1], dtype=np.uint64)
    total = (member * idx[None]).sum(axis=1, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    xor = np.bitwise_xor.reduce(np.where(member, idx[None], np.uint64(0)), axis=1) if member.shape[1] else np.zeros(member.shape[0], np.uint64)
    dmin, _ = _min_and_id(l2_simple(pts, q), member, F(np.inf))
    return dict(member=member, visited=member.sum(axis=1).astype(np.int64), sum=total.astype(np.uint32), xor=xor.astype(np.uint32), min_d2=dmin)
