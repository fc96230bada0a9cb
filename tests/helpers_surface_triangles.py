"""Float64 numpy oracle of the device triangulation (adf_surface_triangles), written from the contract in
include/adsorbdiff_hip.h, with the case builders and the invariants of its tests.

The oracle is brute force: every triple of tiled points whose least index lies in the central tile, its circumcircle, and
the signed distance ``|p - centre| - r`` of every other point to it.  A triple is *strict* when every other point is outside
by more than ``circle_tol`` and *admissible* (empty up to ``circle_tol``) when none is inside by more than ``circle_tol``.
For points in general position the two sets are equal and are the Delaunay triangles that ``surface_triangles`` keeps.
``expected`` goes on to apply the contract's fan rule to the polygons of the admissible triples.  Fine at n <= 81 points.

Exact comparison.  A triple is decided by its deepest point (the least signed distance) and, when admissible, the polygon
on its circle by every point's distance.  ``triples`` returns those figures and ``assert_margins`` states that none lies in
(circle_tol / 10, 10 circle_tol) - the factor-of-ten band of helpers_heuristic_sites - so no decision can flip between this
oracle and the device's float64 arithmetic, and the device's table must be the oracle's exactly."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

from tests import helpers_heuristic_sites as HH

CIRCLE_TOL = 1e-4
GOLDEN = Path(__file__).resolve().parent / "golden" / "surface_triangles.npz"
REPEATS = [(0, 0)] + [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]
LATTICES = ("111_3x3x4", "100_2x2x3", "110_1x1x2", "111_2x2x3")
DEGENERATE = ("100_2x2x3", "110_1x1x2")
SEED = 20240611


# ------------------------------------------------------------------------------------------------------------ the contract
def tiling_vectors(cell):
    """The first two rows v of the cell with |v_x| >= 0.0005 or |v_y| >= 0.05 (None: fewer than two)."""
    cell = np.asarray(cell, np.float32).astype(np.float64).reshape(3, 3)
    vs = [v for v in cell if abs(v[0]) >= 0.0005 or abs(v[1]) >= 0.05]
    return np.stack(vs[:2]) if len(vs) >= 2 else None


def tiled_points(pos, tags, cell):
    """(float64 [9 n_top, 3], n_top): point tile * n_top + ordinal = (p + i v0) + j v1."""
    surf = np.asarray(pos, np.float32).astype(np.float64)[np.asarray(tags) == 1]
    v = tiling_vectors(cell)
    return np.concatenate([(surf + i * v[0]) + j * v[1] for i, j in REPEATS]), len(surf)


def canonical(index, xy):
    """Rows (a, b, c): a the least index, a -> b -> c counter-clockwise in x, y; sorted ascending.  Also the permutation
    applied to every row's corners and the order of the rows: ``out = index[order][rows, perm]``."""
    index = np.asarray(index, np.int64).reshape(-1, 3)
    perm = np.zeros_like(index)
    for r, t in enumerate(index):
        k = int(np.argmin(t))
        p = [k, (k + 1) % 3, (k + 2) % 3]
        a, b, c = xy[t[p[0]]], xy[t[p[1]]], xy[t[p[2]]]
        if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) < 0:
            p = [p[0], p[2], p[1]]
        perm[r] = p
    rows = np.take_along_axis(index, perm, 1)
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0])) if len(rows) else np.zeros(0, np.int64)
    return rows[order], perm[order], order


def triples(xy, n_top, tol=CIRCLE_TOL):
    """Every triple a < b < c with a in the central tile that spans an area: dict ``index`` [M,3], ``centre`` [M,2], ``r``
    [M], ``signed`` [M,n] (|p - centre| - r, +inf at the triple's own corners), ``strict`` / ``admissible`` [M] bool and
    ``figures``: per triple the magnitude of its deepest signed distance, and for the admissible ones every magnitude."""
    xy = np.asarray(xy, np.float64)
    n = len(xy)
    a, b, c = np.meshgrid(np.arange(n_top), np.arange(n), np.arange(n), indexing="ij")
    keep = (a < b) & (b < c)
    idx = np.stack([a[keep], b[keep], c[keep]], 1)
    A, B, C = xy[idx[:, 0]], xy[idx[:, 1]], xy[idx[:, 2]]
    ab, ac = B - A, C - A
    cross = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    spans = np.abs(cross) > 1e-9 * np.linalg.norm(ab, axis=1) * np.linalg.norm(ac, axis=1)
    idx, A, ab, ac, cross = idx[spans], A[spans], ab[spans], ac[spans], cross[spans]
    ab2, ac2 = (ab * ab).sum(1), (ac * ac).sum(1)
    u = np.stack([ac[:, 1] * ab2 - ab[:, 1] * ac2, ab[:, 0] * ac2 - ac[:, 0] * ab2], 1) / (2.0 * cross)[:, None]
    centre, r = A + u, np.linalg.norm(u, axis=1)
    signed = np.linalg.norm(xy[None, :, :] - centre[:, None, :], axis=2) - r[:, None]
    signed[np.arange(len(idx))[:, None], idx] = np.inf
    deepest = signed.min(1)
    strict, admissible = deepest > tol, deepest >= -tol
    on = np.abs(signed[admissible])
    figures = np.concatenate([np.abs(deepest), on[np.isfinite(on)].ravel()])
    return dict(index=idx, centre=centre, r=r, signed=signed, strict=strict, admissible=admissible, figures=figures)


def assert_margins(res, tol=CIRCLE_TOL):
    """No decision lies within a factor of ten of circle_tol."""
    f = res["figures"]
    close = f[(f > tol / 10) & (f < 10 * tol)]
    assert close.size == 0, f"a point lies {close.min():.3e} A off a circumcircle: within a factor of ten of circle_tol = {tol}"


def rows_of(res, which, xy):
    return canonical(res["index"][res[which]], xy)[0]


def expected(xy, n_top, tol=CIRCLE_TOL, res=None):
    """The contract's table: per admissible triple the polygon of the points on its circle, split as a fan from its
    canonical vertex (least x up to tol, then least y, then least index); the fans' triangles with a central corner."""
    xy = np.asarray(xy, np.float64)
    res = triples(xy, n_top, tol) if res is None else res
    out = set()
    for m in np.nonzero(res["admissible"])[0]:
        poly = np.concatenate([res["index"][m], np.nonzero(np.abs(res["signed"][m]) <= tol)[0]])
        c = res["centre"][m]
        poly = poly[np.argsort(np.arctan2(xy[poly, 1] - c[1], xy[poly, 0] - c[0]))]          # counter-clockwise
        near = poly[xy[poly, 0] <= xy[poly, 0].min() + tol]
        v = near[np.lexsort((near, xy[near, 1]))[0]]
        ring = np.roll(poly, -int(np.nonzero(poly == v)[0][0]))
        for s in range(1, len(ring) - 1):
            t = (int(ring[0]), int(ring[s]), int(ring[s + 1]))
            if min(t) < n_top:
                out.add(tuple(sorted(t)))
    return canonical(np.array(sorted(out), np.int64).reshape(-1, 3), xy)[0]


# ---------------------------------------------------------------------------------------------------------- the invariants
def check_table(xy, n_top, index):
    """What holds for any table of the contract, with no oracle: rows canonical, ascending and distinct, every area > 0,
    and around every central point the incident angles sum to 2 pi within 1e-9 - its star is closed and does not overlap."""
    xy, index = np.asarray(xy, np.float64), np.asarray(index, np.int64)
    assert index.min() >= 0 and index.max() < len(xy)
    assert (index[:, 0] < index[:, 1]).all() and (index[:, 0] < index[:, 2]).all() and (index[:, 0] < n_top).all()
    keys = [tuple(t) for t in index]
    assert keys == sorted(set(keys)), "rows not ascending or not distinct"
    A, B, C = xy[index[:, 0]], xy[index[:, 1]], xy[index[:, 2]]
    area = 0.5 * ((B[:, 0] - A[:, 0]) * (C[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (C[:, 0] - A[:, 0]))
    assert (area > 0).all(), f"least signed area {area.min():.3e}"
    total = np.zeros(n_top)
    for corner in range(3):
        p, q, r = xy[index[:, corner]], xy[index[:, (corner + 1) % 3]], xy[index[:, (corner + 2) % 3]]
        e1, e2 = q - p, r - p
        ang = np.arctan2(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0], (e1 * e2).sum(1))
        central = index[:, corner] < n_top
        np.add.at(total, index[central, corner], ang[central])
    assert np.abs(total - 2 * np.pi).max() <= 1e-9, f"angles around a central point sum to 2 pi {np.abs(total - 2 * np.pi).max():+.3e}"


def longest_edge_directions(xy, index):
    """Per triangle the unit vector along its longest edge, its sign fixed (x > 0, or x = 0 and y > 0)."""
    xy, index = np.asarray(xy, np.float64), np.asarray(index, np.int64)
    e = np.stack([xy[index[:, (k + 1) % 3]] - xy[index[:, k]] for k in range(3)], 1)       # [T,3,2]
    d = e[np.arange(len(index)), np.argmax((e * e).sum(2), axis=1)]
    d = d / np.linalg.norm(d, axis=1)[:, None]
    flip = (d[:, 0] < -1e-9) | ((np.abs(d[:, 0]) <= 1e-9) & (d[:, 1] < 0))
    d[flip] *= -1
    return d


def hex_count(p):
    """Kept triangles of a perfect p x p triangular lattice, with no oracle.  Every lattice cell (i, j) is split into the
    triangles U = {(i,j), (i+1,j), (i,j+1)} and D = {(i+1,j), (i+1,j+1), (i,j+1)} (the other diagonal is the mirror image and
    counts the same).  With the central tile at 0 <= i, j < p, U has a central corner for the p^2 cells of the tile and for
    the p cells each with i = -1 or j = -1 whose corner (0, j) or (i, 0) is central, (-1, -1) has none: p^2 + 2 p.  D has
    one for i + 1 in the tile and j in [-1, p - 1], p (p + 1) cells, and for i = p - 1 with j + 1 in the tile, p cells:
    p^2 + 2 p.  Together 2 p^2 + 4 p: two triangles per central point and a ring of 4 p."""
    return 2 * p * p + 4 * p


# ------------------------------------------------------------------------------------------------------- the case builders
def _slab(top_xy, cell, z_top=12.0, z_low=9.8, lower=None):
    """pos float32 [n,3], Z, cell float32 [3,3], tags: the lower layer (tag 0) first, then the tag-1 atoms."""
    top_xy = np.asarray(top_xy, np.float64).reshape(-1, 2)
    lower = top_xy + 0.7 if lower is None else np.asarray(lower, np.float64).reshape(-1, 2)
    pos = np.concatenate([np.column_stack([lower, np.full(len(lower), z_low)]),
                          np.column_stack([top_xy, np.full(len(top_xy), z_top)])]).astype(np.float32)
    tags = np.concatenate([np.zeros(len(lower), np.int64), np.ones(len(top_xy), np.int64)])
    return dict(pos=pos, Z=np.full(len(pos), 29, np.int64), cell=np.asarray(cell, np.float32), tags=tags)


@functools.lru_cache(maxsize=None)
def generic3():
    """Three slabs for one batch with 1, 5 and 9 tag-1 atoms over a lower layer, in-plane jitter 0.15 A, fixed seed.  The
    first has a skewed cell, the second has its cell rows permuted (c first: ``tiling_vectors`` skips it)."""
    rng = np.random.default_rng(SEED)
    jit = lambda k: rng.uniform(-0.15, 0.15, size=(k, 2))
    one = _slab(np.array([[0.9, 0.6]]) + jit(1), [[2.9, 0.0, 0.0], [1.1, 2.6, 0.0], [0.0, 0.0, 20.0]])
    a, b = np.array([5.2, 0.0]), np.array([0.4, 4.9])
    frac = np.array([[0.1, 0.1], [0.6, 0.15], [0.3, 0.5], [0.8, 0.6], [0.45, 0.85]])
    five = _slab(frac[:, :1] * a + frac[:, 1:] * b + jit(5), [[0.0, 0.0, 18.0], [5.2, 0.0, 0.0], [0.4, 4.9, 0.0]])
    grid = np.array([[i * 2.7, j * 2.7] for i in range(3) for j in range(3)]) + 0.4
    nine = _slab(grid + jit(9), [[8.1, 0.0, 0.0], [0.0, 8.1, 0.0], [0.0, 0.0, 22.0]])
    return (one, five, nine)


def lattice(name):
    c = HH.case(name)
    return dict(pos=c["pos"], Z=c["Z"], cell=c["cell"], tags=c["tags"])


def batch_of(cases, device="cpu"):
    import torch

    from adsorbdiff_amd.data import Batch, Data

    data = []
    for k, c in enumerate(cases):
        n = len(c["Z"])
        data.append(Data(pos=torch.from_numpy(np.asarray(c["pos"], np.float32)).clone(),
                         atomic_numbers=torch.from_numpy(np.asarray(c["Z"])).long(),
                         tags=torch.from_numpy(np.asarray(c["tags"])).long(), fixed=torch.zeros(n, dtype=torch.long),
                         cell=torch.from_numpy(np.asarray(c["cell"], np.float32)).reshape(1, 3, 3), natoms=torch.tensor([n]),
                         sid=f"surface-{k}"))
    return Batch.from_data_list(data).to(device)


@functools.lru_cache(maxsize=None)
def oracle(key, which=0):
    """``triples`` of a named case - ``"generic3"`` (slab ``which``) or a lattice - with its tiled points: (xy, n_top, res)."""
    c = generic3()[which] if key == "generic3" else lattice(key)
    pts, n_top = tiled_points(c["pos"], c["tags"], c["cell"])
    return pts[:, :2], n_top, triples(pts[:, :2], n_top)


# ------------------------------------------------------------------------------------------------------------- the fixture
FIXTURE_CASES = (("generic3", 0), ("generic3", 1), ("generic3", 2), ("111_3x3x4", 0))


def fixture_name(key, which):
    return f"{key}_{which}" if key == "generic3" else key


def fixture_case(key, which):
    return generic3()[which] if key == "generic3" else lattice(key)


@functools.lru_cache(maxsize=None)
def load_fixture():
    """name -> dict(pos, Z, cell, tags, index [T,3] int64: scipy's kept triangles as canonical rows, vertices [T,3,3] float32:
    the rows of ``surface_triangles`` in that order)."""
    with np.load(GOLDEN) as z:
        names = sorted({k.rsplit("__", 1)[0] for k in z.files})
        return {n: {f: z[f"{n}__{f}"] for f in ("pos", "Z", "cell", "tags", "index", "vertices")} for n in names}


def scipy_rows(case):
    """``surface_triangles`` (scipy) on one case as the fixture records it: (index, vertices)."""
    from adsorbdiff_amd import placement as PL

    host = PL.surface_triangles(batch_of([case]))[0]                     # [T,3,3] float64, scipy's order
    pts, n_top = tiled_points(case["pos"], case["tags"], case["cell"])
    look = {tuple(p): k for k, p in enumerate(pts)}
    assert len(look) == len(pts), "two tiled points coincide"
    idx = np.array([[look[tuple(v)] for v in t] for t in host], np.int64)  # the host's rows are tiled points, bit for bit
    rows, perm, order = canonical(idx, pts[:, :2])
    vertices = np.take_along_axis(host[order], perm[:, :, None], 1).astype(np.float32)
    return rows, vertices
