"""Float64 numpy oracle of the slab symmetry search (adf_slab_symmetry_search / _emit) and of the symmetry-aware site distance
(adf_site_pair_distances_sym), written from the contract in include/adsorbdiff_hip.h, with the slab and site generators of
the tests.

A slab is ``(pos [n,3] float32, Z [n] int64, cell [3,3] float32)``; the oracle reads the float32 values in float64.  An
operation is a dict ``W`` [2,2] int, ``j``, ``R`` [3,3], ``t`` [3], ``perm`` [n].

Exact comparison.  The search decides twice: a point operation by a length error against ``symprec``, a candidate (W, j) by
its worst atom match against ``symprec``.  ``find`` returns both lists of figures and ``assert_margins`` states, before
anything is compared, that none of them lies between ``symprec / 10`` and ``10 symprec``: then no decision can flip between
the float64 oracle and the device's float64 arithmetic (which may round differently by a few 1e-16), and the accepted
``(W, j)`` and every ``perm`` must be the oracle's exactly.

The distance.  ``d_sym`` is held to ``helpers_unique_sites.DIST_ATOL`` (5e-5 A: fewer than ten float32 roundings of 3.8e-6 A
plus the one rounding of the transformed coordinate).  The ``min_diff`` convention jumps where a fractional component is
0.5.  Among the operations that do not map one site onto the other there are always evaluations at that seam - on a 2 x 2
supercell a primitive translation is exactly half a cell - so the seam margin of section 4h is stated for the evaluations
that can decide a minimum: a displacement of norm below ``(0.5 - SEAM_MARGIN) h`` (h: the least height of the cell) has every
fractional component at least ``SEAM_MARGIN`` from 0.5, and one at the seam is at least that long whichever way it falls.
``assert_distance_margins`` therefore asks every finite ``d_sym`` to stay below ``(0.5 - SEAM_MARGIN) h - 0.05`` A and
``TOL_MARGIN`` away from ``tol``.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import helpers_unique_sites as U

SYMPREC = 0.01
TOL = U.TOL


# ------------------------------------------------------------------------------------------------------------ the oracle
def lagrange(A):
    """A [3,2] (columns a, b) -> integer unimodular U [2,2] with A U Lagrange-reduced."""
    Um = np.eye(2, dtype=np.int64)
    for _ in range(100):
        a, b = (A @ Um).T
        if a @ a > b @ b:
            Um = Um[:, ::-1].copy()
            continue
        m = int(np.rint((a @ b) / (a @ a)))
        if m == 0:
            break
        Um[:, 1] -= m * Um[:, 0]
    return Um


def point_ops(cell, symprec=SYMPREC, proper_only=False, span=1):
    """(accepted W [2,2] int in the given basis, sorted; worst length error of every enumerated W_r)."""
    A = np.asarray(cell, np.float64)[:2].T
    Um = lagrange(A)
    Ui = np.rint(np.linalg.inv(Um)).astype(np.int64)
    Ar = A @ Um
    ref = [np.linalg.norm(Ar[:, 0]), np.linalg.norm(Ar[:, 1]), np.linalg.norm(Ar[:, 0] + Ar[:, 1])]
    out, worst = [], []
    for w in itertools.product(range(-span, span + 1), repeat=4):
        Wr = np.array(w, np.int64).reshape(2, 2)
        det = Wr[0, 0] * Wr[1, 1] - Wr[0, 1] * Wr[1, 0]
        if det not in ((1,) if proper_only else (1, -1)):
            continue
        Bm = Ar @ Wr
        err = max(abs(np.linalg.norm(Bm[:, 0]) - ref[0]), abs(np.linalg.norm(Bm[:, 1]) - ref[1]),
                  abs(np.linalg.norm(Bm[:, 0] + Bm[:, 1]) - ref[2]))
        worst.append(err)
        if err <= symprec:
            out.append(Um @ Wr @ Ui)
    out.sort(key=lambda W: tuple(W.reshape(-1)))
    return out, np.asarray(worst)


def frame(cell):
    """(M = [a b n] as columns, its inverse) in float64."""
    cell = np.asarray(cell, np.float64)
    n = np.cross(cell[0], cell[1])
    M = np.stack([cell[0], cell[1], n / np.linalg.norm(n)], 1)
    return M, np.linalg.inv(M)


def reduce_norm(d, M, Mi):
    """|reduce(d)| of the contract for displacements d [...,3]."""
    f = d @ Mi.T
    f[..., :2] -= np.rint(f[..., :2])
    return np.linalg.norm(f @ M.T, axis=-1)


def half_height(cell):
    cell = np.asarray(cell, np.float64)
    area = np.linalg.norm(np.cross(cell[0], cell[1]))
    return 0.5 * area / max(np.linalg.norm(cell[0]), np.linalg.norm(cell[1]))


def find(pos, Z, cell, symprec=SYMPREC, proper_only=False):
    """(operations in the contract's order, worst length errors of the point candidates, worst atom matches of the (W, j)
    candidates)."""
    pos, Z = np.asarray(pos, np.float64), np.asarray(Z)
    assert symprec < half_height(cell)
    M, Mi = frame(cell)
    Ws, lat = point_ops(cell, symprec, proper_only)
    zs, cnt = np.unique(Z, return_counts=True)
    zr = zs[np.argmin(cnt)]                                            # np.unique sorts: ties go to the smaller number
    idx = np.nonzero(Z == zr)[0]
    i0 = idx[0]
    n = len(Z)
    ops = [dict(W=np.eye(2, dtype=np.int64), j=int(i0), R=np.eye(3), t=np.zeros(3), perm=np.arange(n))]
    worst = []
    for W in Ws:
        We = np.eye(3)
        We[:2, :2] = W
        R = M @ We @ Mi
        for j in idx:
            t = pos[j] - R @ pos[i0]
            y = pos @ R.T + t
            dist = reduce_norm(y[:, None, :] - pos[None, :, :], M, Mi)
            dist[Z[:, None] != Z[None, :]] = np.inf
            best = dist.min(1)
            worst.append(best.max())
            if best.max() > symprec:
                continue
            perm = dist.argmin(1)
            if len(set(perm.tolist())) != n:
                continue
            if (W == np.eye(2)).all() and j == i0:
                continue                                                # the identity: already first
            ops.append(dict(W=W, j=int(j), R=R, t=t, perm=perm))
    return ops, lat, np.asarray(worst)


def assert_margins(lat, worst, symprec=SYMPREC):
    """No decision of the search lies within a factor of ten of ``symprec``."""
    for name, v in (("a point candidate's length error", lat), ("a (W, j) candidate's worst atom match", worst)):
        close = v[(v > symprec / 10) & (v < 10 * symprec)]
        assert close.size == 0, f"{name} is {close.min():.3e}: within a factor of ten of symprec = {symprec}"


def _keys(W, t, Mi):
    """One integer per operation: W [...,2,2] and the in-plane fractional part of t [...,3], to 1e-4 of a lattice vector."""
    f = np.asarray(t) @ Mi.T
    assert np.abs(f[..., 2]).max() < 1e-6, "a translation leaves the plane"
    q = np.rint((f[..., :2] % 1.0) * 10000).astype(np.int64) % 10000
    W = np.asarray(W, np.int64).reshape(W.shape[:-2] + (4,)) + 64
    assert W.min() >= 0 and W.max() < 128
    key = np.zeros(W.shape[:-1], np.int64)
    for k in range(4):
        key = key * 128 + W[..., k]
    return (key * 10000 + q[..., 0]) * 10000 + q[..., 1]


def assert_group(ops, Z, cell):
    """Every perm is a permutation that keeps the atomic numbers; the operations are distinct and closed under composition
    and inverse (tau modulo the in-plane lattice, compared to 1e-4 of a lattice vector)."""
    Z = np.asarray(Z)
    _, Mi = frame(cell)
    n = len(Z)
    perm = np.stack([np.asarray(o["perm"]) for o in ops])
    assert (np.sort(perm, 1) == np.arange(n)).all() and (Z[perm] == Z).all()
    W = np.stack([np.asarray(o["W"]).reshape(2, 2) for o in ops]).astype(np.int64)
    R = np.stack([o["R"] for o in ops])
    t = np.stack([o["t"] for o in ops])
    have = _keys(W, t, Mi)
    assert len(set(have.tolist())) == len(ops), "an operation twice"
    Ri = np.linalg.inv(R)
    Wi = np.rint(np.linalg.inv(W.astype(np.float64))).astype(np.int64)
    assert np.isin(_keys(Wi, -np.einsum("pij,pj->pi", Ri, t), Mi), have).all(), "no inverse"
    WW = np.einsum("pij,qjk->pqik", W, W)
    tt = np.einsum("pij,qj->pqi", R, t) + t[:, None, :]
    assert np.isin(_keys(WW, tt, Mi), have).all(), "not closed"


def assert_maps_slab(ops, pos, cell, symprec=SYMPREC):
    """Every operation takes the slab onto itself through its perm, keeps the normal and translates in the plane."""
    M, Mi = frame(cell)
    p = np.asarray(pos, np.float64)
    for o in ops:
        y = p @ np.asarray(o["R"]).T + np.asarray(o["t"])
        assert reduce_norm(y - p[np.asarray(o["perm"])], M, Mi).max() <= symprec
        assert np.abs(np.asarray(o["R"]) @ M[:, 2] - M[:, 2]).max() < 1e-12 and abs(np.asarray(o["t"]) @ M[:, 2]) < 1e-9


# ------------------------------------------------------------------------------------------------ the symmetric distance
def slab_atoms(site):
    return np.nonzero(np.asarray(site["tags"]) != 2)[0]


def apply_op(site, op, cast=True):
    """g . site: every position R x + tau (float64, rounded to float32 once), slab atom perm[k] of the result is the image of
    slab atom k; adsorbate atoms stay in place in the arrays."""
    pos = np.asarray(site["pos"], np.float64) @ np.asarray(op["R"]).T + np.asarray(op["t"])
    if cast:
        pos = pos.astype(np.float32).astype(np.float64)
    sl = slab_atoms(site)
    out = pos.copy()
    out[sl[np.asarray(op["perm"])]] = pos[sl]
    return dict(site, pos=out)


def pair_distance(a, b, include_slab=True, permutation_invariant=True):
    """Section 4h's d(a, b) with the cell of a."""
    return U.group_distances([a, b], include_slab, permutation_invariant)[0][0, 1]


def row_distances(a, others, include_slab=True, permutation_invariant=True):
    """Section 4h's d(a, b) for every b of ``others``, with the cell of a (+inf where the layouts differ): the first row of
    ``helpers_unique_sites.group_distances([a] + others)`` without the rows nobody asks for (the 65-site group times its
    operations would otherwise take seconds)."""
    out = np.full(len(others), np.inf)
    key = U._layout(a)
    same = [k for k, b in enumerate(others) if U._layout(b) == key]
    if not same:
        return out
    Pa = np.asarray(a["pos"], np.float64)
    if len(Pa) == 0:
        out[same] = 0.0
        return out
    cell = np.asarray(a["cell"], np.float64)
    ads = np.asarray(a["tags"]) == 2
    Za = np.asarray(a["Z"])[ads]
    B = np.stack([np.asarray(others[k]["pos"], np.float64) for k in same])
    norm = np.linalg.norm(U.min_diff(B - Pa[None], cell)[0], axis=-1)       # [m, atoms]
    d = np.zeros(len(same))
    if include_slab and (~ads).any():
        d = np.maximum(d, norm[:, ~ads].max(1))
    if ads.any() and not permutation_invariant:
        d = np.maximum(d, norm[:, ads].max(1))
    if ads.any() and permutation_invariant:
        nrm = np.linalg.norm(U.min_diff(B[:, ads][:, None, :, :] - Pa[ads][None, :, None, :], cell)[0], axis=-1)
        nrm = np.where((Za[:, None] == Za[None, :])[None], nrm, np.inf)      # [m, atoms of a, atoms of b]
        d = np.maximum(d, np.maximum(nrm.min(2).max(1), nrm.min(1).max(1)))
    out[same] = d
    return out


def sym_group_distances(sites, ops, include_slab=True, permutation_invariant=True, return_gap=False):
    """(d_sym [n,n], best_op [n,n]) of one group whose slab has the operations ``ops``; ``return_gap``: also how far the
    second least operation lies above the least (+inf with one operation) - below a rounding error best_op is a toss-up,
    as it is for a bare slab, which every operation takes onto itself."""
    n = len(sites)
    D, best, gap = np.zeros((n, n)), np.zeros((n, n), np.int64), np.full((n, n), np.inf)
    n_slab = len(ops[0]["perm"])
    for i in range(n):
        if i + 1 == n:
            break
        usable = len(slab_atoms(sites[i])) == n_slab
        rows = [row_distances(apply_op(sites[i], op), sites[i + 1:], include_slab, permutation_invariant) if usable
                else np.full(n - i - 1, np.inf) for op in ops]
        rows = np.stack(rows)                                           # [ops, later sites]
        pick = rows.argmin(0)                                           # the first least: ties to the lowest index
        d = rows[pick, np.arange(n - i - 1)]
        pick = np.where(np.isfinite(d), pick, 0)
        D[i, i + 1:] = D[i + 1:, i] = d
        best[i, i + 1:] = best[i + 1:, i] = pick
        if len(ops) > 1:
            second = np.sort(rows, 0)[1]
            with np.errstate(invalid="ignore"):                          # inf - inf where the sites cannot be compared
                gap[i, i + 1:] = gap[i + 1:, i] = np.where(np.isfinite(d), second - d, np.inf)
    return (D, best, gap) if return_gap else (D, best)


def assert_distance_margins(matrices, cells, tol=TOL):
    for D, cell in zip(matrices, cells):
        off = D[~np.eye(len(D), dtype=bool)]
        off = off[np.isfinite(off)]
        if not off.size:
            continue
        gap = float(np.abs(off - tol).min())
        assert gap >= U.TOL_MARGIN, f"a pair distance lies {gap:.2e} A from tol"
        cell = np.asarray(cell, np.float64)
        heights = abs(np.linalg.det(cell)) / np.linalg.norm(np.cross(cell[[1, 2, 0]], cell[[2, 0, 1]]), axis=1)
        bound = (0.5 - U.SEAM_MARGIN) * heights.min() - 0.05
        assert off.max() <= bound, f"d_sym of {off.max():.3f} A could be decided at the 0.5 seam (bound {bound:.3f} A)"


# --------------------------------------------------------------------------------------------------------- the generators
def fcc(kind, p, q, layers, a0=3.9, vac=15.0):
    """An fcc (111), (100) or (110) slab of p x q surface cells and ``layers`` layers (Pt)."""
    s = a0 / np.sqrt(2)
    if kind == "111":
        a, b, dz, offs = np.array([s, 0, 0]), np.array([s / 2, s * np.sqrt(3) / 2, 0]), a0 / np.sqrt(3), [(0, 0), (1 / 3, 1 / 3), (2 / 3, 2 / 3)]
    elif kind == "100":
        a, b, dz, offs = np.array([s, 0, 0]), np.array([0, s, 0]), a0 / 2, [(0, 0), (.5, .5)]
    else:
        a, b, dz, offs = np.array([a0, 0, 0]), np.array([0, s, 0]), a0 / (2 * np.sqrt(2)), [(0, 0), (.5, .5)]
    P = []
    for layer in range(layers):
        o = offs[layer % len(offs)]
        for i in range(p):
            for j in range(q):
                P.append((i + o[0]) * a + (j + o[1]) * b + np.array([0, 0, 5 + layer * dz]))
    cell = np.stack([p * a, q * b, np.array([0, 0, 10 + layers * dz + vac])])
    return np.array(P, np.float32), np.full(len(P), 78, np.int64), cell.astype(np.float32)


def substituted():
    """fcc(111) 2x2x3 with one top atom replaced: the rarest species has one atom, 6 operations are left."""
    p, Z, c = fcc("111", 2, 2, 3)
    Z = Z.copy()
    Z[np.argmax(p[:, 2])] = 8
    return p, Z, c


def two_species():
    """fcc(111) 2x2x3 whose top layer is another element: the rarest species has four atoms."""
    p, Z, c = fcc("111", 2, 2, 3)
    Z = Z.copy()
    Z[p[:, 2] > p[:, 2].max() - 0.1] = 29
    return p, Z, c


def non_reduced(k=2):
    p, Z, c = fcc("111", 2, 2, 3)
    c = c.copy()
    c[0] = c[0] + k * c[1]
    return p, Z, c


def left_handed():
    p, Z, c = fcc("111", 2, 2, 3)
    c = c.copy()
    c[[0, 1]] = c[[1, 0]]
    return p, Z, c


def rattled(symprec=SYMPREC):
    """fcc(111) 3x3x3 with every atom moved by 0.1-0.3 A: the identity alone.  Redrawn (at most 20 times) until the margins hold."""
    p, Z, c = fcc("111", 3, 3, 3)
    for seed in range(20):
        rng = np.random.default_rng(seed)
        v = rng.normal(size=p.shape)
        v *= (rng.uniform(.1, .3, len(p)) / np.linalg.norm(v, axis=1))[:, None]
        moved = (p + v).astype(np.float32)
        _, lat, worst = find(moved, Z, c, symprec)
        if not ((worst > symprec / 10) & (worst < 10 * symprec)).any():
            return moved, Z, c
    raise AssertionError("no rattled slab met the margins in 20 draws")


# name -> (generator, operations expected by crystallography)
SLABS = {
    "111_1x1x3": (lambda: fcc("111", 1, 1, 3), 6),
    "111_2x2x3": (lambda: fcc("111", 2, 2, 3), 24),
    "111_3x3x4": (lambda: fcc("111", 3, 3, 4), 54),
    "111_5x5x3": (lambda: fcc("111", 5, 5, 3), 150),
    "100_1x1x2": (lambda: fcc("100", 1, 1, 2), 8),
    "100_2x2x3": (lambda: fcc("100", 2, 2, 3), 32),
    "110_1x1x2": (lambda: fcc("110", 1, 1, 2), 4),
    "111_2x3x3": (lambda: fcc("111", 2, 3, 3), 6),
    "substituted": (substituted, 6),
    "two_species": (two_species, 24),
    "non_reduced": (non_reduced, 24),
    "left_handed": (left_handed, 24),
    "rattled": (rattled, 1),
    "one_atom": (lambda: fcc("111", 1, 1, 1), 12),
    "111_7x7x4": (lambda: fcc("111", 7, 7, 4), 294),
}
# 1026 atoms: more than the search kernel stages in LDS (csrc/symmetry.hip, SY_CAP = 1024); 19 x 18 translations
LARGE_SLAB = ("111_19x18x3", lambda: fcc("111", 19, 18, 3), 342)
ORACLE_MAX_ATOMS = 75
MIRRORS = {"111_1x1x3", "111_2x2x3", "111_3x3x4", "111_5x5x3", "100_1x1x2", "100_2x2x3", "110_1x1x2", "substituted",
           "two_species", "non_reduced", "left_handed", "one_atom", "111_7x7x4"}


@functools.lru_cache(maxsize=None)
def slab(name):
    return LARGE_SLAB[1]() if name == LARGE_SLAB[0] else SLABS[name][0]()


@functools.lru_cache(maxsize=None)
def oracle(name, proper_only=False):
    """(operations, point margins, candidate margins) of a named slab; the margins are asserted here."""
    ops, lat, worst = find(*slab(name), SYMPREC, proper_only)
    assert_margins(lat, worst)
    return ops, lat, worst


def slab_batch(names, device="cpu"):
    import torch

    from adsorbdiff_amd.data import Batch, Data

    data = []
    for k, name in enumerate(names):
        p, Z, c = slab(name)
        data.append(Data(pos=torch.from_numpy(p).float().clone(), atomic_numbers=torch.from_numpy(Z).long(),
                         tags=torch.ones(len(Z), dtype=torch.long), fixed=torch.zeros(len(Z), dtype=torch.long),
                         cell=torch.from_numpy(c).float().reshape(1, 3, 3), sid=str(k)))
    return Batch.from_data_list(data).to(device)


ADSORBATES = {0: [], 1: [8], 2: [7, 7], 5: [6, 1, 1, 8, 1]}


def base_site(slab_name, n_ads, group, rng, around=None, radius=1.0):
    """The slab with an adsorbate of ``n_ads`` atoms at a random place above it; ``around``: within ``radius`` (in the plane)
    of that slab atom."""
    p, Z, c = slab(slab_name)
    cell = c.astype(np.float64)
    Za = np.asarray(ADSORBATES[n_ads], np.int64)
    if around is None:
        xy = rng.uniform(0, 1, 2) @ cell[:2]
    else:
        r, phi = radius * np.sqrt(rng.uniform()), rng.uniform(0, 2 * np.pi)
        xy = p[around].astype(np.float64) * [1, 1, 0] + [r * np.cos(phi), r * np.sin(phi), 0]
    centre = xy + np.array([0, 0, p[:, 2].max() + 1.8])
    shape = np.column_stack([rng.uniform(-0.7, 0.7, (n_ads, 2)), rng.uniform(0.0, 0.8, n_ads)])
    if n_ads == 2:
        shape = np.array([[0, 0, 0], [1.1 * np.cos(0.4), 0, 1.1 * np.sin(0.4)]])
    pos = np.concatenate([p.astype(np.float64), centre + shape]) if n_ads else p.astype(np.float64)
    tags = np.concatenate([np.arange(len(Z)) % 2, np.full(n_ads, 2)]).astype(np.int64)
    return {"pos": pos.astype(np.float32), "tags": tags, "Z": np.concatenate([Z, Za]).astype(np.int64), "cell": c, "group": group}


def image(site, op, rng, tol=TOL, wrap=False):
    """The site's image under ``op``, rigidly shifted by 0.2-0.4 tol, its slab atoms rattled by less than 0.1 tol and carried
    along by perm; ``wrap``: every atom is brought back into the cell."""
    out = apply_op(site, op, cast=False)
    u = rng.normal(size=3)
    pos = out["pos"] + u / np.linalg.norm(u) * rng.uniform(0.2, 0.4) * tol
    sl = slab_atoms(site)
    v = rng.normal(size=(len(sl), 3))
    pos[sl] += v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0, 0.1 * tol, (len(sl), 1))
    if wrap:
        cell = np.asarray(site["cell"], np.float64)
        pos = (pos @ np.linalg.inv(cell) % 1.0) @ cell
    return dict(site, pos=pos.astype(np.float32))


# (slab, sites, base sites, adsorbate atoms): group id = position in this list = slab index of the symmetry
DISTANCE_GROUPS = [("100_2x2x3", 1, 1, 1), ("111_2x2x3", 2, 1, 2), ("100_2x2x3", 3, 2, 0), ("111_2x2x3", 6, 2, 5),
                   ("substituted", 65, 12, 1)]


DISTANCE_SEED = 32            # a draw whose margins hold (assert_distance_margins, in float64)


@functools.lru_cache(maxsize=None)
def distance_case():
    """(sites in the caller's order - groups interleaved -, slab names by group id).  Every group holds a few base sites and
    images of them under randomly chosen operations of its slab (mirrors included), half of them wrapped.  The 6-site group
    also holds a site whose slab has lost an atom."""
    rng = np.random.default_rng(DISTANCE_SEED)
    sites = []
    for g, (name, n, n_base, n_ads) in enumerate(DISTANCE_GROUPS):
        ops = oracle(name)[0]
        # the substituted slab has no translation among its operations: its sites stay within 1 A of the three-fold axis
        # through the substituted atom, so that no two of them are far enough apart to be compared across the 0.5 seam
        around = int(np.argmin(slab(name)[1])) if name == "substituted" else None
        bases = [base_site(name, n_ads, g, rng, around=around) for _ in range(n_base)]
        members = list(bases)
        while len(members) < n:
            k = len(members)
            members.append(image(bases[int(rng.integers(n_base))], ops[int(rng.integers(1, len(ops)))], rng, wrap=bool(k % 2)))
        if n == 6:
            s = members[-1]
            members[-1] = dict(s, pos=s["pos"][1:], tags=s["tags"][1:], Z=s["Z"][1:])
        sites += members
    order = rng.permutation(len(sites))
    return [sites[i] for i in order], [d[0] for d in DISTANCE_GROUPS]


def distance_oracle(include_slab=True, permutation_invariant=True):
    """(d_sym matrices, best_op matrices) of ``distance_case`` in ascending group order, the margins asserted."""
    return _distance_oracle(include_slab, permutation_invariant)[:2]


def distance_gaps():
    """Per group, how far the second least operation lies above the least (default mode)."""
    return _distance_oracle(True, True)[2]


@functools.lru_cache(maxsize=None)
def _distance_oracle(include_slab, permutation_invariant):
    sites, names = distance_case()
    _, members = U.regroup_numpy([s["group"] for s in sites])
    D, best, gaps = [], [], []
    for g, m in enumerate(members):
        d, b, q = sym_group_distances([sites[i] for i in m], oracle(names[g])[0], include_slab, permutation_invariant, True)
        D.append(d)
        best.append(b)
        gaps.append(q)
    assert_distance_margins(D, [slab(n)[2] for n in names])
    return D, best, gaps
