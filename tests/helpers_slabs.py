"""An independent float64 numpy statement of the slab-cutting contract (include/adsorbdiff_hip.h "Slab cutting"), by brute
force: the in-plane basis and u3 come from a search over small integer vectors (no Euclid, no reduction), a slab's atoms
from a block of periodic images cut by height and by the in-plane cell (no lifting of the oriented cell), equivalence from
trying every pairing of one atom with every atom of the other slab and every periodic image.  Also the invariant checkers
(a)-(g) and the margin assertions that keep every decision of a case away from a rounding.  Parity with pymatgen unpinned:
neither pymatgen nor spglib was run against it."""
from __future__ import annotations

import itertools
import math

import numpy as np

TIE = 1e-9          # squared lengths within TIE * L^2 tie (L: the longest cell edge)
FTOL = 1e-6         # fractional in-plane coordinates within FTOL are equal
BOX = 8             # the integer vectors searched: |coordinates| <= BOX
IMAGES = 7          # periodic images of the bulk generated per direction: -IMAGES .. IMAGES


# ---- the crystals of the case table (cell rows, fractional coordinates, atomic numbers)
def _crystal(cell, frac, Z):
    cell = np.asarray(cell, np.float64)
    return {"cell": cell, "pos": np.asarray(frac, np.float64) @ cell, "Z": np.asarray(Z, np.int64)}


def crystals():
    fcc = [(0, 0, 0), (0.5, 0.5, 0), (0.5, 0, 0.5), (0, 0.5, 0.5)]
    s3 = math.sqrt(3.0)
    return {
        "fcc_cu": _crystal(np.eye(3) * 3.61, fcc, [29] * 4),
        "bcc_fe": _crystal(np.eye(3) * 2.87, [(0, 0, 0), (0.5, 0.5, 0.5)], [26, 26]),
        "cscl": _crystal(np.eye(3) * 3.0, [(0, 0, 0), (0.5, 0.5, 0.5)], [55, 17]),
        "cu3au": _crystal(np.eye(3) * 3.75, fcc, [79, 29, 29, 29]),
        "hcp_mg": _crystal([(3.21, 0, 0), (-3.21 / 2, 3.21 * s3 / 2, 0), (0, 0, 5.21)],
                           [(1 / 3, 2 / 3, 0.25), (2 / 3, 1 / 3, 0.75)], [12, 12]),
        "triclinic": _crystal([(3.1, 0, 0), (0.7, 3.6, 0), (0.4, 0.9, 4.2)], [(0.1, 0.2, 0.3), (0.6, 0.55, 0.8)], [13, 28]),
        "tetragonal": _crystal(np.diag([3.0, 3.0, 4.0]), [(0, 0, 0)], [78]),
    }


# (crystal, h, d, n_slab, distinct cuts, slabs out, atoms of a primitive slab, atomic layers)
CASE_TABLE = [
    ("fcc_cu", (1, 1, 1), 2.0842, 4, 1, 1, 4, 4), ("fcc_cu", (1, 0, 0), 3.61, 2, 1, 1, 4, 4),
    ("fcc_cu", (1, 1, 0), 2.5527, 3, 1, 1, 6, 6), ("fcc_cu", (2, 1, 1), 1.4738, 5, 1, 1, 10, 10),
    ("fcc_cu", (2, 1, 0), 1.6144, 5, 1, 1, 10, 10),
    ("bcc_fe", (1, 0, 0), 2.87, 3, 1, 1, 6, 6), ("bcc_fe", (1, 1, 0), 2.0294, 4, 1, 1, 4, 4),
    ("bcc_fe", (1, 1, 1), 1.6570, 5, 1, 1, 10, 10),
    ("cscl", (1, 0, 0), 3.0, 3, 2, 4, 6, 6), ("cscl", (1, 1, 0), 2.1213, 4, 1, 1, 8, 4), ("cscl", (1, 1, 1), 1.7321, 5, 2, 4, 10, 10),
    ("cu3au", (1, 0, 0), None, 2, 2, 4, 8, 4), ("cu3au", (1, 1, 0), None, 3, 2, 4, 12, 6), ("cu3au", (1, 1, 1), None, 4, 1, 1, 16, 4),
    ("hcp_mg", (0, 0, 1), 5.21, 2, 1, 1, 4, 4), ("hcp_mg", (1, 0, 0), 2.7799, 3, 2, 2, 6, 6),
    ("triclinic", (1, 0, 0), 3.0388, 3, 2, 4, 6, 6), ("triclinic", (1, -1, 2), 1.4304, 5, 1, 2, 10, 10),
]
# further (bulk, h) pairs of the device batch: unreduced and negative indices, the rest of the low-index faces
EXTRA_PAIRS = [("fcc_cu", (2, 2, 2)), ("fcc_cu", (-1, 0, 0)), ("fcc_cu", (2, 2, 1)), ("bcc_fe", (2, 1, 0)), ("bcc_fe", (2, 1, 1)),
               ("cscl", (2, 1, 0)), ("cscl", (0, 0, -1)), ("cu3au", (2, 1, 0)), ("cu3au", (2, 1, 1)), ("hcp_mg", (1, 0, 1)),
               ("hcp_mg", (1, 1, 0)), ("hcp_mg", (0, 1, 0)), ("triclinic", (0, 1, 0)), ("triclinic", (0, 0, 1)), ("triclinic", (1, 1, 0)),
               ("triclinic", (0, -1, 1)), ("tetragonal", (1, 0, 1))]
# (operations, indices at max_miller 1, at 2)
MILLER_TABLE = {"fcc_cu": (48, 3, 6), "bcc_fe": (48, 3, 6), "cscl": (48, 3, 6), "cu3au": (48, 3, 6), "hcp_mg": (24, 5, 12),
                "tetragonal": (16, 5, 12), "triclinic": (1, 13, 49)}


def _clear(value, bound, margin, what):
    """The margin assertion: ``value`` is not within ``margin`` of ``bound``."""
    assert abs(value - bound) > margin, f"{what}: {value!r} is within {margin} of {bound!r}: the case sits on a rounding"


def _grid(box):
    r = np.arange(-box, box + 1)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def _lex_greatest(vs):
    return max((tuple(int(x) for x in v) for v in vs))


def _pick_shortest(vs, len2, scale, what):
    """The vectors of the least ``len2``; those within TIE * scale tie; margins: nothing between 1e-3 TIE and 1e3 TIE away."""
    lo = len2.min()
    tied = len2 <= lo + TIE * scale
    near = (len2 > lo + 1e-3 * TIE * scale) & (len2 <= lo + 1e3 * TIE * scale)
    assert not near.any(), f"{what}: a length tie within 1e-9 that the tie rule does not decide"
    return vs[tied]


def oriented_cell(cell, h):
    """(h reduced, u1, u2, u3, d, frame rows ex ey ez) by search."""
    h = np.asarray(h, np.int64)
    g = math.gcd(math.gcd(abs(int(h[0])), abs(int(h[1]))), abs(int(h[2])))
    if g == 0:
        raise ValueError("Miller index (0,0,0)")
    h = h // g
    if not np.linalg.det(cell) > 0:
        raise ValueError("singular or left-handed cell")
    L2 = (cell ** 2).sum(1).max()
    G = _grid(BOX)
    plane = G[(G @ h == 0) & (np.abs(G).sum(1) > 0)]
    pc = plane @ cell
    u1 = np.array(_lex_greatest(_pick_shortest(plane, (pc ** 2).sum(1), L2, "u1")))
    u1c = u1 @ cell
    ok = (np.cross(u1, plane) == h).all(1)
    cand, cc = plane[ok], pc[ok]
    dots = cc @ u1c / (u1c @ u1c)
    for t in dots:
        assert abs(t) < 1e-12 or abs(t - TIE) > 1e-7, "u2: u1.v sits on the obtuse bound"
    keep = dots <= TIE
    cand, cc = cand[keep], cc[keep]
    u2 = cand[np.argmin((cc ** 2).sum(1))]
    u2c = u2 @ cell
    n = np.cross(u1c, u2c)
    n /= np.linalg.norm(n)
    ex = u1c / np.linalg.norm(u1c)
    ey = np.cross(n, ex)
    up = G[G @ h == 1]
    uc = up @ cell
    inpl = uc - np.outer(uc @ n, n)
    u3 = np.array(_lex_greatest(_pick_shortest(up, (inpl ** 2).sum(1), L2, "u3")))
    assert np.abs(u1).max() < BOX and np.abs(u2).max() < BOX and np.abs(u3).max() < BOX, "search box too small"
    assert round(np.linalg.det(np.stack([u1, u2, u3]))) == 1
    d = float((u3 @ cell) @ n)
    recip = np.linalg.inv(cell).T
    assert abs(d - 1.0 / np.linalg.norm(h @ recip)) < 1e-12 * max(1.0, d)
    return h, u1, u2, u3, d, np.stack([ex, ey, n])


def _obtuse_partner(p1, v):
    k = math.floor(TIE - (p1 @ v) / (p1 @ p1))
    return v + k * p1


def _frac2(xy, c0, c1):
    f2 = xy[..., 1] / c1[1]
    f1 = (xy[..., 0] - f2 * c1[0]) / c0[0]
    return f1, f2


def _min_image_dist(dxy, c0, c1):
    """Shortest length of dxy modulo the lattice (c0, c1), over the 5 x 5 nearest images."""
    f1, f2 = _frac2(dxy, c0, c1)
    f1, f2 = f1 - np.round(f1), f2 - np.round(f2)
    best = np.full(np.shape(f1), np.inf)
    for i, j in itertools.product(range(-2, 3), repeat=2):
        x = (f1 + i) * c0[0] + (f2 + j) * c1[0]
        y = (f2 + j) * c1[1]
        best = np.minimum(best, np.hypot(x, y))
    return best


def maps_onto(A, ZA, B, ZB, c0, c1, R, tau, symprec, margins=True):
    """Does (x, y) -> R (x, y) + tau, z as it is, take every atom of A onto an atom of its species of B within symprec, modulo
    (c0, c1)?  With ``margins`` the nearest distances are asserted away from symprec."""
    if len(A) != len(B):
        return False
    T = np.concatenate([A[:, :2] @ R.T + tau, A[:, 2:]], 1)
    for t, z in zip(T, ZA):
        m = ZB == z
        if not m.any():
            return False
        dz = t[2] - B[m, 2]
        dist = np.hypot(_min_image_dist(t[:2] - B[m, :2], c0, c1), dz)
        near = dist.min()
        if margins:
            _clear(near, symprec, 1e-6, "a pair distance")
        if near > symprec:
            return False
    return True


def point_operations(c0, c1, symprec):
    """(W, R) of the lattice (c0, c1): integer W, entries -2 .. 2, det +-1, that keep |c0|, |c1|, |c0 + c1| within symprec."""
    M = np.array([[c0[0], c1[0]], [c0[1], c1[1]]])
    l = [np.linalg.norm(c0), np.linalg.norm(c1), np.linalg.norm(c0 + c1)]
    out = []
    for w in itertools.product(range(-2, 3), repeat=4):
        W = np.array(w, np.float64).reshape(2, 2)
        if round(np.linalg.det(W)) not in (1, -1):
            continue
        C = M @ W
        m = [np.linalg.norm(C[:, 0]), np.linalg.norm(C[:, 1]), np.linalg.norm(C[:, 0] + C[:, 1])]
        err = max(abs(a - b) for a, b in zip(m, l))
        _clear(err, symprec, 1e-6, "a lattice length")
        if err <= symprec:
            out.append((np.array(w).reshape(2, 2), C @ np.linalg.inv(M)))
    return out


def equivalent(A, ZA, B, ZB, c0, c1, ops, symprec, mirror=False):
    """Step 5 (step 6 with ``mirror``): slabs given in a common frame, compared about their mid-planes."""
    A, B = A.copy(), B.copy()
    A[:, 2] -= 0.5 * (A[:, 2].min() + A[:, 2].max())
    B[:, 2] -= 0.5 * (B[:, 2].min() + B[:, 2].max())
    if mirror:
        A[:, 2] = -A[:, 2]
    for _, R in ops:
        for q in np.nonzero(ZB == ZA[0])[0]:
            tau = B[q, :2] - R @ A[0, :2]
            if maps_onto(A, ZA, B, ZB, c0, c1, R, tau, symprec):
                return True
    return False


def order_atoms(f1, f2, z, symprec):
    """The contract's atom order: the position of an atom is the number of atoms that precede it."""
    n = len(z)
    rank = np.zeros(n, np.int64)
    for i in range(n):
        for k in range(n):
            if k == i:
                continue
            if abs(z[k] - z[i]) > symprec:
                _clear(abs(z[k] - z[i]), symprec, 1e-6, "a layer distance")
                before = z[k] < z[i]
            elif abs(f1[k] - f1[i]) > FTOL:
                _clear(abs(f1[k] - f1[i]), FTOL, 1e-8, "a fractional coordinate")
                before = f1[k] < f1[i]
            elif abs(f2[k] - f2[i]) > FTOL:
                _clear(abs(f2[k] - f2[i]), FTOL, 1e-8, "a fractional coordinate")
                before = f2[k] < f2[i]
            else:
                before = k < i
            rank[i] += before
    assert sorted(rank.tolist()) == list(range(n))
    return np.argsort(rank)


def _wrap(f):
    w = f - np.floor(f + FTOL)
    for v in np.atleast_1d(w):
        _clear(v, 1.0 - FTOL, 1e-8, "a wrapped coordinate")
        _clear(v, -FTOL, 1e-8, "a wrapped coordinate")
    return w


def _finish(xyz, Z, c0, c1, height, symprec):
    """Centre, wrap and order a slab given in its output frame; returns pos, Z."""
    z = xyz[:, 2] - 0.5 * (xyz[:, 2].min() + xyz[:, 2].max()) + 0.5 * height
    f1, f2 = _frac2(xyz[:, :2], c0, c1)
    f1, f2 = _wrap(f1), _wrap(f2)
    o = order_atoms(f1, f2, z, symprec)
    pos = np.stack([f1 * c0[0] + f2 * c1[0], f2 * c1[1], z], 1)
    return pos[o], Z[o]


def cut_slabs(bulk, h, min_slab_size=7.0, min_vacuum_size=20.0, tol=0.3, symprec=1e-3):
    """The slabs of one (bulk, h) in the contract's order: a list of dicts (pos, Z, cell, millers, shift, top) and a record
    of the intermediate facts (d, n_slab, cuts, kept, translations, frame, gaps ...)."""
    cell, pos, Z = bulk["cell"], bulk["pos"], bulk["Z"]
    for name, v in (("min_slab_size", min_slab_size), ("min_vacuum_size", min_vacuum_size), ("tol", tol), ("symprec", symprec)):
        if not (0.0 < float(v) < math.inf):
            raise ValueError(f"{name} = {v}: finite and positive expected")
    hr, u1, u2, u3, d, F = oriented_cell(cell, h)
    L2 = (cell ** 2).sum(1).max()
    for v, name in ((min_slab_size / d, "min_slab_size / d"), (min_vacuum_size / d, "min_vacuum_size / d")):
        _clear(v, round(v), 1e-9, name)
    n_slab, n_vac = math.ceil(min_slab_size / d), math.ceil(min_vacuum_size / d)
    height = (n_slab + n_vac) * d
    # cut planes from the sorted heights modulo d
    hs = np.sort((pos @ F[2]) % d)
    gaps = np.append(np.diff(hs), hs[0] + d - hs[-1])
    for gp in gaps:
        _clear(gp, tol, 1e-6, "a height gap")
    def plane(i):
        # in [0, d); a plane within 1e-9 A of d is the plane at 0
        mid = float(hs[i] + 0.5 * gaps[i])
        assert abs(mid - d) < 1e-12 or abs(mid - (d - 1e-9)) > 1e-7, "a cut plane sits on the wrap"
        return max(mid - d, 0.0) if mid >= d - 1e-9 else mid

    if (gaps > tol).any():
        shifts = sorted(plane(i) for i in np.nonzero(gaps > tol)[0])
    else:
        srt = np.sort(gaps)
        assert len(srt) < 2 or srt[-1] - srt[-2] > 1e-6, "largest gap tied"
        i = int(np.argmax(gaps))
        shifts = [plane(i)]
    # a block of periodic images in the frame of u1
    G = _grid(IMAGES)
    img = (pos[None, :, :] + (G @ cell)[:, None, :]).reshape(-1, 3) @ F.T
    imgZ = np.tile(Z, len(G))
    c0 = np.array([np.linalg.norm(u1 @ cell), 0.0])
    c1 = np.array([(u2 @ cell) @ F[0], (u2 @ cell) @ F[1]])

    def slab_of(shift, a0, a1):
        """Atoms above the plane within the in-plane cell (a0, a1), heights from the plane."""
        zz = img[:, 2] - shift
        m = (zz >= 0) & (zz < n_slab * d)
        for v in zz[(zz > -0.1) & (zz < 0.1)]:
            _clear(v, 0.0, 1e-6, "an atom on the cut plane")
        M = np.array([[a0[0], a1[0]], [a0[1], a1[1]]])
        f = np.linalg.solve(M, img[m, :2].T).T
        inside = ((f >= -FTOL) & (f < 1 - FTOL)).all(1)
        out = np.concatenate([img[m][inside, :2], zz[m][inside, None]], 1)
        return out, imgZ[m][inside]

    # in-plane translations of the slab (first cut), every candidate from atom 0
    A, ZA = slab_of(shifts[0], c0, c1)
    assert len(A) == n_slab * len(Z), "image block too small"
    ident = np.eye(2)
    trans = []
    for q in np.nonzero(ZA == ZA[0])[0][1:]:
        if abs(A[q, 2] - A[0, 2]) > symprec:
            continue
        t = A[q, :2] - A[0, :2]
        if _min_image_dist(t, c0, c1) > symprec and maps_onto(A, ZA, A, ZA, c0, c1, ident, t, symprec):
            trans.append(t)
    k = len(trans) + 1
    p1, p2 = c0.copy(), c1.copy()
    if trans:
        pts = []
        for t in [np.zeros(2)] + trans:
            f1, f2 = _frac2(t, c0, c1)
            f1, f2 = f1 - round(f1), f2 - round(f2)
            pts += [(f1 + i) * c0 + (f2 + j) * c1 for i, j in itertools.product(range(-2, 3), repeat=2)]
        pts = np.array([p for p in pts if np.linalg.norm(p) > 1e-6])
        short = _pick_shortest(pts, (pts ** 2).sum(1), L2, "p1")
        tx = 1e-9 * math.sqrt(L2)
        p1 = short[0]
        for v in short[1:]:
            if v[0] > p1[0] + tx or (abs(v[0] - p1[0]) <= tx and v[1] > p1[1] + tx):
                p1 = v
        want = c0[0] * c1[1] / k
        dets = p1[0] * pts[:, 1] - p1[1] * pts[:, 0]
        cand = pts[np.abs(dets - want) < 1e-6 * want]
        cand = np.array([_obtuse_partner(p1, v) for v in cand])
        assert np.ptp(cand, 0).max() < 1e-9
        p2 = cand[0]
    # the frame turned onto p1
    co, si = p1 / np.linalg.norm(p1)
    T = np.array([[co, si], [-si, co]])
    F2 = np.concatenate([T @ F[:2], F[2:]], 0)
    img[:, :2] = img[:, :2] @ T.T
    c0 = np.array([np.linalg.norm(p1), 0.0])
    c1 = T @ p2
    assert c0[0] <= np.linalg.norm(c1) + 1e-9 and c0 @ c1 <= TIE * c0[0] ** 2 and c1[1] > 0
    ops = point_operations(c0, c1, symprec)
    raw = [slab_of(s, c0, c1) for s in shifts]
    kept, invertible = [], []
    for i, (A, ZA) in enumerate(raw):
        assert len(A) * k == n_slab * len(Z)
        if any(equivalent(raw[j][0], raw[j][1], A, ZA, c0, c1, ops, symprec) for j in kept):
            continue
        kept.append(i)
        invertible.append(equivalent(A, ZA, A, ZA, c0, c1, ops, symprec, mirror=True))
    slabs = []
    cellT = np.array([[c0[0], 0, 0], [c1[0], c1[1], 0], [0, 0, height]])
    for i in kept:
        p, z = _finish(raw[i][0], raw[i][1], c0, c1, height, symprec)
        slabs.append({"pos": p, "Z": z, "cell": cellT.copy(), "millers": tuple(int(x) for x in hr), "shift": shifts[i], "top": True})
    f1 = _obtuse_partner(c0, np.array([-c1[0], c1[1]]))
    cellF = np.array([[c0[0], 0, 0], [f1[0], f1[1], 0], [0, 0, height]])
    for i, inv in zip(kept, invertible):
        if inv:
            continue
        xyz = raw[i][0] * np.array([1.0, -1.0, -1.0])
        p, z = _finish(xyz, raw[i][1], c0, f1, height, symprec)
        slabs.append({"pos": p, "Z": z, "cell": cellF.copy(), "millers": tuple(int(x) for x in hr), "shift": shifts[i], "top": False})
    facts = {"d": d, "n_slab": n_slab, "n_vac": n_vac, "cuts": len(shifts), "kept": len(kept), "translations": k, "frame": F2,
             "max_gap": float(gaps.max()), "u": (u1, u2, u3), "layers": None, "ops": ops}
    return slabs, facts


def count_layers(slab, symprec=1e-3):
    z = np.sort(slab["pos"][:, 2])
    return 1 + int((np.diff(z) > symprec).sum())


# ---- invariants (a)-(g) of one slab; `facts` from cut_slabs of the same (bulk, h), `partner`: the top slab of a flipped one
def check_invariants(bulk, slab, facts, min_slab_size=7.0, min_vacuum_size=20.0, symprec=1e-3, partner=None):
    cell, pos, Z = slab["cell"], slab["pos"], slab["Z"]
    d, n_slab, k, F = facts["d"], facts["n_slab"], facts["translations"], facts["frame"]
    V = np.linalg.det(bulk["cell"])
    # (f) the cell
    assert cell[2, 0] == 0 and cell[2, 1] == 0 and cell[2, 2] > 0 and cell[0, 1] == 0 and cell[0, 2] == 0 and cell[1, 2] == 0
    assert np.linalg.det(cell) > 0, "left-handed"
    assert np.linalg.norm(cell[0]) <= np.linalg.norm(cell[1]) * (1 + 1e-12) and cell[0] @ cell[1] <= 1e-9 * (cell[0] @ cell[0])
    # (b), (c)
    assert len(pos) * k == n_slab * len(bulk["Z"]), "(b) atom count"
    assert abs(cell[0, 0] * cell[1, 1] * d * k - V) < 1e-9 * V, "(c) area"
    # (d), (e)
    thick = pos[:, 2].max() - pos[:, 2].min()
    assert thick >= min_slab_size - facts["max_gap"] - 1e-9, "(d) thickness"
    assert cell[2, 2] - thick >= min_vacuum_size - 1e-9, "(e) vacuum"
    assert abs(0.5 * (pos[:, 2].max() + pos[:, 2].min()) - 0.5 * cell[2, 2]) < 1e-9, "centred"
    f1, f2 = _frac2(pos[:, :2], cell[0, :2], cell[1, :2])
    assert (f1 >= -FTOL - 1e-9).all() and (f1 < 1).all() and (f2 >= -FTOL - 1e-9).all() and (f2 < 1).all(), "wrapped"
    # (a) back through the rotation (a flipped slab is turned back first): every atom on a bulk site of its species
    xyz = pos.copy()
    if not slab["top"]:
        xyz = xyz * np.array([1.0, -1.0, -1.0])
    inv = np.linalg.inv(bulk["cell"])
    on_site = False
    for j in np.nonzero(bulk["Z"] == Z[0])[0]:
        r = (xyz - xyz[0]) @ F + bulk["pos"][j]
        good = True
        for ri, zi in zip(r, Z):
            df = (ri - bulk["pos"][bulk["Z"] == zi]) @ inv
            good = good and bool(np.abs(df - np.round(df)).max(1).min() < 1e-7)
        on_site = on_site or good
    assert on_site, "(a) an atom off the bulk's sites"
    # (g) turned back (the flip undone) it is its partner under the in-plane motions of step 5; as it stands it is not
    if partner is not None:
        back = pos * np.array([1.0, -1.0, -1.0])
        pops = point_operations(partner["cell"][0, :2], partner["cell"][1, :2], symprec)
        assert equivalent(back, Z, partner["pos"], partner["Z"], partner["cell"][0, :2], partner["cell"][1, :2], pops, symprec), \
            "(g) mirrored back it is not its partner"
        assert not equivalent(pos, Z, partner["pos"], partner["Z"], partner["cell"][0, :2], partner["cell"][1, :2], pops, symprec), \
            "(g) equal to its partner before mirroring"


# ---- distinct Miller indices
def point_group(bulk, symprec=1e-3):
    """The integer matrices W, entries in {-1, 0, 1}, whose rows sum_j W_ij a_j keep the edges' and face diagonals' lengths and
    under which f -> f W + t maps the atoms onto themselves for some t."""
    cell, pos, Z = bulk["cell"], bulk["pos"], bulk["Z"]
    if not np.linalg.det(cell) > 0:
        raise ValueError("singular or left-handed cell")
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]

    def lengths(c):
        return np.array([np.linalg.norm(c[i] if i == j else c[i] + c[j]) for i, j in pairs])

    ref = lengths(cell)
    W = np.array(list(itertools.product((-1, 0, 1), repeat=9))).reshape(-1, 3, 3)
    B = W @ cell
    L = np.stack([np.linalg.norm(B[:, i] if i == j else B[:, i] + B[:, j], axis=1) for i, j in pairs], 1)
    err = np.abs(L - ref).max(1)
    assert not ((err > symprec - 1e-6) & (err < symprec + 1e-6)).any()
    frac = pos @ np.linalg.inv(cell)
    ops = []
    for w in W[err <= symprec]:
        g = frac @ w
        found = False
        for j in np.nonzero(Z == Z[0])[0]:
            t = frac[j] - g[0]
            ok = True
            for gi, zi in zip(g + t, Z):
                df = gi - frac[Z == zi]
                dist = np.linalg.norm((df - np.round(df)) @ cell, axis=1).min()
                _clear(dist, symprec, 1e-6, "a pair distance")
                ok = ok and dist <= symprec
            if ok:
                found = True
                break
        if found:
            ops.append(w)
    return ops


def distinct_millers(bulk, max_miller=2, symprec=1e-3):
    """(indices in descending lexicographic order, order of the point group)."""
    if not 1 <= max_miller <= 4:
        raise ValueError(f"max_miller = {max_miller}: 1 .. 4 expected")
    ops = point_group(bulk, symprec)
    r = range(max_miller, -max_miller - 1, -1)
    out = []
    for h in itertools.product(r, repeat=3):
        if h == (0, 0, 0) or math.gcd(math.gcd(abs(h[0]), abs(h[1])), abs(h[2])) != 1:
            continue
        orbit = {tuple(int(x) for x in s * (w @ np.array(h))) for w in ops for s in (1, -1)}
        orbit = {g for g in orbit if max(abs(x) for x in g) <= max_miller}
        if max(orbit) == h:
            out.append(h)
    return out, len(ops)


def all_pairs():
    """The device batch: every (crystal, h) of the case table and the further pairs, grouped by crystal in a fixed order."""
    names = list(crystals())
    pairs = [(c[0], c[1]) for c in CASE_TABLE] + EXTRA_PAIRS
    return names, sorted(pairs, key=lambda p: names.index(p[0]))
