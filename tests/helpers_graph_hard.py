"""Hard cells for the radius graph (csrc/graph.hip) and a float64 brute-force checker with a stated rounding band.

Pure torch / numpy, no GPU.  ``case(name)`` builds the inputs of one row of the table in DESIGN.md ("graph on hard
cells"); ``check_directed`` judges a directed strict top-K list (the oracle's or the device's) against all n x C
candidate d^2 in float64; ``check_symmetrised`` rebuilds the symmetrised CSR from the same directed lists and judges
the exported edges.  On general cells "the oracle's bits" is not a target (``offsets_exact``), hence the band

    tau(v) = 8 sqrt(v) u + 4 * 2^-24 v,     u = 2^-23 (max|pos| + max|offset|) of the system:

four float32 roundings on a coordinate difference (two in the offset chain, one in p_j + off, one in the subtraction)
with a factor two to spare, plus squaring and summing.  A centre with a candidate within tau of rc^2 or of 1e-4 is a
*boundary centre*: its count may differ by the number of such candidates.  At most 5 % of a case's centres may be
boundary centres (MAX_BOUNDARY_SHARE); a case that has more gets another seed, never another rule.
"""
from collections import namedtuple

import numpy as np
import torch

from adsorbdiff_amd.data import Batch, Data
from oracle import painn_oracle as O
from tests.helpers import batch_from_fixture, load_npz

Case = namedtuple("Case", "batch cutoff K pbc")
MAX_BOUNDARY_SHARE = 0.05
D2_FLOOR = 1e-4
ALL = (True, True, True)


def skew(a, c):
    """The project's cell shape (synthetic.make_system) at any size."""
    return torch.tensor([[a, 0.0, 0.0], [0.3 * a, 0.95 * a, 0.0], [0.0, 0.0, c]], dtype=torch.float32)


def triclinic(a=4.0, c=6.0):
    """All nine entries non-zero."""
    return torch.tensor([[a, 0.1 * a, -0.2 * a], [-0.45 * a, 0.9 * a, 0.15 * a], [0.2 * c, -0.1 * c, c]], dtype=torch.float32)


def _lin(coef, cell):
    """coef (row vectors) . cell in float64, as an elementwise chain: a matrix product's bits depend on the CPU it runs on
    (a lattice built with one gave other ties on another machine)."""
    coef, cell = coef.double(), cell.double().reshape(3, 3)
    return coef[:, 0:1] * cell[0] + coef[:, 1:2] * cell[1] + coef[:, 2:3] * cell[2]


def _system(gen, cell, n, sid="0", extra=None):
    """n atoms uniform in fractional coordinates times the cell (+ rows of ``extra``)."""
    frac = torch.rand(n, 3, generator=gen, dtype=torch.float64)
    pos = _lin(frac, cell).float()
    if extra is not None:
        pos = torch.cat([pos, extra.float()])
    n = pos.shape[0]
    return Data(pos=pos, atomic_numbers=torch.randint(1, 80, (n,), generator=gen).float(), tags=torch.ones(n, dtype=torch.long),
                fixed=torch.zeros(n, dtype=torch.long), cell=cell.reshape(1, 3, 3).clone(), natoms=torch.tensor([n]), sid=sid)


def _batch(systems, pbc=ALL):
    b = Batch.from_data_list(systems)
    if tuple(pbc) != ALL:
        b.pbc = torch.tensor([list(pbc)] * len(systems), dtype=torch.bool)
    return b


# name -> (cell, atoms, cutoff, K, pbc, default seed).  Seeds: the first one (from 0) with at most 5 % boundary centres
# and, for near_cap / overflow, the candidate counts the table names.
_SIMPLE = {
    "uncached147": (skew(4.3, 35.0), 8, 12.0, 50, ALL, 0),
    "bulk343": (skew(4.3, 5.5), 5, 12.0, 50, ALL, 0),
    "bulk343_k128": (skew(4.3, 5.5), 10, 12.0, 128, ALL, 0),
    "near_cap": (skew(4.3, 5.5), 12, 12.0, 50, ALL, 0),
    "overflow": (skew(4.3, 5.5), 16, 12.0, 50, ALL, 0),
    "triclinic245": (triclinic(), 7, 10.0, 40, ALL, 0),
    "k64": (skew(4.3, 35.0), 10, 12.0, 64, ALL, 0),
    "k65": (skew(4.3, 35.0), 10, 12.0, 65, ALL, 0),
    "k1": (skew(4.3, 35.0), 10, 12.0, 1, ALL, 0),
    "pbc_ttf": (skew(4.3, 9.0), 9, 12.0, 50, (True, True, False), 0),
    "pbc_tff": (skew(4.3, 9.0), 12, 12.0, 50, (True, False, False), 0),
    "pbc_fff": (skew(9.0, 9.0), 40, 6.0, 20, (False, False, False), 0),
}
CASES = tuple(_SIMPLE) + ("unwrapped147", "seam256", "one_atom", "close_pair", "tie")
# close_pair: atoms 8 / 9 are 0.009 A apart (below the d^2 > 1e-4 floor), atoms 10 / 11 are 0.011 A apart (above it)
CLOSE_PAIRS = ((8, 9, 0.009), (10, 11, 0.011))


def case(name, seed=None):
    """-> Case(batch, cutoff, K, pbc) of one row of the case table."""
    if name in _SIMPLE:
        cell, n, cutoff, K, pbc, s0 = _SIMPLE[name]
        gen = torch.Generator().manual_seed(s0 if seed is None else seed)
        return Case(_batch([_system(gen, cell, n, name)], pbc), cutoff, K, pbc)
    # unwrapped147: hops of two 35 A vectors put coordinates near 100 A, where the float32 difference pos[j] - pos[i] (the
    # reference's own first operation) alone rounds by up to 3.8e-6; seed 4 is the first one at which the float32 oracle
    # holds check_symmetrised's 2e-6 on dist with 1e-6 (one ulp of a 12 A distance) to spare for the rounding of the norm
    # (oracle: 7.1e-7; seeds 0-3: 2.3e-6, 1.5e-6, 1.9e-6, 1.8e-6)
    gen = torch.Generator().manual_seed((4 if name == "unwrapped147" else 0) if seed is None else seed)
    cell = skew(4.3, 35.0)
    if name == "unwrapped147":   # atoms drawn as in uncached147, each then moved by integer lattice vectors in [-2, 2]
        d = _system(gen, cell, 8, name)
        hop = torch.randint(-2, 3, (8, 3), generator=gen).double()
        d.pos = (d.pos.double() + _lin(hop, cell)).float()
        return Case(_batch([d]), 12.0, 50, ALL)
    if name == "seam256":        # the small cell sets the batch-wide reps: the big systems run C = 147 too
        big = skew(16.0, 35.0)
        return Case(_batch([_system(gen, cell, 8, "s8"), _system(gen, big, 256, "s256"), _system(gen, big, 257, "s257")]),
                    12.0, 50, ALL)
    if name == "one_atom":
        return Case(_batch([_system(gen, cell, 1, "one"), _system(gen, cell, 6, "six")]), 12.0, 50, ALL)
    if name == "close_pair":
        base = _lin(torch.rand(2, 3, generator=gen, dtype=torch.float64), cell)
        dirs = torch.nn.functional.normalize(torch.randn(2, 3, generator=gen, dtype=torch.float64), dim=1)
        extra = torch.stack([base[0], base[0] + CLOSE_PAIRS[0][2] * dirs[0], base[1], base[1] + CLOSE_PAIRS[1][2] * dirs[1]])
        return Case(_batch([_system(gen, cell, 8, name, extra=extra)]), 12.0, 50, ALL)
    if name == "tie":            # the perfect lattice of graph_tie.npz (oracle/make_golden.py): exact ties at the K-th place
        fx = load_npz("graph_tie.npz")
        return Case(batch_from_fixture(fx), float(fx["cutoff"]), int(fx["K"]), ALL)
    raise KeyError(name)


def _f32(x):
    return torch.as_tensor(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)).to(torch.float32)


def _np(x, dtype):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x).astype(dtype)


def shift_tables(cell, cutoff, pbc):
    """(reps, integer shift table [C, 3]) exactly as the engine and the oracle form them (float32 cell)."""
    reps = O.cell_repeats(_f32(cell).reshape(-1, 3, 3), float(cutoff), pbc)
    return reps, O.shift_table(reps).numpy().astype(np.int64)


def _offset_chains(c):
    """float32 offsets [B, 3, C] of a case: torch.bmm as the oracle calls it, the unfused chain (t0 + t1) + t2 of graph.hip,
    and the same three rounded products summed as t0 + (t1 + t2)."""
    cell = c.batch.cell.reshape(-1, 3, 3).float()
    _, sh = shift_tables(cell, c.cutoff, c.pbc)
    s = torch.from_numpy(sh).float()
    B, C = cell.shape[0], s.shape[0]
    bmm = torch.bmm(cell.transpose(1, 2), s.t().reshape(1, 3, C).expand(B, -1, -1)).numpy()
    cl, sn = cell.numpy(), s.numpy()
    chain, other = np.empty_like(bmm), np.empty_like(bmm)
    for k in range(3):
        t0, t1, t2 = (cl[:, x, k, None] * sn[None, :, x] for x in range(3))
        chain[:, k, :] = (t0 + t1) + t2
        other[:, k, :] = t0 + (t1 + t2)
    assert chain.dtype == np.float32 and other.dtype == np.float32
    return bmm, chain, other


def offsets_exact(c):
    """Does the oracle's (and the reference's) torch.bmm, on the CPU this runs on, give the bits of the unfused float32 chain
    (c0k sa + c1k sb) + c2k sc that graph.hip evaluates, for every offset of the case?  Where it does not, the oracle's
    lists are not the device's target."""
    bmm, chain, _ = _offset_chains(c)
    return bool(np.array_equal(bmm, chain))


def offsets_order_dependent(c):
    """Number of offset elements whose bits depend on the order in which the three rounded products are summed.  None on
    the project's cell shape (every component has at most two non-zero products), so there any in-order or reordered
    float32 product sum gives the kernel's bits; hundreds on a cell with nine non-zero entries, where torch.bmm's bits
    are a property of the CPU."""
    _, chain, other = _offset_chains(c)
    return int((chain != other).sum())


def oracle_graph(c):
    """The float32 oracle's graph of a case in the device's export layout: dict(cnt [N], src [N, K] (-1 beyond cnt),
    shift [N, K, 3], es, ed, dist, vec) with the symmetrised edges in CSR order (target, distance, source)."""
    b = c.batch
    pos, cell, natoms = b.pos.float(), b.cell.reshape(-1, 3, 3).float(), b.natoms
    ei0, sh0, nb0 = O.radius_graph_pbc(pos, cell, natoms, c.cutoff, c.K, c.pbc)
    if tuple(c.pbc) == ALL:
        ei, _, d, u = O.generate_graph_values(pos, cell, natoms, c.cutoff, c.K)
    else:   # generate_graph_values has no pbc argument: its stages one by one (no distance reaches the 1e-3 clamp)
        ei, d, v, _ = O.pbc_distances(pos, ei0, cell, sh0, nb0)
        ei, _, _, d, u = O.symmetrize_edges(ei, sh0, nb0, d, v / d[:, None])
    N = pos.shape[0]
    cnt = np.bincount(ei0[1].numpy(), minlength=N).astype(np.int32)
    src = np.full((N, c.K), -1, np.int32)
    shift = np.zeros((N, c.K, 3), np.int32)
    slot = np.arange(ei0.shape[1]) - np.repeat(np.cumsum(cnt) - cnt, cnt)     # centres come in ascending order
    assert np.all(np.diff(ei0[1].numpy()) >= 0)
    src[ei0[1].numpy(), slot] = ei0[0].numpy()
    shift[ei0[1].numpy(), slot] = sh0.numpy().astype(np.int32)
    es, ed, d, u = ei[0].numpy(), ei[1].numpy(), d.numpy(), u.numpy()
    order = np.lexsort((es, d, ed))
    return dict(cnt=cnt, src=src, shift=shift, es=es[order].astype(np.int32), ed=ed[order].astype(np.int32), dist=d[order],
                vec=u[order])


def tau(v, u):
    return 8.0 * np.sqrt(v) * u + 4.0 * 2.0 ** -24 * v


def candidate_d2(pos, cell, natoms, cutoff, pbc, b, centres=None):
    """float64 d^2 [m, n * C] of every candidate (atom j of system b, shift c), index j * C + c, for the listed centres
    (local indices; default all), and the band unit u of the system."""
    pos, cell = _np(pos, np.float64), _np(cell, np.float64).reshape(-1, 3, 3)
    natoms = _np(natoms, np.int64).reshape(-1)
    _, sh = shift_tables(cell, cutoff, pbc)
    a0, n = int(natoms[:b].sum()), int(natoms[b])
    P = pos[a0:a0 + n]
    off = sh.astype(np.float64) @ cell[b]                                      # [C, 3]: shift (row vector) . cell
    u = 2.0 ** -23 * (np.abs(P).max() + np.abs(off).max())
    Pi = P if centres is None else P[np.asarray(centres)]
    diff = Pi[:, None, None, :] - (P[None, :, None, :] + off[None, None, :, :])
    return (diff * diff).sum(-1).reshape(Pi.shape[0], -1), u


def check_directed(pos, cell, natoms, cutoff, K, pbc, cnt, src, shift, stats=None):
    """Rules 1-4 of the module docstring's band on directed lists (cnt [N], src [N, K], shift [N, K, 3]); AssertionError
    names the centre.  Returns the share of boundary centres; ``stats`` (a dict) also receives ``worst`` = max
    |d^2 - expected| / tau over the compared places, ``boundary`` [N] bool and ``in_range`` [N] (candidates per centre)."""
    natoms = _np(natoms, np.int64).reshape(-1)
    cnt, src, shift = _np(cnt, np.int64), _np(src, np.int64), _np(shift, np.int64)
    reps, sh = shift_tables(cell, cutoff, pbc)
    C = sh.shape[0]
    n1, n2 = 2 * reps[1] + 1, 2 * reps[2] + 1
    rc2 = float(cutoff) ** 2
    N = int(natoms.sum())
    assert cnt.shape == (N,) and src.shape == (N, K) and shift.shape == (N, K, 3)
    boundary, in_range, worst = np.zeros(N, bool), np.zeros(N, np.int64), 0.0
    a0 = 0
    for b, n in enumerate(natoms.tolist()):
        chunk = max(1, (1 << 22) // max(1, n * C))
        for i0 in range(0, n, chunk):
            loc = np.arange(i0, min(n, i0 + chunk))
            d2, u = candidate_d2(pos, cell, natoms, cutoff, pbc, b, loc)
            t_hi, t_lo = tau(rc2, u), tau(D2_FLOOR, u)
            for r, il in enumerate(loc):
                i, row = a0 + int(il), d2[r]
                k = int(cnt[i])
                assert 0 <= k <= K, f"centre {i}: count {k}"
                js, ss = src[i, :k], shift[i, :k]
                # 1. own system, inside the table, distinct
                assert np.all((js >= a0) & (js < a0 + n)), f"centre {i}: a source outside its system"
                assert np.all(np.abs(ss) <= np.asarray(reps)[None, :]), f"centre {i}: a shift outside the table"
                ids = (js - a0) * C + ((ss[:, 0] + reps[0]) * n1 + (ss[:, 1] + reps[1])) * n2 + (ss[:, 2] + reps[2])
                assert np.unique(ids).size == k, f"centre {i}: a candidate listed twice"
                # 2. in range up to the band
                S = np.sort(row[ids])
                assert np.all(S > D2_FLOOR - t_lo) and np.all(S <= rc2 + t_hi), f"centre {i}: a listed candidate out of range"
                band = (np.abs(row - rc2) <= t_hi) | (np.abs(row - D2_FLOOR) <= t_lo)
                nb = int(band.sum())
                inr = (row > D2_FLOOR) & (row <= rc2)
                in_range[i] = int(inr.sum())
                if nb == 0:
                    # 3. the K nearest, as a distance multiset
                    T = np.sort(row[inr])[:K]
                    assert S.size == T.size, f"centre {i}: {S.size} listed, {T.size} expected"
                else:
                    # 4. the same without the in-band candidates; the count may differ by their number
                    boundary[i] = True
                    T = np.sort(row[inr & ~band])
                    S = S[(np.abs(S - rc2) > t_hi) & (np.abs(S - D2_FLOOR) > t_lo)]
                    want = min(K, T.size)
                    assert want - nb <= S.size <= want, f"boundary centre {i}: {S.size} listed, {want} expected, {nb} in band"
                    T = T[:S.size]
                if S.size:
                    ratio = np.abs(S - T) / tau(T, u)
                    worst = max(worst, float(ratio.max()))
                    assert ratio.max() <= 1.0, (f"centre {i}: place {int(ratio.argmax())} has d^2 {S[ratio.argmax()]!r}, the "
                                                f"float64 search {T[ratio.argmax()]!r}: {ratio.max():.3g} tau")
        a0 += n
    if stats is not None:
        stats.update(worst=worst, boundary=boundary, in_range=in_range)
    return float(boundary.mean())


def check_symmetrised(cnt, src, shift, es, ed, dist, vec, pos, cell, natoms):
    """The exported symmetrised CSR against the edge set rebuilt from the directed lists it was made from (so tie picks
    cannot matter): keep j < i, or j == i with a lexicographically negative shift, and add the reversed copy.  Same
    (source, target, image) set, E = twice the kept count; dist / vec within 2e-6 absolute of the float64 |v| and v / |v|
    of the matching image; every target's segment non-decreasing in dist, equal dist by source index; an edge and its
    reverse carry exactly negated vec and the same dist bits."""
    cnt, src, shift = _np(cnt, np.int64), _np(src, np.int64), _np(shift, np.int64)
    es, ed = _np(es, np.int64), _np(ed, np.int64)
    dist32, vec32 = _np(dist, np.float32), _np(vec, np.float32)
    pos, cell = _np(pos, np.float64), _np(cell, np.float64).reshape(-1, 3, 3)
    natoms = _np(natoms, np.int64).reshape(-1)
    N, K = src.shape
    sysof = np.repeat(np.arange(natoms.size), natoms)
    valid = np.arange(K)[None, :] < cnt[:, None]
    i = np.broadcast_to(np.arange(N)[:, None], (N, K))[valid]
    j, s = src[valid], shift[valid]
    neg = (s[:, 0] < 0) | ((s[:, 0] == 0) & (s[:, 1] < 0)) | ((s[:, 0] == 0) & (s[:, 1] == 0) & (s[:, 2] < 0))
    keep = (j < i) | ((j == i) & neg)
    i, j, s = i[keep], j[keep], s[keep]
    Ek = i.size
    assert es.size == 2 * Ek, f"{es.size} edges, {2 * Ek} expected"
    v = pos[j] - pos[i] + np.einsum("ek,ekx->ex", s.astype(np.float64), cell[sysof[i]])
    w_src, w_dst = np.concatenate([j, i]), np.concatenate([i, j])                # reversed copy of edge q: q + Ek
    w_s, w_v = np.concatenate([s, -s]), np.concatenate([v, -v])
    # the image of every exported edge: its lattice shift, recovered from its own geometry (0.5 is far from 1e-5)
    assert np.all((es >= 0) & (es < N) & (ed >= 0) & (ed < N))
    assert np.array_equal(sysof[es], sysof[ed]), "an edge between two systems"
    frac = np.einsum("ex,exk->ek", dist32[:, None].astype(np.float64) * vec32 - (pos[es] - pos[ed]),
                     np.linalg.inv(cell)[sysof[ed]])
    g_s = np.rint(frac).astype(np.int64)
    assert np.abs(frac - g_s).max(initial=0.0) < 1e-3, "an edge vector that is no lattice image of its atom pair"
    o_w = np.lexsort((w_s[:, 2], w_s[:, 1], w_s[:, 0], w_src, w_dst))
    o_g = np.lexsort((g_s[:, 2], g_s[:, 1], g_s[:, 0], es, ed))
    kw = np.column_stack([w_dst, w_src, w_s])[o_w]
    kg = np.column_stack([ed, es, g_s])[o_g]
    assert np.array_equal(kw, kg), "the exported (source, target, image) set differs from the one the lists give"
    assert Ek == 0 or np.all(np.any(np.diff(kw, axis=0) != 0, axis=1)), "an edge listed twice"
    dev = np.empty(2 * Ek, np.int64)       # expected edge -> exported edge
    dev[o_w] = o_g
    d64 = np.sqrt((w_v * w_v).sum(-1))
    err_d = np.abs(dist32[dev].astype(np.float64) - d64).max(initial=0.0)
    err_v = np.abs(vec32[dev].astype(np.float64) - w_v / d64[:, None]).max(initial=0.0)
    assert err_d <= 2e-6, f"dist off by {err_d:.3g}"
    assert err_v <= 2e-6, f"vec off by {err_v:.3g}"
    same = ed[1:] == ed[:-1]
    assert np.all(ed[1:] >= ed[:-1]), "targets out of order"
    assert np.all(~same | (dist32[1:] >= dist32[:-1])), "a segment is not ordered by distance"
    assert np.all(~(same & (dist32[1:] == dist32[:-1])) | (es[1:] >= es[:-1])), "equal distances not ordered by source"
    fw, bw = dev[:Ek], dev[Ek:]
    assert np.array_equal(vec32[fw], -vec32[bw]), "an edge and its reverse: vec not exact negatives"
    assert np.array_equal(dist32[fw].view(np.uint32), dist32[bw].view(np.uint32)), "an edge and its reverse: dist bits differ"
    return dict(E=int(es.size), err_dist=float(err_d), err_vec=float(err_v))
