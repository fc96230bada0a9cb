"""Float64 numpy oracle of the duplicate-site stage (adf_site_pair_distances, adf_unique_sites, adf_select_top_sites), written
from the contract in include/adsorbdiff_hip.h, and the generators of the tests' batches.

A case is a list of sites in the caller's order.  A site is a dict: ``pos`` [n,3] float32, ``tags`` [n], ``Z`` [n], ``cell``
[3,3] float32 (rows = lattice vectors), ``group`` (any integer id).  The oracle reads those float32 values in float64.

Tolerances.  Distances are compared within ``DIST_ATOL`` = 5e-5 A: coordinates and cell entries stay below 64 A, where the
float32 spacing is at most 3.8e-6 A, and the difference, the 3 x 3 inverse product and the back product accumulate fewer
than ten such roundings.  The convention is discontinuous where a fractional component is 0.5, and the clustering where a
distance is ``tol`` or an energy difference ``energy_tol``: ``assert_margins`` states, in float64, that a case stays clear of
all three (``SEAM_MARGIN``, ``TOL_MARGIN``, ``ENERGY_MARGIN``); then ``rep``, ``n_unique`` and ``top`` must be exactly the oracle's.
A case that violates a margin is a bug in its generator, never a reason to skip.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from adsorbdiff_amd.data import Batch, Data

DIST_ATOL = 5e-5
SEAM_MARGIN = 1e-3
TOL_MARGIN = 1e-3
ENERGY_MARGIN = 1e-4
TOL = 0.05


# ------------------------------------------------------------------------------------------------------------ the oracle
def min_diff(diff, cell):
    """scripts/eval.py:765-777 in float64 with an explicit inverse: (vectors [...,3], fractional components [...,3])."""
    frac = diff @ np.linalg.inv(cell)
    frac = frac % 1.0
    frac = frac % 1.0
    frac = np.where(frac > 0.5, frac - 1.0, frac)
    return frac @ cell, frac


def _seam(frac):
    return float(np.abs(np.abs(frac) - 0.5).min()) if frac.size else np.inf


def _layout(s):
    return (np.asarray(s["tags"], np.int64).tobytes(), np.asarray(s["Z"], np.int64).tobytes())


def group_distances(sites, include_slab=True, permutation_invariant=True):
    """([n,n] float64 matrix of one group's sites, least distance of a compared fractional component from the 0.5 seam)."""
    n = len(sites)
    D = np.zeros((n, n))
    seam = np.inf
    keys = [_layout(s) for s in sites]
    P = [np.asarray(s["pos"], np.float64) for s in sites]
    for i in range(n):
        for j in range(i + 1, n):
            if keys[j] != keys[i]:
                D[i, j] = D[j, i] = np.inf
        same = [j for j in range(i + 1, n) if keys[j] == keys[i]]
        if not same or len(P[i]) == 0:
            continue
        cell = np.asarray(sites[i]["cell"], np.float64)
        tags, Z = np.asarray(sites[i]["tags"]), np.asarray(sites[i]["Z"])
        ads = tags == 2
        B = np.stack([P[j] for j in same])                              # [m, na, 3]
        vec, frac = min_diff(B - P[i][None], cell)
        norm = np.linalg.norm(vec, axis=-1)                             # [m, na]
        d = np.zeros(len(same))
        if include_slab and (~ads).any():
            d = np.maximum(d, norm[:, ~ads].max(1))
            seam = min(seam, _seam(frac[:, ~ads]))
        if ads.any() and not permutation_invariant:
            d = np.maximum(d, norm[:, ads].max(1))
            seam = min(seam, _seam(frac[:, ads]))
        if ads.any() and permutation_invariant:
            A, Bq, Za = P[i][ads], B[:, ads], Z[ads]
            vec, frac = min_diff(Bq[:, None, :, :] - A[None, :, None, :], cell)      # [m, ka (of a), kb (of b), 3]
            nrm = np.linalg.norm(vec, axis=-1)
            same_el = Za[:, None] == Za[None, :]
            seam = min(seam, _seam(frac[:, same_el]))
            nrm = np.where(same_el[None], nrm, np.inf)
            d = np.maximum(d, np.maximum(nrm.min(2).max(1), nrm.min(1).max(1)))
        D[i, same] = d
        D[same, i] = d
    return D, seam


def regroup_numpy(group):
    """(ids ascending, members per id in the caller's order) - flag_anomaly.regroup's order."""
    group = np.asarray(group)
    ids = sorted(set(group.tolist()))
    return ids, [np.nonzero(group == g)[0] for g in ids]


def case_distances(sites, include_slab=True, permutation_invariant=True):
    """(matrices in ascending id order, the seam margin of the whole case)."""
    _, members = regroup_numpy([s["group"] for s in sites])
    out, seam = [], np.inf
    for m in members:
        D, sm = group_distances([sites[i] for i in m], include_slab, permutation_invariant)
        out.append(D)
        seam = min(seam, sm)
    return out, seam


def _valid(energy, flags, S):
    ok = np.ones(S, bool)
    if energy is not None:
        ok &= ~np.isnan(np.asarray(energy, np.float64))
    if flags is not None:
        ok &= ~np.asarray(flags).astype(bool).any(1)
    return ok


def unique_sites(matrices, group, tol, energy=None, energy_tol=None, flags=None):
    """(rep [S] in the caller's indexing, n_unique [G]) by the contract's greedy rule."""
    S = len(group)
    ids, members = regroup_numpy(group)
    ok = _valid(energy, flags, S)
    E = None if energy is None else np.asarray(energy, np.float64)
    rep = np.full(S, -1, np.int64)
    n_unique = []
    for D, m in zip(matrices, members):
        local = [k for k in range(len(m)) if ok[m[k]]]
        if E is not None:
            local.sort(key=lambda k: (E[m[k]], k))
        reps = []
        for k in local:
            fit = np.asarray([D[k, r] <= tol for r in reps], bool)
            if E is not None and energy_tol is not None and energy_tol >= 0 and reps:
                fit &= np.abs(E[m[k]] - E[m[reps]]) <= energy_tol
            if fit.any():
                rep[m[k]] = m[reps[int(np.argmax(fit))]]
            else:
                reps.append(k)
                rep[m[k]] = m[k]
        n_unique.append(len(reps))
    return rep, np.asarray(n_unique, np.int64)


def top_sites(energy, flags, group, k, rep=None):
    """(top [G,k] in the caller's indexing, top_energy [G,k])."""
    E = np.asarray(energy, np.float64)
    ok = _valid(energy, flags, len(E))
    if rep is not None:
        ok &= np.asarray(rep) == np.arange(len(E))
    _, members = regroup_numpy(group)
    top = np.full((len(members), k), -1, np.int64)
    top_e = np.full((len(members), k), np.inf)
    for g, m in enumerate(members):
        cand = sorted((E[i], pos, i) for pos, i in enumerate(m) if ok[i])[:k]
        for c, (e, _, i) in enumerate(cand):
            top[g, c], top_e[g, c] = i, e
    return top, top_e


def assert_margins(matrices, seam, group, tol, energy=None, energy_tol=None):
    """The conditions under which exact equality is asked: stated in float64, before anything is compared."""
    assert seam >= SEAM_MARGIN, f"a compared fractional component lies {seam:.2e} from the 0.5 seam"
    _, members = regroup_numpy(group)
    for D, m in zip(matrices, members):
        off = D[~np.eye(len(m), dtype=bool)]
        off = off[np.isfinite(off)]
        if off.size:
            gap = float(np.abs(off - tol).min())
            assert gap >= TOL_MARGIN, f"a pair distance lies {gap:.2e} A from tol"
        if energy is not None and energy_tol is not None and len(m) > 1:
            E = np.asarray(energy, np.float64)[m]
            E = E[~np.isnan(E)]
            diff = np.abs(E[:, None] - E[None, :])[~np.eye(len(E), dtype=bool)]
            if diff.size:
                gap = float(np.abs(diff - energy_tol).min())
                assert gap >= ENERGY_MARGIN, f"an energy difference lies {gap:.2e} from energy_tol"


# --------------------------------------------------------------------------------------------------------- the generators
ORTHO = np.array([[9.0, 0.0, 0.0], [0.0, 10.0, 0.0], [0.0, 0.0, 20.0]])
SKEWED = np.array([[9.0, 0.8, 0.6], [2.5, 8.5, 0.7], [1.2, 1.6, 18.0]])          # no zero entry: fully skewed
WIDE = np.array([[24.0, 0.0, 0.0], [3.0, 25.0, 0.0], [0.0, 0.0, 30.0]])


def _site(frac_slab, frac_ads, Z_slab, Z_ads, cell, group):
    frac = np.concatenate([frac_slab, frac_ads]) if len(frac_ads) else frac_slab
    tags = np.concatenate([np.arange(len(frac_slab)) % 2, np.full(len(frac_ads), 2)]).astype(np.int64)
    return {"pos": (frac @ cell).astype(np.float32), "tags": tags, "Z": np.concatenate([Z_slab, Z_ads]).astype(np.int64),
            "cell": cell.astype(np.float32), "group": group}


def duplicate(site, rng, tol=TOL, wrap=False, flip=False):
    """A copy of ``site`` rigidly shifted by at most 0.4 tol.  ``wrap``: every atom is then brought back into the cell, so
    an atom the shift pushed through a cell face sits a lattice vector away from its original.  ``flip``: the two
    adsorbate atoms trade places (a homonuclear adsorbate placed upside down)."""
    u = rng.normal(size=3)
    shift = u / np.linalg.norm(u) * rng.uniform(0.2, 0.4) * tol
    pos = site["pos"].astype(np.float64) + shift
    if wrap:
        cell = site["cell"].astype(np.float64)
        pos = (pos @ np.linalg.inv(cell) % 1.0) @ cell
    if flip:
        a = np.nonzero(site["tags"] == 2)[0]
        assert len(a) == 2 and site["Z"][a[0]] == site["Z"][a[1]]
        pos[a] = pos[a[::-1]]
    return dict(site, pos=pos.astype(np.float32))


def _family(rng, n_base, n_slab, Z_ads, cell, group, spread=0.06, centres=None):
    """``n_base`` distinct sites of one slab: the same slab atoms (some of them within 0.4 tol of a cell face), the same
    adsorbate shape, centres at least 0.035 apart in fractional coordinates inside [0.15, 0.45]^2 - so that every compared
    fractional component stays below 0.3 + 2 x spread < 0.5."""
    frac_slab = np.column_stack([rng.uniform(0, 1, n_slab), rng.uniform(0, 1, n_slab), rng.uniform(0.1, 0.3, n_slab)])
    frac_slab[0, 0], frac_slab[1 % n_slab, 1] = 5e-4, 1.0 - 5e-4       # a shift of 0.01 A and more carries these through a face
    Z_slab = rng.choice([29, 46, 78], n_slab)
    shape = np.column_stack([rng.uniform(-spread, spread, (len(Z_ads), 2)), rng.uniform(0.0, 0.05, len(Z_ads))])
    if centres is None:
        centres = []
        while len(centres) < n_base:
            c = rng.uniform(0.15, 0.45, 2)
            if all(np.abs(c - o).max() >= 0.035 for o in centres):
                centres.append(c)
    return [_site(frac_slab, shape + np.array([c[0], c[1], 0.4]), Z_slab, np.asarray(Z_ads, np.int64), cell, group)
            for c in centres]


@functools.lru_cache(maxsize=None)
def main_case():
    """The distance tests' batch: groups of 1, 2, 3 and 65 sites, adsorbates of 0, 1, 2 (homonuclear, one flipped), 5 and 70
    atoms, slabs of 8 to 40 atoms, a fully skewed cell, duplicates wrapped through cell faces, one group whose members
    differ in atom count and in an element, ids interleaved in the caller's order.  Returns (sites, energy float32 [S])."""
    rng = np.random.default_rng(20241)
    sites = []
    sites += _family(rng, 1, 8, [8], ORTHO, 7)                                        # 1 site, 1-atom adsorbate
    a, = _family(rng, 1, 12, [7, 7], ORTHO, -3)                                       # 2 sites: N2 and N2 upside down
    a["pos"][-1] = a["pos"][-2] + np.float32([1.1, 0, 0])
    sites += [a, duplicate(a, rng, flip=True)]
    a, b = _family(rng, 2, 40, [6, 1, 1, 8, 1], SKEWED, 12)                           # 3 sites, skewed, one wrapped duplicate
    sites += [a, b, duplicate(a, rng, wrap=True)]
    bases = _family(rng, 20, 9, [6, 8], ORTHO, 40)                                    # 65 sites: 20 distinct, 45 duplicates
    sites += bases + [duplicate(bases[int(rng.integers(20))], rng, wrap=bool(k % 2)) for k in range(45)]
    a, b = _family(rng, 2, 10, rng.choice([6, 1, 8], 70), WIDE, 41, spread=0.12,          # 70-atom adsorbate: more than a wave
                   centres=[np.array([0.2, 0.2]), np.array([0.3, 0.32])])
    sites += [a, duplicate(a, rng, wrap=True), b]
    a, = _family(rng, 1, 8, [], ORTHO, 5)                                             # no adsorbate
    sites += [a, duplicate(a, rng)]
    a, = _family(rng, 1, 10, [8], ORTHO, 100)                                         # members that cannot be compared
    longer = _site(a["pos"][:10].astype(np.float64) @ np.linalg.inv(ORTHO), np.array([[0.3, 0.3, 0.4], [0.35, 0.3, 0.4]]),
                   a["Z"][:10], np.array([8, 1]), ORTHO, 100)
    other = dict(a, Z=np.concatenate([a["Z"][:10], [16]]))
    sites += [a, duplicate(a, rng), longer, other]
    order = rng.permutation(len(sites))
    sites = [sites[i] for i in order]
    return sites, site_energies(sites, rng)


def site_energies(sites, rng, tol=TOL):
    """Energies that follow the geometry: sites within tol of each other (float64 oracle) differ by less than 2e-3, a third of
    the duplicates are lifted by 0.05 (so that energy_tol = 0.01 splits their cluster), distinct sites differ by 0.3 and more."""
    matrices, _ = case_distances(sites)
    group = [s["group"] for s in sites]
    rep, _ = unique_sites(matrices, group, tol)
    E = np.zeros(len(sites))
    level = 0.0
    for s in range(len(sites)):
        if rep[s] == s:
            level += 0.3 + rng.uniform(0, 0.1)
            E[s] = level
    lifted = 0
    for s in range(len(sites)):
        if rep[s] != s:
            lifted += 1
            E[s] = E[rep[s]] + rng.uniform(2e-4, 1e-3) * rng.choice([-1, 1]) + (0.05 if lifted % 3 == 0 else 0.0)
    return (E - 4.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def large_case(n=1100, n_base=400):
    """One group of 1100 sites, a one-atom adsorbate on a two-atom slab: 400 distinct sites on a 20 x 20 grid (0.2 A and
    more apart) and 700 duplicates, shuffled.  Returns (sites, energy)."""
    rng = np.random.default_rng(7)
    grid = [np.array([0.05 + 0.02 * i, 0.05 + 0.02 * j]) for i in range(20) for j in range(20)][:n_base]
    bases = _family(rng, n_base, 2, [8], np.diag([10.0, 10.0, 20.0]), 3, centres=grid)
    sites = bases + [duplicate(bases[int(rng.integers(n_base))], rng, wrap=bool(k % 2)) for k in range(n - n_base)]
    sites = [sites[i] for i in rng.permutation(n)]
    return sites, site_energies(sites, rng)


def chain_case():
    """a ~ b ~ c with a and c apart: b = a + 0.7 tol, c = a + 1.4 tol along x.  In the order a, b, c the greedy rule gives two
    clusters ({a, b}, {c}); visited b first, one."""
    rng = np.random.default_rng(5)
    a, = _family(rng, 1, 8, [8], ORTHO, 0)
    step = np.float32([0.7 * TOL, 0, 0])
    return [a, dict(a, pos=a["pos"] + step), dict(a, pos=a["pos"] + 2 * step)]


def to_batch(sites, device="cpu"):
    """The case as a collated batch (``site_group`` included), in the caller's order."""
    data = [Data(pos=torch.from_numpy(s["pos"]).float().clone(), atomic_numbers=torch.from_numpy(s["Z"]).long(),
                 tags=torch.from_numpy(s["tags"]).long(), fixed=torch.zeros(len(s["Z"]), dtype=torch.long),
                 cell=torch.from_numpy(s["cell"]).float().reshape(1, 3, 3), sid=str(i)) for i, s in enumerate(sites)]
    b = Batch.from_data_list(data)
    b.site_group = torch.tensor([s["group"] for s in sites], dtype=torch.long)
    return b.to(device)


def groups_of(sites):
    return np.asarray([s["group"] for s in sites])
