"""Duplicate sites on the device (csrc/unique.hip): ``site_distances`` - the pairwise distance of the sites
of every slab; ``unique_sites`` - a deterministic greedy clustering on top of it; ``top_sites`` - the k valid (and, given
the clustering, distinct) sites of least energy per slab.  An extension: the reference has no counterpart; its
``scripts/run_vasp_dft/write_vasp_inputs_nsite.py`` takes the best N relaxed sites per slab on the host, where N copies of
one minimum are N sites.

The displacement of two positions follows the IS2RS metric (``scripts/eval.py:765-777``, ``min_diff``): fractional
coordinates in the first site's cell, ``% 1`` twice, minus 1 above 0.5.  In a strongly skewed cell that is the reference's
convention and not the shortest lattice image.  The contract is written out in include/adsorbdiff_hip.h.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import lib as _lib
from .flag_anomaly import regroup
from .hostargs import geometry, stream


def to_caller_order(index: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """Indices into the regrouped order -> indices into the caller's order; negative entries (none) are kept."""
    index = index.long()
    return torch.where(index >= 0, perm[index.clamp(min=0)], index)


def to_group_order(index: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """``index[s]`` (caller's order, pointing at the caller's order) -> the same array in the regrouped order, pointing at
    the regrouped order; negative entries are kept."""
    index = index.long()
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(perm.numel(), device=perm.device)
    moved = index[perm]
    return torch.where(moved >= 0, inverse[moved.clamp(min=0)], moved)


def _groups(batch, group, S: int, dev):
    if group is None:
        group = getattr(batch, "site_group", None)
        if group is None:
            raise ValueError("no group ids: pass group=, or a batch that carries site_group (place_adsorbates)")
    group = torch.as_tensor(group).reshape(-1)
    if int(group.numel()) != S:
        raise ValueError(f"{S} sites, {int(group.numel())} group ids")
    return group.to(dev)


class _Matrices:
    """The distance matrices of a batch in the regrouped order, with what the clustering needs next to them."""

    def __init__(self, batch, group, include_slab: bool, permutation_invariant: bool, symmetry=None):
        S = int(batch.natoms.shape[0])
        group = _groups(batch, group, S, batch.pos.device)
        g = geometry(batch, "site_distances", Z=True, tags=True)
        lib = _lib.load()
        dev, N, natoms = g.dev, g.N, g.natoms
        self.S, self.dev = S, dev
        self.perm, self.offsets, self.ids = regroup(group)
        self.G = int(self.ids.numel())
        start = g.atom_offset.long()[:-1]
        # the atoms in the regrouped order of their sites
        moved = natoms[self.perm]
        new_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        new_off[1:] = torch.cumsum(moved, 0)
        rows = torch.arange(N, device=dev) + torch.repeat_interleave(start[self.perm] - new_off[:-1], moved, output_size=N)
        p, tags, Z = g.pos[rows].contiguous(), g.tags[rows].contiguous(), g.Z[rows].contiguous()
        cell = g.cell[self.perm].contiguous()
        self.counts = (self.offsets[1:] - self.offsets[:-1]).long()
        self.pair_offset = torch.zeros(self.G + 1, dtype=torch.int64, device=dev)
        self.pair_offset[1:] = torch.cumsum(self.counts * self.counts, 0)
        self.sizes = self.counts.tolist()                       # the one read-back: the output's size
        self.total = sum(n * n for n in self.sizes)
        self.dist = torch.empty(self.total, dtype=torch.float32, device=dev)
        atom_offset = new_off.to(torch.int32)
        self.best_op = None
        if symmetry is not None:
            # slab b of the symmetry is group id b: the operations of the groups present, group by group (the ids come to
            # the host for it: a second small read-back)
            op_off, rot, trans, sperm, perm_off, K, P = symmetry.for_groups(self.ids.tolist())
            self.best_op = torch.empty(self.total, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.adf_site_pair_distances_sym(p.data_ptr(), cell.data_ptr(), tags.data_ptr(), Z.data_ptr(),
                                                           atom_offset.data_ptr(), self.offsets.data_ptr(),
                                                           self.pair_offset.data_ptr(), N, S, self.G, self.total,
                                                           int(bool(include_slab)), int(bool(permutation_invariant)),
                                                           op_off.data_ptr(), rot.data_ptr(), trans.data_ptr(),
                                                           sperm.data_ptr(), perm_off.data_ptr(), K, P,
                                                           self.dist.data_ptr(), self.best_op.data_ptr(), stream(dev)))
            return
        with torch.cuda.device(dev):
            _lib.check(lib.adf_site_pair_distances(p.data_ptr(), cell.data_ptr(), tags.data_ptr(), Z.data_ptr(),
                                                   atom_offset.data_ptr(), self.offsets.data_ptr(),
                                                   self.pair_offset.data_ptr(), N, S, self.G, self.total,
                                                   int(bool(include_slab)), int(bool(permutation_invariant)),
                                                   self.dist.data_ptr(), stream(dev)))

    def matrices(self, flat=None):
        flat = self.dist if flat is None else flat
        out, at = [], 0
        for n in self.sizes:
            out.append(flat[at:at + n * n].view(n, n))
            at += n * n
        return out


def site_distances(batch, group=None, include_slab: bool = True, permutation_invariant: bool = True, symmetry=None,
                   return_op: bool = False):
    """One [n,n] float32 matrix per distinct id of ``group`` (default ``batch.site_group``), ascending ids, rows and columns in
    the caller's order of the group's sites: ``d = max(d_ads, d_slab)``, symmetric, zero diagonal, ``+inf`` between sites that
    differ in atom count, tags or atomic numbers.  ``include_slab=False``: the adsorbate alone.  ``permutation_invariant``:
    the adsorbate through the symmetric per-element Hausdorff distance (a flipped N2 is the same site) instead of atom by
    atom.  ``symmetry`` (``slab_symmetry.find_symmetry``; its slab b is group id b): the least distance over the slab's
    operations applied to the earlier site of a pair; ``return_op``: also one [n,n] int32 matrix per group
    with the minimising operation's index within its slab, the direction always "earlier site onto later site"."""
    m = _Matrices(batch, group, include_slab, permutation_invariant, symmetry)
    if not return_op:
        return m.matrices()
    if m.best_op is None:
        raise ValueError("return_op needs symmetry=")
    return m.matrices(), m.matrices(m.best_op)


def unique_sites(batch, group=None, tol: float = 0.05, energy=None, energy_tol: Optional[float] = None, flags=None,
                 include_slab: bool = True, permutation_invariant: bool = True, symmetry=None, return_op: bool = False):
    """(rep [S] long, is_rep [S] bool, n_unique [G] long).  Per group the valid sites (no flag set, energy not NaN) are
    visited by (energy, the caller's order) - without ``energy`` in the caller's order - and each joins the first
    representative within ``tol`` of it (and within ``energy_tol`` in energy, when given), or becomes one.  ``rep[s]`` is the
    representative of site s in the caller's indexing, s itself for a representative, -1 for an invalid site.

    ``symmetry`` (``slab_symmetry.find_symmetry``; its slab b is group id b): the distance is the least over the slab's
    operations, so sites that are images of each other under a symmetry of their slab fall into one cluster.
    ``return_op`` (with ``symmetry``): also ``site_op`` [S] long - the operation of its slab under which site s was merged into
    ``rep[s]``, 0 for a representative or an invalid site - and ``site_op_inverse`` [S] bool: the operation takes the earlier
    site of a pair onto the later one, so it takes s onto its representative where s comes first (True) and the
    representative onto s otherwise."""
    S = int(batch.natoms.shape[0])
    if energy is not None and int(energy.numel()) != S:
        raise ValueError(f"{S} sites, {int(energy.numel())} energies")
    if flags is not None and tuple(flags.shape) != (S, 4):
        raise ValueError(f"flags has shape {tuple(flags.shape)}, expected ({S}, 4)")
    tol = float(tol)
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol = {tol}: must be finite and not negative")
    if return_op and symmetry is None:
        raise ValueError("return_op needs symmetry=")
    m = _Matrices(batch, group, include_slab, permutation_invariant, symmetry)
    lib, dev = _lib.load(), m.dev
    e = None if energy is None else energy.detach().reshape(-1).to(dev, torch.float32)[m.perm].contiguous()
    f = None if flags is None else flags.to(dev)[m.perm].to(torch.int32).contiguous()
    rep = torch.empty(S, dtype=torch.int32, device=dev)
    n_unique = torch.empty(m.G, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_unique_sites(m.dist.data_ptr(), m.offsets.data_ptr(), m.pair_offset.data_ptr(), S, m.G, m.total,
                                        None if e is None else e.data_ptr(), None if f is None else f.data_ptr(),
                                        C.c_float(tol), C.c_float(-1.0 if energy_tol is None else float(energy_tol)),
                                        rep.data_ptr(), n_unique.data_ptr(), stream(dev)))
    out = torch.empty(S, dtype=torch.long, device=dev)
    out[m.perm] = to_caller_order(rep, m.perm)
    if not return_op:
        return out, out == torch.arange(S, device=dev), n_unique.long()
    # in the regrouped order: site s of group g sits at row s - offsets[g] of the group's matrix, its representative likewise
    at = torch.arange(S, device=dev)
    g = torch.repeat_interleave(torch.arange(m.G, device=dev), m.counts, output_size=S)
    first, n = m.offsets.long()[g], m.counts[g]
    r = rep.long()
    merged = (r >= 0) & (r != at)
    cell_at = m.pair_offset[g] + (at - first) * n + (r.clamp(min=0) - first)
    op = torch.where(merged, m.best_op.long()[cell_at.clamp(0, max(m.total - 1, 0))], torch.zeros_like(at))
    site_op = torch.empty(S, dtype=torch.long, device=dev)
    site_op[m.perm] = op
    inverse = torch.empty(S, dtype=torch.bool, device=dev)
    inverse[m.perm] = merged & (at < r)
    return out, out == torch.arange(S, device=dev), n_unique.long(), site_op, inverse


def top_sites(energy: torch.Tensor, flags: Optional[torch.Tensor], group, k: int, rep=None):
    """(top [G,k] long, top_energy [G,k]) per distinct id of ``group`` (ascending): the k valid sites of least energy, ascending,
    ties to the site that comes first in the caller's order; with ``rep`` (``unique_sites``) only representatives.  ``top``
    indexes the caller's arrays; a group with fewer such sites has -1 and +inf in the remaining columns.  Column 0 without
    ``rep`` is ``best_sites``."""
    energy = energy.detach().reshape(-1)
    S = int(energy.numel())
    group = torch.as_tensor(group).reshape(-1)
    if int(group.numel()) != S:
        raise ValueError(f"{S} energies, {int(group.numel())} group ids")
    if flags is not None and tuple(flags.shape) != (S, 4):
        raise ValueError(f"flags has shape {tuple(flags.shape)}, expected ({S}, 4)")
    if rep is not None and int(torch.as_tensor(rep).numel()) != S:
        raise ValueError(f"{S} energies, {int(torch.as_tensor(rep).numel())} representatives")
    if int(k) < 1:
        raise ValueError(f"k = {k}: at least one site per group")
    if S == 0:
        raise ValueError("top_sites: no site")
    if not energy.is_cuda:
        raise RuntimeError("top_sites runs on a ROCm device (no CPU fallback)")
    lib = _lib.load()
    dev = energy.device
    perm, offsets, ids = regroup(group.to(dev))
    e = energy.to(torch.float32)[perm].contiguous()
    f = None if flags is None else flags.to(dev)[perm].to(torch.int32).contiguous()
    r = None if rep is None else to_group_order(torch.as_tensor(rep).to(dev).reshape(-1), perm).to(torch.int32).contiguous()
    G, k = int(ids.numel()), int(k)
    top = torch.empty(G, k, dtype=torch.int32, device=dev)
    top_e = torch.empty(G, k, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_select_top_sites(e.data_ptr(), None if f is None else f.data_ptr(),
                                            None if r is None else r.data_ptr(), offsets.data_ptr(), G, k, top.data_ptr(),
                                            top_e.data_ptr(), stream(dev)))
    return to_caller_order(top, perm), top_e
