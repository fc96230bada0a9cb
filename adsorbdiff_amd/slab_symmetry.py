"""Slab symmetry on the device (csrc/symmetry.hip): ``find_symmetry`` - the operations ``x -> R x + tau`` of
every bare slab of a batch that keep the surface normal (rotations about it, mirrors containing it, supercell translations),
each with the permutation it induces on the slab's atoms; ``carry`` - sites carried through such operations.  With a
``SlabSymmetry``, ``site_select.site_distances`` / ``unique_sites`` and ``ml_relaxation.ml_relax_unique`` treat sites that
are images of each other under an operation of their slab as one site.  An extension: the reference has no counterpart (it
leaves symmetry reduction to pymatgen's site finder, ``placement/adsorbate_slab_config.py:113-116``); the contract, written
out in include/adsorbdiff_hip.h, stands alone - neither pymatgen nor spglib was run against it.

The search is for pristine slabs: a relaxed, distorted slab has the identity alone.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List

import torch

from . import lib as _lib
from .hostargs import geometry, stream


@dataclass
class SlabSymmetry:
    """The operations of B slabs, K in all.  Slab b owns operations ``op_offset[b] .. op_offset[b+1]``; operation 0 of a
    slab is the identity (``R = I``, ``tau = 0``, ``perm = iota`` exactly), the others follow in ascending
    ``(W00, W01, W10, W11, j)``.  ``perm`` is flat: operation k of slab b (k counted within the slab) owns the ``natoms[b]``
    entries from ``perm_offset[b] + k natoms[b]``; entry i is the slab atom that atom i is taken onto."""
    n_ops: torch.Tensor          # [B] long
    op_offset: torch.Tensor      # [B+1] int32
    rot: torch.Tensor            # [K,3,3] float64
    trans: torch.Tensor          # [K,3] float64
    W: torch.Tensor              # [K,4] int32: the point operation in the basis (cell[0], cell[1]), row-major
    perm: torch.Tensor           # [sum n_ops[b] natoms[b]] int32
    perm_offset: torch.Tensor    # [B+1] int64
    natoms: torch.Tensor         # [B] long
    counts: List[int]            # n_ops on the host
    sizes: List[int]             # natoms on the host

    @property
    def num_slabs(self) -> int:
        return len(self.counts)

    def ops(self, b: int):
        """(rot [k,3,3], trans [k,3], W [k,4], perm [k,n]) of slab b."""
        o = sum(self.counts[:b])
        p = sum(c * n for c, n in zip(self.counts[:b], self.sizes[:b]))
        k, n = self.counts[b], self.sizes[b]
        return self.rot[o:o + k], self.trans[o:o + k], self.W[o:o + k], self.perm[p:p + k * n].view(k, n)

    @staticmethod
    def identity(natoms, device) -> "SlabSymmetry":
        """The identity alone for slabs of ``natoms`` atoms: with it every symmetry-aware call computes what the plain one does."""
        sizes = [int(n) for n in torch.as_tensor(natoms).reshape(-1).tolist()]
        B = len(sizes)
        nat = torch.tensor(sizes, dtype=torch.long, device=device)
        off = torch.zeros(B + 1, dtype=torch.int64, device=device)
        off[1:] = torch.cumsum(nat, 0)
        local = torch.arange(sum(sizes), device=device) - torch.repeat_interleave(off[:-1], nat, output_size=sum(sizes))
        W = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=device).repeat(B, 1)
        return SlabSymmetry(n_ops=torch.ones(B, dtype=torch.long, device=device),
                            op_offset=torch.arange(B + 1, dtype=torch.int32, device=device),
                            rot=torch.eye(3, dtype=torch.float64, device=device).repeat(B, 1, 1),
                            trans=torch.zeros(B, 3, dtype=torch.float64, device=device), W=W,
                            perm=local.to(torch.int32), perm_offset=off, natoms=nat, counts=[1] * B, sizes=sizes)

    def for_groups(self, ids: List[int]):
        """The operations of the slabs ``ids`` (ascending group ids), laid out group by group as adf_site_pair_distances_sym
        reads them: (op_offset [G+1] int32, rot, trans, perm, perm_offset [G+1] int64, operations, permutation entries)."""
        B = self.num_slabs
        if any(i < 0 or i >= B for i in ids):
            raise ValueError(f"symmetry of {B} slabs, group ids {min(ids)} .. {max(ids)}: a site's group id is its slab's index")
        if ids == list(range(B)):
            return self.op_offset, self.rot, self.trans, self.perm, self.perm_offset, sum(self.counts), int(self.perm.numel())
        dev = self.rot.device
        idx = torch.tensor(ids, dtype=torch.long, device=dev)
        k = [self.counts[i] for i in ids]
        e = [self.counts[i] * self.sizes[i] for i in ids]
        K, P = sum(k), sum(e)
        kt, et = torch.tensor(k, dtype=torch.long, device=dev), torch.tensor(e, dtype=torch.long, device=dev)
        op_off = torch.zeros(len(ids) + 1, dtype=torch.int64, device=dev)
        op_off[1:] = torch.cumsum(kt, 0)
        perm_off = torch.zeros(len(ids) + 1, dtype=torch.int64, device=dev)
        perm_off[1:] = torch.cumsum(et, 0)
        rows = torch.arange(K, device=dev) + torch.repeat_interleave(self.op_offset.long()[idx] - op_off[:-1], kt, output_size=K)
        cols = torch.arange(P, device=dev) + torch.repeat_interleave(self.perm_offset[idx] - perm_off[:-1], et, output_size=P)
        return (op_off.to(torch.int32), self.rot[rows].contiguous(), self.trans[rows].contiguous(), self.perm[cols].contiguous(),
                perm_off, K, P)


def find_symmetry(slab_batch, symprec: float = 0.01, proper_only: bool = False) -> SlabSymmetry:
    """The symmetry operations of every slab of ``slab_batch`` - the batch of bare slabs ``place_adsorbates`` takes: slab b is
    group b of ``site_group`` and its atom k the k-th ``tags != 2`` atom of every site placed on it.  ``symprec`` (A): how
    far a lattice vector's length and an atom's image may be off; it must stay below half the shortest in-plane lattice
    height (``ValueError`` otherwise).  ``proper_only``: rotations only, no mirrors.  Two launches and one read-back (the
    counts, which size the outputs) between them; no loop over slabs."""
    g = geometry(slab_batch, "find_symmetry", Z=True)
    dev, B, N, atom_offset = g.dev, g.B, g.N, g.atom_offset
    if N == 0:
        raise ValueError("find_symmetry: no slab")
    symprec = float(symprec)
    lib = _lib.load()
    scratch = torch.empty(int(lib.adf_slab_symmetry_scratch(N, B)), dtype=torch.uint8, device=dev)
    found = torch.empty(2 * B, dtype=torch.int32, device=dev)          # counts, then atom counts
    host = torch.empty(2 * B, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_slab_symmetry_search(g.pos.data_ptr(), g.cell.data_ptr(), g.Z.data_ptr(), atom_offset.data_ptr(), N, B,
                                                C.c_double(symprec), int(bool(proper_only)), scratch.data_ptr(),
                                                found.data_ptr(), host.data_ptr(), stream(dev)))
    counts, sizes = host[:B].tolist(), host[B:].tolist()
    K, P = sum(counts), sum(c * n for c, n in zip(counts, sizes))
    n_ops, nat = found[:B].long(), found[B:].long()
    op_offset = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    op_offset[1:] = torch.cumsum(n_ops, 0)
    perm_offset = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    perm_offset[1:] = torch.cumsum(n_ops * nat, 0)
    rot = torch.empty(K, 3, 3, dtype=torch.float64, device=dev)
    trans = torch.empty(K, 3, dtype=torch.float64, device=dev)
    W = torch.empty(K, 4, dtype=torch.int32, device=dev)
    perm = torch.empty(P, dtype=torch.int32, device=dev)
    if K > 0 and P > 0:
        with torch.cuda.device(dev):
            _lib.check(lib.adf_slab_symmetry_emit(atom_offset.data_ptr(), N, B, C.c_double(symprec), scratch.data_ptr(),
                                                  op_offset.data_ptr(), perm_offset.data_ptr(), K, P, rot.data_ptr(),
                                                  trans.data_ptr(), W.data_ptr(), perm.data_ptr(), stream(dev)))
    return SlabSymmetry(n_ops=n_ops, op_offset=op_offset, rot=rot, trans=trans, W=W, perm=perm, perm_offset=perm_offset,
                        natoms=nat, counts=counts, sizes=sizes)


def carry(symmetry: SlabSymmetry, slab, op, inverse, tags, natoms, pos, force=None):
    """Sites carried through operations of their slabs, on the device, without a read-back.  Site s (``natoms[s]`` atoms of
    ``pos`` / ``force`` / ``tags``) lies on slab ``slab[s]`` and goes through its operation ``op[s]`` = (R, tau, perm):

    * ``inverse[s]`` False: the slab atom of rank ``perm[i]`` (rank: position among the ``tags != 2`` atoms) of the result
      is ``R x_i + tau``, an adsorbate atom m becomes ``R x_m + tau`` in place;
    * ``inverse[s]`` True: the slab atom of rank i is ``R^-1 (x_perm[i] - tau)``, an adsorbate atom ``R^-1 (x_m - tau)``.

    Forces go through ``R`` / ``R^-1`` alone.  The arithmetic is float64, rounded to the input's dtype once; positions are not
    wrapped back into the cell.  Sites with ``op[s] == 0`` are returned as they are, bit for bit.  Returns ``pos`` (and
    ``force`` when given)."""
    dev = pos.device
    natoms = natoms.to(dev).long().reshape(-1)
    S, N = int(natoms.shape[0]), int(pos.shape[0])
    slab, op = slab.to(dev).long().reshape(-1), op.to(dev).long().reshape(-1)
    inverse = inverse.to(dev).bool().reshape(-1)
    start = torch.cumsum(natoms, 0) - natoms
    site = torch.repeat_interleave(torch.arange(S, device=dev), natoms, output_size=N)
    is_slab = tags.to(dev).reshape(-1) != 2
    before = torch.cumsum(is_slab.long(), 0) - is_slab.long()            # slab atoms before this one in the batch
    rank = before - before[start.clamp(max=max(N - 1, 0))][site]       # ... in its site
    atoms = torch.arange(N, device=dev)
    # atom_of[start + q]: the site's slab atom of rank q
    atom_of = torch.zeros(N + 1, dtype=torch.long, device=dev)
    atom_of[torch.where(is_slab, start[site] + rank, torch.full_like(rank, N))] = atoms
    nb = symmetry.natoms.to(dev)[slab]
    row = symmetry.perm_offset.to(dev)[slab] + op * nb                  # the operation's permutation
    P = int(symmetry.perm.numel())
    at = (row[site] + torch.minimum(rank, (nb[site] - 1).clamp(min=0))).clamp(0, max(P - 1, 0))
    partner = symmetry.perm.to(dev).long()[at].clamp(0, None)
    partner_atom = atom_of[(start[site] + torch.minimum(partner, (natoms[site] - 1).clamp(min=0))).clamp(0, N)]
    moved = (op != 0)[site]
    inv_atom = inverse[site]
    source = atoms.clone()
    take = moved & is_slab
    source = torch.where(take & inv_atom, partner_atom, source)
    fwd = take & ~inv_atom
    scatter = torch.zeros(N + 1, dtype=torch.long, device=dev)
    scatter[torch.where(fwd, partner_atom, torch.full_like(partner_atom, N))] = atoms
    # (every slab atom of a forward site is some atom's partner: perm is a permutation)
    source = torch.where(fwd, scatter[:N], source)
    k = (symmetry.op_offset.to(dev).long()[slab] + op).clamp(0, max(int(symmetry.rot.shape[0]) - 1, 0))
    R = symmetry.rot.to(dev)[k]
    Ri = torch.linalg.inv(R)
    tau = symmetry.trans.to(dev)[k]
    R, Ri, tau = R[site], Ri[site], tau[site]

    def through(v, shift):
        x = v[source].double()
        f = torch.einsum("nij,nj->ni", R, x) + (tau if shift else 0.0)
        b = torch.einsum("nij,nj->ni", Ri, x - tau if shift else x)
        return torch.where(moved[:, None], torch.where(inv_atom[:, None], b, f).to(v.dtype), v)

    out = through(pos, True)
    return out if force is None else (out, through(force, False))
