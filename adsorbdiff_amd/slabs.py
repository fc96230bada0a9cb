"""Slabs from bulk crystals on the device (csrc/slabcut.hip): the reference's ``compute_slabs``, ``Slab`` and
``Bulk`` (adsorbdiff/placement/slab.py:44-223, 485-616) for a whole batch of bulks - oriented cell, thickness, terminations,
primitive in-plane cell, duplicate terminations, top and bottom - and ``distinct_millers``, pymatgen's
``get_symmetrically_distinct_miller_indices``.  With ``cut_and_tag`` (the reference's ``tile_and_tag_atoms`` over
``compute_slabs``) ``bulk -> slabs -> tags -> sites -> placement -> sampling -> relaxation -> ranked sites`` needs nothing
outside this package.

The rule is the contract written in include/adsorbdiff_hip.h, section "Slab cutting".  Neither pymatgen nor spglib is a
dependency and neither was run against it: parity with pymatgen unpinned; the contract is pinned to an independent float64 statement
(tests/helpers_slabs.py), to crystallographic facts and to the invariants of a correct slab.  The bulk's cell is taken as
given: ``standardize_bulk`` (spglib's conventional cell) stays out, and so do ``lll_reduce``, ``max_normal_search``,
bond-aware cuts, ``symmetrize=True``, pickles (``from_precomputed_slabs_pkl``, ``save_path``) and ASE / pymatgen objects.
Stated deviations: the third cell vector is perpendicular to the surface (pymatgen keeps the oblique one), and
``is_structure_invertible`` is read as "any operation with zz = -1".  The point-group search of ``distinct_millers`` is
complete for conventional and reduced cells; for other cells it can only miss operations, which yields duplicate slabs,
never a wrong one.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import lib as _lib
from . import surface_tags
from .data import Batch
from .hostargs import i32, offsets, stream


class BulkArgs(NamedTuple):
    dev: torch.device
    pos: torch.Tensor            # float64 [N,3]
    cell: torch.Tensor           # float64 [B,9]
    Z: torch.Tensor              # int32 [N]
    natoms: torch.Tensor         # int64 [B]
    atom_offset: torch.Tensor    # int32 [B+1]
    B: int
    N: int


def _positive(name: str, v) -> float:
    v = float(v)
    if not (0.0 < v < math.inf):
        raise ValueError(f"{name} = {v}: finite and positive expected")
    return v


def _max_miller(v) -> int:
    if int(v) != v or not 1 <= int(v) <= 4:
        raise ValueError(f"max_miller = {v}: an integer 1 .. 4 expected")
    return int(v)


def _bulks(bulk_batch, who: str) -> BulkArgs:
    """A batch of bulks as device arguments: positions and cells widened to float64 (exact for float32 input)."""
    if not bulk_batch.pos.is_cuda:
        raise RuntimeError(f"{who} runs on a ROCm device (the HIP path has no CPU fallback)")
    dev = bulk_batch.pos.device
    natoms = bulk_batch.natoms.to(dev, torch.int64).reshape(-1)
    B, N = int(natoms.numel()), int(bulk_batch.pos.shape[0])
    if B < 1 or N < 1:
        raise ValueError(f"{who}: an empty batch")
    pbc = getattr(bulk_batch, "pbc", None)
    if pbc is not None and not bool((torch.as_tensor(pbc) != 0).all()):
        raise ValueError(f"{who}: a bulk is periodic in all three directions")
    return BulkArgs(dev, bulk_batch.pos.detach().to(torch.float64).contiguous(),
                    bulk_batch.cell.to(dev, torch.float64).reshape(B, 9).contiguous(), i32(bulk_batch.atomic_numbers, dev),
                    natoms, offsets(natoms), B, N)


@torch.no_grad()
def distinct_millers(bulk_batch, max_miller: int = 2, symprec: float = 1e-3):
    """The symmetrically distinct Miller indices of every bulk: ``(millers int32 [K,3], offsets int32 [B+1], n_ops int64 [B])``
    on the device - bulk b owns rows ``offsets[b] .. offsets[b+1]``, in descending lexicographic order; ``n_ops`` is the order
    of the point group found.  Two launches and one read-back (the counts) between them."""
    max_miller, symprec = _max_miller(max_miller), _positive("symprec", symprec)
    g = _bulks(bulk_batch, "distinct_millers")
    return _distinct_millers(g, max_miller, symprec)


def _distinct_millers(g: BulkArgs, max_miller: int, symprec: float):
    lib = _lib.load()
    scratch = torch.empty(int(lib.adf_distinct_millers_scratch(g.N, g.B)), dtype=torch.uint8, device=g.dev)
    found = torch.empty(3 * g.B, dtype=torch.int32, device=g.dev)
    host = torch.empty(3 * g.B, dtype=torch.int32)
    with torch.cuda.device(g.dev):
        _lib.check(lib.adf_distinct_millers_count(g.pos.data_ptr(), g.cell.data_ptr(), g.Z.data_ptr(), g.atom_offset.data_ptr(),
                                                  g.N, g.B, max_miller, C.c_double(symprec), scratch.data_ptr(), found.data_ptr(),
                                                  host.data_ptr(), stream(g.dev)))
    counts = found.view(g.B, 3)[:, 0]
    K = int(host.view(g.B, 3)[:, 0].sum())
    off = offsets(counts)
    millers = torch.empty(K, 3, dtype=torch.int32, device=g.dev)
    with torch.cuda.device(g.dev):
        _lib.check(lib.adf_distinct_millers_fill(scratch.data_ptr(), found.data_ptr(), host.data_ptr(), off.data_ptr(), g.N, g.B,
                                                 max_miller, K, millers.data_ptr(), stream(g.dev)))
    return millers, off, found.view(g.B, 3)[:, 1].long()


class CutSlabs(NamedTuple):
    """``compute_slabs``: ``batch`` - the untiled slabs (``pos`` float32 [M,3], ``cell`` float32 [S,3,3], ``atomic_numbers``
    int64 [M], ``natoms`` int64 [S], ``pbc`` [S,3] = (1, 1, 0), and per slab ``millers`` int32 [S,3] (gcd-reduced), ``shift``
    float64 [S], ``top`` bool [S], ``bulk_index`` int64 [S]); ``pos64`` float64 [M,3] and ``cell64`` float64 [S,3,3]: what
    the float32 tensors were rounded from."""
    batch: Batch
    pos64: torch.Tensor
    cell64: torch.Tensor


def _pairs(specific_millers, B: int, dev):
    """(pair_bulk int32 [P], pair_miller int32 [P,3]) from one list of indices for all bulks, or one list per bulk."""
    rows = list(specific_millers)
    if len(rows) == 0:
        raise ValueError("specific_millers: empty")
    per_bulk = not (np.ndim(rows[0]) == 1 and len(rows[0]) == 3 and np.ndim(rows[0][0]) == 0)
    if per_bulk and len(rows) != B:
        raise ValueError(f"specific_millers: {len(rows)} lists for {B} bulks (one list for all, or one per bulk)")
    lists = rows if per_bulk else [rows] * B
    bulk, hkl = [], []
    for b, lst in enumerate(lists):
        arr = np.asarray(list(lst))
        if arr.ndim != 2 or arr.shape[1] != 3 or arr.shape[0] == 0 or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError(f"specific_millers: bulk {b}: a non-empty list of integer (h, k, l) expected")
        bulk += [b] * arr.shape[0]
        hkl.append(arr)
    return (torch.tensor(bulk, dtype=torch.int32, device=dev),
            torch.from_numpy(np.concatenate(hkl, 0).astype(np.int32)).to(dev).contiguous())


@torch.no_grad()
def compute_slabs(bulk_batch, max_miller: int = 2, specific_millers=None, min_slab_size: float = 7.0,
                  min_vacuum_size: float = 20.0, tol: float = 0.3, symprec: float = 1e-3) -> CutSlabs:
    """Every slab of every bulk of ``bulk_batch`` (``pos``, ``cell`` [B,3,3], ``atomic_numbers``, ``natoms``; periodic in all
    three directions) along its distinct Miller indices up to ``max_miller`` - or along ``specific_millers``, one list of
    ``(h, k, l)`` for all bulks or one list per bulk (``max_miller`` is then ignored, as in the reference).  Slabs of a bulk
    come Miller index by Miller index in the order asked for; within one, the ``top`` slabs by ascending ``shift``, then the
    flipped ones.  A count launch, one read-back that sizes the output, a fill launch; no loop over bulks."""
    min_slab_size, min_vacuum_size = _positive("min_slab_size", min_slab_size), _positive("min_vacuum_size", min_vacuum_size)
    tol, symprec = _positive("tol", tol), _positive("symprec", symprec)
    if specific_millers is None:
        max_miller = _max_miller(max_miller)
    g = _bulks(bulk_batch, "compute_slabs")
    dev = g.dev
    if specific_millers is None:
        millers, off, _ = _distinct_millers(g, max_miller, symprec)
        per_bulk = (off[1:] - off[:-1]).long()
        pair_miller = millers
        pair_bulk = torch.repeat_interleave(torch.arange(g.B, dtype=torch.int32, device=dev), per_bulk,
                                            output_size=int(millers.shape[0]))
    else:
        pair_bulk, pair_miller = _pairs(specific_millers, g.B, dev)
    P = int(pair_bulk.numel())
    seg = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(g.natoms[pair_bulk.long()], 0)
    A = int(seg[-1])                                                   # (a read-back of one word: it sizes the scratch)
    lib = _lib.load()
    scratch = torch.empty(int(lib.adf_slab_cut_scratch(A, P)), dtype=torch.uint8, device=dev)
    counts = torch.empty(3 * P, dtype=torch.int32, device=dev)
    host = torch.empty(3 * P, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_slab_cut_count(g.pos.data_ptr(), g.cell.data_ptr(), g.Z.data_ptr(), g.atom_offset.data_ptr(), g.N, g.B,
                                          pair_bulk.data_ptr(), pair_miller.data_ptr(), seg.data_ptr(), P, A,
                                          C.c_double(min_slab_size), C.c_double(min_vacuum_size), C.c_double(tol),
                                          C.c_double(symprec), scratch.data_ptr(), counts.data_ptr(), host.data_ptr(),
                                          stream(dev)))
    hv = host.view(P, 3).long()
    S, M = int(hv[:, 0].sum()), int((hv[:, 0] * hv[:, 1]).sum())
    cv = counts.view(P, 3)
    slab_off = offsets(cv[:, 0])
    out_off = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    out_off[1:] = torch.cumsum(cv[:, 0].long() * cv[:, 1].long(), 0)
    pos64 = torch.empty(M, 3, dtype=torch.float64, device=dev)
    pos32 = torch.empty(M, 3, dtype=torch.float32, device=dev)
    Z = torch.empty(M, dtype=torch.int32, device=dev)
    cell = torch.empty(S, 9, dtype=torch.float64, device=dev)
    millers = torch.empty(S, 3, dtype=torch.int32, device=dev)
    shift = torch.empty(S, dtype=torch.float64, device=dev)
    top = torch.empty(S, dtype=torch.int32, device=dev)
    bulk_index = torch.empty(S, dtype=torch.int32, device=dev)
    natoms = torch.empty(S, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_slab_cut_fill(scratch.data_ptr(), pair_bulk.data_ptr(), seg.data_ptr(), slab_off.data_ptr(),
                                         out_off.data_ptr(), P, A, C.c_double(symprec), S, M, pos64.data_ptr(), pos32.data_ptr(),
                                         Z.data_ptr(), cell.data_ptr(), millers.data_ptr(), shift.data_ptr(), top.data_ptr(),
                                         bulk_index.data_ptr(), natoms.data_ptr(), stream(dev)))
    out = Batch()
    out.pos = pos32
    out.cell = cell.view(S, 3, 3).to(torch.float32)
    out.atomic_numbers = Z.long()
    out.natoms = natoms.long()
    out.batch = torch.repeat_interleave(torch.arange(S, device=dev), out.natoms, output_size=M)
    out.pbc = torch.tensor([1, 1, 0], dtype=torch.long, device=dev).repeat(S, 1)
    out.millers = millers
    out.shift = shift
    out.top = top != 0
    out.bulk_index = bulk_index.long()
    return CutSlabs(out, pos64, cell.view(S, 3, 3))


@torch.no_grad()
def cut_and_tag(bulk_batch, max_miller: int = 2, specific_millers=None, min_slab_size: float = 7.0,
                min_vacuum_size: float = 20.0, tol: float = 0.3, symprec: float = 1e-3, min_ab: float = 8.0,
                height: float = 2.0, masses=None) -> Batch:
    """The reference's ``tile_and_tag_atoms`` over ``compute_slabs``: the unit slabs are tagged against their bulks' Voronoi
    coordination (``surface_tags.tag_surface_atoms(slabs, bulk=bulk_coordination(bulks)[bulk_index])``) and then tiled to at
    least ``min_ab`` (``surface_tags.tile_atoms``) - tag, then tile, the reference's order.  The result (``tags``, ``fixed``,
    and ``millers`` / ``shift`` / ``top`` / ``bulk_index`` per slab) is what ``heuristic_sites`` and ``place_adsorbates`` take
    as it is.  ``masses``: the table of ``tag_surface_atoms`` (None: ``placement.default_masses``, ASE's)."""
    slabs = compute_slabs(bulk_batch, max_miller, specific_millers, min_slab_size, min_vacuum_size, tol, symprec).batch
    table = surface_tags.bulk_coordination(bulk_batch)
    tagged = surface_tags.tag_surface_atoms(slabs, bulk=table[slabs.bulk_index], height=height, masses=masses)
    return surface_tags.tile_atoms(tagged, min_ab)


class Bulk:
    """One bulk crystal (the reference's ``Bulk``, without ASE or pickles): Cartesian ``pos`` [n,3], ``cell`` [3,3] (rows =
    lattice vectors, right-handed, taken as given), ``atomic_numbers`` [n]; ``src_id`` names it in a slab's metadata."""

    def __init__(self, pos, cell, atomic_numbers, src_id=None, device="cuda:0") -> None:
        self.pos = torch.as_tensor(np.asarray(pos), dtype=torch.float64).reshape(-1, 3)
        self.cell = torch.as_tensor(np.asarray(cell), dtype=torch.float64).reshape(3, 3)
        self.atomic_numbers = torch.as_tensor(np.asarray(atomic_numbers)).long().reshape(-1)
        if int(self.atomic_numbers.numel()) != int(self.pos.shape[0]) or int(self.pos.shape[0]) == 0:
            raise ValueError(f"Bulk: {int(self.pos.shape[0])} positions for {int(self.atomic_numbers.numel())} atomic numbers")
        self.src_id = src_id
        self.device = torch.device(device)

    def batch(self) -> Batch:
        """The bulk as a batch of one on its device."""
        b = Batch()
        b.pos = self.pos.to(self.device)
        b.cell = self.cell.reshape(1, 3, 3).to(self.device)
        b.atomic_numbers = self.atomic_numbers.to(self.device)
        b.natoms = torch.tensor([int(self.pos.shape[0])], dtype=torch.long, device=self.device)
        b.batch = torch.zeros(int(self.pos.shape[0]), dtype=torch.long, device=self.device)
        return b

    def __len__(self) -> int:
        return int(self.pos.shape[0])

    def __repr__(self) -> str:
        return f"Bulk: ({self.src_id}, {len(self)} atoms)"


class Slab:
    """One tiled, tagged slab of a bulk (the reference's ``Slab``): ``batch`` - a batch of one that ``heuristic_sites`` and
    ``place_adsorbates`` take -, ``millers`` (tuple), ``shift`` (float), ``top`` (bool)."""

    def __init__(self, bulk: Bulk, batch: Batch, millers, shift: float, top: bool, min_ab: float = 0.8) -> None:
        if bulk is None:
            raise ValueError("Slab: a bulk is required")
        self.bulk, self.batch = bulk, batch
        self.millers, self.shift, self.top = tuple(int(x) for x in millers), float(shift), bool(top)
        length = torch.linalg.norm(batch.cell.reshape(3, 3).double(), dim=1)
        if not (float(length[0]) >= min_ab and float(length[1]) >= min_ab):
            raise ValueError("Slab not tiled")
        if not bool((batch.tags == 1).any()):
            raise ValueError("Slab not tagged")
        if sorted(set(batch.atomic_numbers.tolist())) != sorted(set(bulk.atomic_numbers.tolist())):
            raise ValueError("Mismatched bulk and surface")

    @staticmethod
    def _all(bulk: Bulk, min_ab: float, **kw) -> List["Slab"]:
        tiled = cut_and_tag(bulk.batch(), min_ab=min_ab, **kw)
        millers, shift, top = tiled.millers.tolist(), tiled.shift.tolist(), tiled.top.tolist()
        out = []
        sizes = tiled.natoms.tolist()
        start = 0
        for s, n in enumerate(sizes):
            one = Batch()
            one.pos = tiled.pos[start:start + n]
            one.atomic_numbers = tiled.atomic_numbers[start:start + n]
            one.tags = tiled.tags[start:start + n]
            one.fixed = tiled.fixed[start:start + n]
            one.cell = tiled.cell[s:s + 1]
            one.pbc = tiled.pbc[s:s + 1]
            one.natoms = tiled.natoms[s:s + 1]
            one.batch = torch.zeros(n, dtype=torch.long, device=tiled.pos.device)
            out.append(Slab(bulk, one, millers[s], shift[s], top[s]))
            start += n
        return out

    @classmethod
    def from_bulk_get_all_slabs(cls, bulk: Bulk, max_miller: int = 2, min_ab: float = 8.0, masses=None) -> List["Slab"]:
        return cls._all(bulk, min_ab, max_miller=max_miller, masses=masses)

    @classmethod
    def from_bulk_get_specific_millers(cls, specific_millers, bulk: Bulk, min_ab: float = 8.0, masses=None) -> List["Slab"]:
        if not (isinstance(specific_millers, tuple) and len(specific_millers) == 3):
            raise ValueError("specific_millers: a tuple (h, k, l) expected")
        return cls._all(bulk, min_ab, specific_millers=[specific_millers], masses=masses)

    @classmethod
    def from_bulk_get_random_slab(cls, bulk: Bulk, max_miller: int = 2, min_ab: float = 8.0,
                                  generator: Optional[torch.Generator] = None, masses=None) -> "Slab":
        """One slab drawn uniformly from ``from_bulk_get_all_slabs``; ``generator``: a seeded (CPU) ``torch.Generator`` in the
        place of the reference's ``np.random``."""
        slabs = cls._all(bulk, min_ab, max_miller=max_miller, masses=masses)
        return slabs[int(torch.randint(len(slabs), (1,), generator=generator))]

    def has_surface_tagged(self) -> bool:
        return bool((self.batch.tags == 1).any())

    def get_metadata_dict(self) -> dict:
        return {"slab_batch": self.batch,
                "slab_metadata": {"bulk_id": self.bulk.src_id, "millers": self.millers, "shift": self.shift, "top": self.top}}

    def __len__(self) -> int:
        return int(self.batch.pos.shape[0])

    def __repr__(self) -> str:
        return f"Slab: ({len(self)} atoms, {self.millers}, {self.shift}, {self.top})"
