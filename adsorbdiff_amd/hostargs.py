"""A batch as device arguments: the conversions every geometry stage (placement, surface_tags, slab_symmetry, site_select,
flag_anomaly) hands to its ``adf_*`` entry.  ``geometry`` is the whole unpacking; ``stream``, ``i32``, ``offsets``,
``pbc_rows`` and ``desc`` are its pieces, for the stages that reorder rows or build tables of their own.  The samplers,
``ml_relax`` and the trainers marshal through ``engine.PreparedBatch`` or handles of their own and do not come through
here."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import lib as _lib


def stream(dev) -> C.c_void_p:
    """The current HIP stream of ``dev`` as the ``void* stream`` argument."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def i32(t, dev) -> torch.Tensor:
    """Contiguous int32 on ``dev``; a float-typed table (atomic numbers read from a file) is truncated as ``.long()`` does."""
    return torch.as_tensor(t).to(dev).long().to(torch.int32).contiguous()


def offsets(counts: torch.Tensor) -> torch.Tensor:
    """int32 [n+1]: the exclusive prefix sum of ``counts`` [n], on its device."""
    off = torch.zeros(int(counts.numel()) + 1, dtype=torch.int32, device=counts.device)
    off[1:] = torch.cumsum(counts.long(), 0).to(torch.int32)
    return off


def pbc_rows(batch, B: int, dev) -> torch.Tensor:
    """int32 [B,3]: ``batch.pbc`` per system, all periodic without one (the project's default, engine.batch_pbc)."""
    pbc = getattr(batch, "pbc", None)
    if pbc is None:
        return torch.ones(B, 3, dtype=torch.int32, device=dev)
    pbc = torch.atleast_2d(torch.as_tensor(pbc)).to(dev)
    if pbc.shape[0] == 1 and B > 1:
        pbc = pbc.expand(B, 3)
    if tuple(pbc.shape) != (B, 3):
        raise ValueError(f"batch.pbc: [{B}, 3] expected, got {list(pbc.shape)}")
    return (pbc != 0).to(torch.int32).contiguous()


def desc(pos, cell, Z, atom_offset, B: int, N: int) -> _lib.BatchDesc:
    """The ``adf_batch`` of the entries that take one outside a sampler: no ``batch`` index, ``reps`` left at 0."""
    d = _lib.BatchDesc()
    d.num_systems, d.num_atoms = B, N
    d.pos, d.cell, d.atomic_numbers, d.batch = pos.data_ptr(), cell.data_ptr(), Z.data_ptr(), None
    d.atom_offset = atom_offset.data_ptr()
    return d


class Geometry(NamedTuple):
    """``geometry``: ``pos`` float32 [N,3], ``cell`` float32 [B,9] (rows = lattice vectors), ``natoms`` int64 [B] and
    ``atom_offset`` int32 [B+1], all contiguous on ``dev``; ``Z``, ``tags`` int32 [N] and ``pbc`` int32 [B,3] where asked for."""
    dev: torch.device
    pos: torch.Tensor
    cell: torch.Tensor
    natoms: torch.Tensor
    atom_offset: torch.Tensor
    B: int
    N: int
    Z: Optional[torch.Tensor] = None
    tags: Optional[torch.Tensor] = None
    pbc: Optional[torch.Tensor] = None


def geometry(batch, who: str, Z: bool = False, tags: bool = False, pbc: bool = False) -> Geometry:
    """Unpack ``batch`` for the entry point ``who``; refuses a batch that is not on a device, or that is empty."""
    if not batch.pos.is_cuda:
        raise RuntimeError(f"{who} runs on a ROCm device (the HIP path has no CPU fallback)")
    dev = batch.pos.device
    pos = batch.pos.detach().to(torch.float32).contiguous()
    natoms = batch.natoms.to(dev, torch.int64).reshape(-1)
    B, N = int(natoms.numel()), int(pos.shape[0])
    if B < 1:
        raise ValueError(f"{who}: an empty batch")
    cell = batch.cell.to(dev, torch.float32).reshape(B, 9).contiguous()
    return Geometry(dev, pos, cell, natoms, offsets(natoms), B, N,
                    i32(batch.atomic_numbers, dev) if Z else None, i32(batch.tags, dev) if tags else None,
                    pbc_rows(batch, B, dev) if pbc else None)
