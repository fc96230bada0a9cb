"""Relaxation anomalies and site ranking on the device.

``flag_anomalies`` evaluates the four first-frame / last-frame tests of the reference's ``DetectTrajAnomaly``
(adsorbdiff/placement/flag_anomaly.py:6-154) for a whole batch in one kernel call (``adf_flag_anomalies``);
``DetectTrajAnomaly`` is the reference's per-structure interface on top of it; ``best_sites`` takes, per system, the valid
site of least relaxed energy (scripts/eval.py:566-579, ``adf_select_best_sites``).

The connectivity rule is the contract written in include/adsorbdiff_hip.h: a reading of ASE's
``NeighborList(natural_cutoffs(atoms, mult), self_interaction=False, bothways=True)`` with its default ``skin=0.3``.  ASE is
not a dependency and was not run against it: parity with ASE is unpinned, ``skin`` and ``radii`` are parameters.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import lib as _lib
from .engine import batch_pbc, cell_repeats
from .hostargs import desc, geometry, stream

FLAG_NAMES = ("dissociated", "desorbed", "surface_changed", "intercalated")   # scripts/eval.py's order


def default_radii() -> np.ndarray:
    """``ase.data.covalent_radii`` (what ``natural_cutoffs`` reads).  No table is kept here: without ASE, pass one."""
    try:
        from ase.data import covalent_radii
    except ImportError as e:
        raise ImportError("flag_anomalies: radii=None loads ase.data.covalent_radii and the ase package is not installed; "
                          "pass a table of radii indexed by atomic number (radii=...)") from e
    return np.asarray(covalent_radii, dtype=np.float64)


def _radii_tensor(radii, device) -> torch.Tensor:
    t = torch.as_tensor(radii).to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if t.numel() == 0:
        raise ValueError("flag_anomalies: empty radius table")
    return t


def scatter_slab_positions(tags: torch.Tensor, init_pos: torch.Tensor, slab_pos: torch.Tensor) -> torch.Tensor:
    """[N_slab,3] over the tag != 2 atoms in batch order -> [N,3] aligned with the batch (adsorbate rows: initial)."""
    slab = tags != 2
    n_slab = int(slab.sum())
    if tuple(slab_pos.shape) != (n_slab, 3):
        raise ValueError(f"final_slab_pos has shape {tuple(slab_pos.shape)}, the batch has {n_slab} slab atoms")
    out = init_pos.clone()
    out[slab] = slab_pos.to(out.device, out.dtype)
    return out


def flag_anomalies(init_batch, final, final_slab_pos=None, radii=None, skin: float = 0.3,
                   surface_change_cutoff_multiplier: float = 1.5, desorption_cutoff_multiplier: float = 1.5) -> torch.Tensor:
    """[B,4] bool on the device: (dissociated, desorbed, surface_changed, intercalated) per system of ``init_batch``.
    ``final``: a batch, or an [N,3] tensor, aligned with ``init_batch``; ``final_slab_pos``: [N_slab,3] over the tag != 2
    atoms in batch order (the relaxed clean slab), default the initial positions."""
    table = default_radii() if radii is None else radii   # before the device check: a missing ase is reported first
    g = geometry(init_batch, "flag_anomalies", Z=True, tags=True)
    lib = _lib.load()
    dev, B, pos0, Z, tags = g.dev, g.B, g.pos, g.Z, g.tags
    pos_final = final if torch.is_tensor(final) else final.pos
    pos_final = pos_final.detach().to(dev, torch.float32).contiguous()
    if pos_final.shape != pos0.shape:
        raise ValueError(f"final positions {tuple(pos_final.shape)} are not aligned with the batch {tuple(pos0.shape)}")
    radii_t = _radii_tensor(table, dev)
    ref = None
    if final_slab_pos is not None:
        ref = scatter_slab_positions(tags, pos0, torch.as_tensor(final_slab_pos)).contiguous()
    # the largest threshold of the batch sizes the image loop (one read-back); 0.01 A covers the float32 rounding of the
    # nearest-image reduction
    r_max = float(radii_t[Z.long().clamp(0, radii_t.numel() - 1)].max())
    mult = max(1.0, float(surface_change_cutoff_multiplier), float(desorption_cutoff_multiplier))
    reach = mult * 2.0 * r_max + 2.0 * float(skin)
    reps = cell_repeats(g.cell, max(reach, 0.0) + 0.01, batch_pbc(init_batch))
    d = desc(pos0, g.cell, Z, g.atom_offset, B, g.N)
    d.reps[0], d.reps[1], d.reps[2] = reps
    flags = torch.empty(B, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_flag_anomalies(C.byref(d), pos_final.data_ptr(), None if ref is None else ref.data_ptr(),
                                          tags.data_ptr(), radii_t.data_ptr(), int(radii_t.numel()), C.c_float(skin),
                                          C.c_float(surface_change_cutoff_multiplier), C.c_float(desorption_cutoff_multiplier),
                                          flags.data_ptr(), stream(dev)))
    return flags != 0


def _positions(atoms) -> np.ndarray:
    p = atoms.get_positions() if hasattr(atoms, "get_positions") else atoms.positions
    return np.asarray(p, dtype=np.float64).reshape(-1, 3)


class DetectTrajAnomaly:
    """The reference's interface (placement/flag_anomaly.py:6-45) on the batched kernel: one call on first use, the four
    answers cached.  Atoms objects are duck-typed: ``positions`` / ``get_positions()``, ``cell``, ``numbers``, ``pbc``."""

    def __init__(self, init_atoms, final_atoms, atoms_tag, final_slab_atoms=None, surface_change_cutoff_multiplier=1.5,
                 desorption_cutoff_multiplier=1.5, radii=None, skin=0.3, device="cuda:0"):
        self.init_atoms = init_atoms
        self.final_atoms = final_atoms
        self.final_slab_atoms = final_slab_atoms
        self.atoms_tag = atoms_tag
        self.surface_change_cutoff_multiplier = surface_change_cutoff_multiplier
        self.desorption_cutoff_multiplier = desorption_cutoff_multiplier
        self.radii, self.skin, self.device = radii, skin, device
        self._flags = None

    def _evaluate(self):
        if self._flags is None:
            from .data import Batch

            dev = torch.device(self.device)
            a = self.init_atoms
            b = Batch()
            b.pos = torch.as_tensor(_positions(a), dtype=torch.float32, device=dev)
            b.cell = torch.as_tensor(np.asarray(a.cell, dtype=np.float64).reshape(1, 3, 3), dtype=torch.float32, device=dev)
            b.atomic_numbers = torch.as_tensor(np.asarray(a.numbers), dtype=torch.long, device=dev)
            b.tags = torch.as_tensor(np.asarray(self.atoms_tag), dtype=torch.long, device=dev)
            b.natoms = torch.tensor([b.pos.shape[0]], dtype=torch.long, device=dev)
            pbc = getattr(a, "pbc", None)
            if pbc is not None:
                b.pbc = torch.as_tensor(np.broadcast_to(np.asarray(pbc, dtype=bool), (3,)).copy()).reshape(1, 3)
            final = torch.as_tensor(_positions(self.final_atoms), dtype=torch.float32, device=dev)
            slab = None if self.final_slab_atoms is None else torch.as_tensor(_positions(self.final_slab_atoms),
                                                                             dtype=torch.float32, device=dev)
            f = flag_anomalies(b, final, slab, radii=self.radii, skin=self.skin,
                               surface_change_cutoff_multiplier=self.surface_change_cutoff_multiplier,
                               desorption_cutoff_multiplier=self.desorption_cutoff_multiplier)
            self._flags = tuple(bool(v) for v in f[0].tolist())
        return self._flags

    def is_adsorbate_dissociated(self) -> bool:
        return self._evaluate()[0]

    def is_adsorbate_desorbed(self) -> bool:
        return self._evaluate()[1]

    def has_surface_changed(self) -> bool:
        return self._evaluate()[2]

    def is_adsorbate_intercalated(self) -> bool:
        return self._evaluate()[3]


def regroup(group: torch.Tensor):
    """Sites with any integer ids -> (perm, offsets, ids): ``perm`` brings the sites into contiguous groups (a stable sort:
    the caller's order is kept inside a group), ``offsets`` [G+1] bounds them, ``ids`` [G] ascending distinct ids."""
    group = torch.as_tensor(group).reshape(-1).long()
    perm = torch.sort(group, stable=True).indices
    ids, counts = torch.unique_consecutive(group[perm], return_counts=True)
    offsets = torch.zeros(ids.numel() + 1, dtype=torch.int32, device=group.device)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return perm, offsets, ids


def best_sites(energy: torch.Tensor, flags: Optional[torch.Tensor], group):
    """Per distinct id of ``group`` (ascending): (best, best_energy, n_valid).  ``best`` indexes the caller's arrays (-1:
    no valid site, then ``best_energy`` is +inf).  A site is valid when none of its four flags is set (``flags`` None: no
    filter) and its energy is not NaN; ties go to the site that comes first in the caller's order."""
    if not energy.is_cuda:
        raise RuntimeError("best_sites runs on a ROCm device (no CPU fallback)")
    lib = _lib.load()
    dev = energy.device
    energy = energy.detach().reshape(-1)
    S = int(energy.numel())
    group = torch.as_tensor(group).to(dev).reshape(-1)
    if int(group.numel()) != S:
        raise ValueError(f"{S} energies, {int(group.numel())} group ids")
    if flags is not None and tuple(flags.shape) != (S, 4):
        raise ValueError(f"flags has shape {tuple(flags.shape)}, expected ({S}, 4)")
    if S == 0:
        raise ValueError("best_sites: no site")
    perm, offsets, ids = regroup(group)
    e = energy.to(torch.float32)[perm].contiguous()
    f = None if flags is None else flags.to(dev)[perm].to(torch.int32).contiguous()
    G = int(ids.numel())
    best = torch.empty(G, dtype=torch.int32, device=dev)
    best_e = torch.empty(G, dtype=torch.float32, device=dev)
    n_valid = torch.empty(G, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_select_best_sites(e.data_ptr(), None if f is None else f.data_ptr(), offsets.data_ptr(), G,
                                             best.data_ptr(), best_e.data_ptr(), n_valid.data_ptr(), stream(dev)))
    best = best.long()
    best = torch.where(best >= 0, perm[best.clamp(min=0)], best)   # sorted order -> the caller's order
    return best, best_e, n_valid.long()
