"""Surface tags on the device (csrc/voronoi.hip): the reference's ``tag_surface_atoms``, ``tile_atoms`` and
``set_fixed_atom_constraints`` (adsorbdiff/placement/slab.py:226-482) for a whole batch of slabs, so that a slab which
arrives without tags can enter ``surface_triangles_device``, ``heuristic_sites``, ``place_adsorbates``, ``flag_anomalies``
and ``ml_relax``, which all start from ``batch.tags`` (1: surface, 0: the rest, fixed).

``voronoi_coordination`` is pymatgen's ``VoronoiNN(tol).get_cn(use_weights=True)`` for every (selected) atom of a batch
(``adf_voronoi_coordination``), ``bulk_coordination`` the per-element minima of a batch of bulks
(``calculate_coordination_of_bulk_atoms``, reduced to what the comparison uses) and ``tag_surface_atoms`` the height rule
followed, with a bulk, by the coordination rule (``adf_tag_surface_atoms``).  ``tile_atoms`` is plain torch.

The rule is the contract written in include/adsorbdiff_hip.h.  Neither pymatgen nor ASE is a dependency and neither was run
against it: parity with pymatgen is unpinned; the geometry is pinned to qhull (``scipy.spatial.Voronoi`` on the same points,
tests/golden/voronoi_cn.npz).  Two deliberate deviations from the reference: one wrapped fractional height serves both the
height and the centre-of-mass test, and the coordination is compared as ``cn < bulk minimum - cn_tol`` instead of
``round(cn, 5) < bulk minimum`` (with float32 positions a fully coordinated fcc atom comes out at 11.999995).
Slab cutting from a Miller index (``Slab``, ``Bulk``, ``compute_slabs``) is adsorbdiff_amd/slabs.py.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import lib as _lib
from .data import _TENSOR_GRAPH_KEYS, Batch
from .hostargs import geometry, i32, offsets, stream
from .placement import default_masses

NUM_ELEMENTS = 119             # rows of the tables indexed by atomic number: 0 .. 118


class VoronoiCoordination(NamedTuple):
    """``voronoi_coordination``, per atom, on the device: ``cn`` float64 [N] (the sum of the weights above ``tol``),
    ``omega_max`` float64 [N] (the largest facet's solid angle, in sr), ``num_neighbors`` int32 [N] and ``open`` bool [N]
    (a cell its candidates do not close - pymatgen's RuntimeError -: ``cn`` and ``omega_max`` are NaN, ``num_neighbors`` 0).
    Rows of atoms outside ``select`` hold NaN, NaN, 0, False."""
    cn: torch.Tensor
    omega_max: torch.Tensor
    num_neighbors: torch.Tensor
    open: torch.Tensor


def _positive(name: str, v) -> float:
    v = float(v)
    if not (0.0 < v < math.inf):
        raise ValueError(f"{name} = {v}: finite and positive expected")
    return v


def _not_negative(name: str, v) -> float:
    v = float(v)
    if not (0.0 <= v < math.inf):
        raise ValueError(f"{name} = {v}: finite and not negative expected")
    return v


@torch.no_grad()
def voronoi_coordination(batch, select=None, cutoff: float = 13.0, tol: float = 0.1, far: float = 100.0) -> VoronoiCoordination:
    """The Voronoi coordination number of every atom of ``batch`` (``select``: a mask [N] of the atoms to evaluate) among
    the periodic images of its own system within ``cutoff`` - ``VoronoiNN(tol=tol, cutoff=cutoff).get_cn(use_weights=True)``.
    ``batch.pbc`` says which directions repeat (all, without one).  One launch for the batch, a wave per atom; no host loop."""
    cutoff, tol, far = _positive("cutoff", cutoff), _positive("tol", tol), _positive("far", far)
    g = geometry(batch, "voronoi_coordination", pbc=True)
    dev, N = g.dev, g.N
    sel = None
    if select is not None:
        sel = torch.as_tensor(select).to(dev).reshape(-1)
        if int(sel.numel()) != N:
            raise ValueError(f"select: [{N}] expected, got {list(sel.shape)}")
        sel = (sel != 0).to(torch.int32).contiguous()
    cn = torch.full((N,), math.nan, dtype=torch.float64, device=dev)
    om = torch.full((N,), math.nan, dtype=torch.float64, device=dev)
    nn = torch.zeros(N, dtype=torch.int32, device=dev)
    flags = torch.zeros(N, dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.adf_voronoi_coordination(g.pos.data_ptr(), g.cell.data_ptr(), g.pbc.data_ptr(), g.atom_offset.data_ptr(),
                                                N, g.B, None if sel is None else sel.data_ptr(), C.c_double(cutoff), C.c_double(tol),
                                                C.c_double(far), cn.data_ptr(), om.data_ptr(), nn.data_ptr(), flags.data_ptr(),
                                                stream(dev)))
    return VoronoiCoordination(cn, om, nn, (flags & 1) != 0)


@torch.no_grad()
def bulk_coordination(bulk_batch, cutoff: float = 13.0, tol: float = 0.1, far: float = 100.0) -> torch.Tensor:
    """float64 [B,119] on the device: per bulk and atomic number the least coordination number over that element's atoms,
    ``+inf`` where the bulk has none - what ``tag_surface_atoms`` compares with.  Every atom is evaluated (the reference
    takes one per symmetry class; equivalent atoms have the same cell).  A bulk atom whose cell is open is a ``ValueError``."""
    vc = voronoi_coordination(bulk_batch, None, cutoff, tol, far)
    dev = vc.cn.device
    natoms = bulk_batch.natoms.to(dev, torch.int64).reshape(-1)
    B, N = int(natoms.numel()), int(vc.cn.numel())
    Z = i32(bulk_batch.atomic_numbers, dev)
    table = torch.full((B, NUM_ELEMENTS), math.inf, dtype=torch.float64, device=dev)
    flags = vc.open.to(torch.int32).contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.adf_bulk_coordination_min(vc.cn.data_ptr(), flags.data_ptr(), Z.data_ptr(), offsets(natoms).data_ptr(),
                                                 N, B, table.data_ptr(), stream(dev)))
    return table


def _mass_table(masses, dev) -> torch.Tensor:
    m = np.asarray(default_masses() if masses is None else masses, dtype=np.float64).reshape(-1)
    if m.size == 0:
        raise ValueError("surface_tags: empty mass table")
    full = np.zeros(NUM_ELEMENTS, np.float64)               # a short table (the tests' 100 rows) is padded with zeros
    full[:min(m.size, NUM_ELEMENTS)] = m[:NUM_ELEMENTS]
    return torch.from_numpy(full).to(dev)


@torch.no_grad()
def tag_surface_atoms(slab_batch, bulk=None, height: float = 2.0, cn_tol: float = 1e-3, masses=None, cutoff: float = 13.0,
                      tol: float = 0.1, far: float = 100.0) -> Batch:
    """A copy of ``slab_batch`` with ``tags`` (int64: 1 surface, 0 the rest) and ``fixed = (tags == 0)`` - the mask of
    ``set_fixed_atom_constraints`` - set.  Every atom counts as a slab atom; the tags the batch came with are not read.
    ``bulk``: None - the height rule alone (within ``height`` A of the highest atom along the third cell vector); a batch of
    the slabs' bulks, one per slab in the same order, or a float64 [B,119] table (``bulk_coordination``) - then every other
    atom not below the centre of mass gets its Voronoi coordination and is tagged when its cell is open or its
    coordination is below its element's bulk minimum by more than ``cn_tol``.  ``masses``: a table indexed by atomic number
    (None: ``placement.default_masses``, ASE's).  The result carries ``surface_cn`` (float64 [N], NaN where not evaluated)
    and ``surface_open`` (bool [N]) per atom.  Reference order of use: tag the unit slab, then ``tile_atoms``."""
    height, cn_tol = _not_negative("height", height), _not_negative("cn_tol", cn_tol)
    cutoff, tol, far = _positive("cutoff", cutoff), _positive("tol", tol), _positive("far", far)
    g = geometry(slab_batch, "tag_surface_atoms", Z=True, pbc=True)
    dev, N, B = g.dev, g.N, g.B
    table = None
    if bulk is not None:
        if torch.is_tensor(bulk) or isinstance(bulk, np.ndarray):
            table = torch.as_tensor(bulk).to(dev, torch.float64).contiguous()
        else:
            if int(bulk.natoms.numel()) != B:
                raise ValueError(f"bulk: {int(bulk.natoms.numel())} bulks for {B} slabs (one per slab, in the same order)")
            table = bulk_coordination(bulk if bulk.pos.device == dev else bulk.clone().to(dev), cutoff, tol, far)
        if tuple(table.shape) != (B, NUM_ELEMENTS):
            raise ValueError(f"bulk: a [{B}, {NUM_ELEMENTS}] table expected, got {list(table.shape)}")
    m = _mass_table(masses, dev)
    tags = torch.zeros(N, dtype=torch.int32, device=dev)
    cn = torch.full((N,), math.nan, dtype=torch.float64, device=dev)
    flags = torch.zeros(N, dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.adf_tag_surface_atoms(g.pos.data_ptr(), g.cell.data_ptr(), g.pbc.data_ptr(), g.Z.data_ptr(),
                                             g.atom_offset.data_ptr(), N, B,
                                             m.data_ptr(), None if table is None else table.data_ptr(), C.c_double(height),
                                             C.c_double(cutoff), C.c_double(tol), C.c_double(far), C.c_double(cn_tol),
                                             tags.data_ptr(), cn.data_ptr(), flags.data_ptr(), stream(dev)))
    out = slab_batch.clone()
    out.tags = tags.to(torch.int64)
    out.fixed = (out.tags == 0).to(torch.int64)
    out.surface_cn = cn
    out.surface_open = (flags & 1) != 0
    return out


def tile_atoms(batch, min_ab: float = 8.0) -> Batch:
    """``tile_atoms`` (slab.py:324-347) for a batch: slab b is repeated ``ceil(min_ab / |a|)`` by ``ceil(min_ab / |b|)`` by 1
    times.  Atoms are image-major - copy (i, j) of the whole slab, shifted by ``i a + j b``, follows copy (i, j - 1); the a
    index is the outer one - which is the order of ``ase.Atoms.repeat`` as we read it (ASE was not run against it).  Cell
    rows a and b are scaled; every per-atom tensor of the batch is carried, per-system ones are kept.  Plain torch ops on
    whatever device the batch is on."""
    min_ab = _positive("min_ab", min_ab)
    dev = batch.pos.device
    natoms = batch.natoms.to(dev, torch.int64).reshape(-1)
    B, N = int(natoms.numel()), int(batch.pos.shape[0])
    cell = batch.cell.reshape(B, 3, 3)
    length = torch.linalg.norm(cell.double(), dim=2)
    na = torch.ceil(min_ab / length[:, 0]).long().clamp(min=1)
    nb = torch.ceil(min_ab / length[:, 1]).long().clamp(min=1)
    new_natoms = natoms * na * nb
    M = int(new_natoms.sum())
    system = torch.repeat_interleave(torch.arange(B, device=dev), new_natoms, output_size=M)
    off_new = torch.cumsum(new_natoms, 0) - new_natoms
    off_old = torch.cumsum(natoms, 0) - natoms
    local = torch.arange(M, device=dev) - off_new[system]
    image, atom = local // natoms[system], local % natoms[system]
    ia, ib = image // nb[system], image % nb[system]
    src = off_old[system] + atom
    out = Batch()
    for k, v in batch.__dict__.items():
        if k in ("batch", "natoms", "cell", "pos"):
            continue
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N and k not in _TENSOR_GRAPH_KEYS:
            out.__dict__[k] = v[src.to(v.device)]
        else:
            out.__dict__[k] = v.clone() if torch.is_tensor(v) else (list(v) if isinstance(v, list) else v)
    shift = ia.to(cell.dtype)[:, None] * cell[system, 0] + ib.to(cell.dtype)[:, None] * cell[system, 1]
    out.pos = batch.pos[src] + shift.to(batch.pos.dtype)
    new_cell = cell.clone()
    new_cell[:, 0] = cell[:, 0] * na.to(cell.dtype)[:, None]
    new_cell[:, 1] = cell[:, 1] * nb.to(cell.dtype)[:, None]
    out.cell = new_cell
    out.natoms = new_natoms
    out.batch = system
    return out
