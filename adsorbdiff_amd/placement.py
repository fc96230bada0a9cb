"""Adsorbate placement on slabs on the device: the reference's ``AdsorbateSlabConfig``
(adsorbdiff/placement/adsorbate_slab_config.py:99-439, 460-575 with adsorbate.py:122-169) in its modes ``"random"`` and
``"random_site_heuristic_placement"``, for a whole batch of slabs.

``AdsorbatePlacer.sites`` samples candidate sites on the surface triangles (``adf_place_site_candidates``) and selects
``num_sites`` of them per slab; ``AdsorbatePlacer.place`` rotates, translates and lifts the adsorbate of every placement
in one launch (``adf_place_adsorbates``) and returns the collated batch that ``Denoiser``, ``ml_relax``,
``ml_relax_sharded``, ``flag_anomalies`` and ``best_sites(group=batch.site_group)`` take as is;
``interstitial_distances`` / ``there_is_overlap`` measure the overlap of any adsorbate + slab batch
(``adf_interstitial_distances``).  ``AdsorbateSlabConfig`` is the reference's per-structure interface on top.

The rule is the contract written in include/adsorbdiff_hip.h: a reading of the reference's lines and of the ASE calls
they make.  ASE is not a dependency and was not run against it: parity with ASE is unpinned, ``radii`` and ``masses`` are
parameters.

The reference's third mode, ``"heuristic"`` (:113-116, 185-194: the ontop, bridge and hollow sites of pymatgen's
``AdsorbateSiteFinder``, all of them, each with heuristic placement), is ``heuristic_sites`` / ``place_adsorbates_heuristic``
/ ``AdsorbateSlabConfig.heuristic`` (csrc/sites.hip): the candidates and their reduction - near-duplicates,
then sites equivalent under the slab's symmetry (``slab_symmetry.find_symmetry``) - run on the device for the whole batch.
It is a written contract; pymatgen was not run against it.  ``place``, ``place_adsorbates`` and
``AdsorbateSlabConfig(...)`` keep refusing the string ``mode="heuristic"`` (``ValueError``): that mode takes no ``num_sites``
and draws no site, so it has entry points of its own.  ``reduce_sites`` runs the same reduction on any ``Sites``.

All of them start from the triangles of the tiled surface atoms: ``surface_triangles`` makes them on the host with
``scipy.spatial.Delaunay``, ``surface_triangles_device`` (csrc/triangulate.hip) on the device for the whole
batch, and every ``triangles=`` takes ``"device"`` or the ``SurfaceTriangles`` it returns besides host tables.

Draws are counter based (``adf_place_draws``): a row of eight uniforms ``(r1, r2, selection key, u0, u1, u2, binding
pick, spare)`` depends on ``(seed, noising.noise_keys(slab_batch)[b], index)`` alone, where ``index`` is the candidate's
position among its slab's candidates (``sites``) or ``site * num_augmentations_per_site + augmentation`` within its slab
(``place``).  A slab identified by ``noise_key`` or ``sid`` therefore gets the same sites and orientations alone, in any
batch, in any order and on any rank.  Every stage takes ``draws=`` to inject a table instead.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import lib as _lib
from .data import Batch
from .hostargs import desc, geometry, i32, offsets, pbc_rows, stream
from .noising import noise_keys
from .slab_symmetry import SlabSymmetry, find_symmetry

MODES = {"random": 0, "random_site_heuristic_placement": 1}
DRAW_COLUMNS = ("r1", "r2", "select", "u0", "u1", "u2", "binding", "spare")
SITE_KINDS = ("ontop", "bridge", "hollow")     # SurfaceSites.kind: 0, 1, 2


def default_radii() -> np.ndarray:
    """``ase.data.covalent_radii``.  No table is kept here: without ASE, pass one."""
    try:
        from ase.data import covalent_radii
    except ImportError as e:
        raise ImportError("placement: radii=None loads ase.data.covalent_radii and the ase package is not installed; "
                          "pass a table of radii indexed by atomic number (radii=...)") from e
    return np.asarray(covalent_radii, dtype=np.float64)


def default_masses() -> np.ndarray:
    """``ase.data.atomic_masses`` (what ``get_center_of_mass`` weighs with)."""
    try:
        from ase.data import atomic_masses
    except ImportError as e:
        raise ImportError("placement: masses=None loads ase.data.atomic_masses and the ase package is not installed; "
                          "pass a table of masses indexed by atomic number (masses=...)") from e
    return np.asarray(atomic_masses, dtype=np.float64)


def _table(values, device, what) -> torch.Tensor:
    t = torch.as_tensor(values).to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if t.numel() == 0:
        raise ValueError(f"placement: empty {what} table")
    return t


# ------------------------------------------------------------------------------------------------ surface triangles (host: scipy)
def tiling_vectors(cell: np.ndarray) -> np.ndarray:
    """The two lattice vectors ``custom_tile_atoms`` (:479-508) tiles with: the first two rows of the cell that pass its
    test ``round(v[0], 3) != 0 or round(v[1], 3 != 0)`` - as written there, the second ``round`` has one decimal."""
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    vs = [v for v in cell if (round(float(v[0]), 3) != 0) or (round(float(v[1]), 1) != 0)]
    if len(vs) < 2:
        raise ValueError("surface_triangles: the cell has fewer than two in-plane lattice vectors")
    return np.stack(vs[:2])


def surface_triangles(slab_batch) -> List[np.ndarray]:
    """Per slab a float64 ``[T,3,3]`` array of triangle vertices: the reference's tiling and pruning (:117-142).  The tag-1
    atoms are tiled 3 x 3 in the plane (the central tile first), ``scipy.spatial.Delaunay`` triangulates their x, y, and
    the triangles with at least one vertex in the central tile are kept."""
    try:
        from scipy.spatial import Delaunay
    except ImportError as e:
        raise ImportError("surface_triangles needs scipy (scipy.spatial.Delaunay), which is not installed; pass the "
                          "triangle tables yourself (triangles=...) or have them made on the device (triangles=\"device\")") from e
    pos = slab_batch.pos.detach().cpu().double().numpy()
    tags = slab_batch.tags.detach().cpu().numpy()
    cells = slab_batch.cell.detach().cpu().double().numpy().reshape(-1, 3, 3)
    natoms = slab_batch.natoms.detach().cpu().numpy().reshape(-1)
    repeats = [(0, 0)] + [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]
    out, start = [], 0
    for b, n in enumerate(natoms):
        surf = pos[start:start + n][tags[start:start + n] == 1]
        start += int(n)
        v = tiling_vectors(cells[b])
        tiled = np.concatenate([surf + i * v[0] + j * v[1] for i, j in repeats]) if len(surf) else surf
        simplices = np.zeros((0, 3), dtype=np.int64)
        if len(tiled) >= 3:
            try:
                simplices = Delaunay(tiled[:, :2]).simplices
            except Exception as e:   # QhullError: a degenerate (collinear) surface
                raise ValueError(f"surface_triangles: slab {b} cannot be triangulated: {e}") from e
            simplices = simplices[(simplices < len(surf)).any(axis=1)]
        if len(simplices) == 0:
            raise ValueError(f"surface_triangles: slab {b} has no surface triangle ({len(surf)} atoms of tag 1)")
        out.append(tiled[simplices])
    return out


# ------------------------------------------------------------------------------------------------ surface triangles (device)
class SurfaceTriangles(NamedTuple):
    """``surface_triangles_device``: ``tri`` float32 [T,3,3] (the vertices), ``tri_offset`` int32 [B+1] (slab b owns rows
    ``tri_offset[b] .. tri_offset[b+1]``) and ``index`` int32 [T,3] (the tiled indices ``tile * n_top + ordinal``, the
    least first, counter-clockwise, the rows of a slab ascending) on the device; ``counts``: triangles per slab, a host
    list."""
    tri: torch.Tensor
    tri_offset: torch.Tensor
    index: torch.Tensor
    counts: list

    def to_list(self) -> List[np.ndarray]:
        """The host form ``surface_triangles`` returns: per slab a float64 ``[T,3,3]`` array."""
        tri = self.tri.detach().cpu().double().numpy()
        bounds = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        return [tri[bounds[b]:bounds[b + 1]].copy() for b in range(len(self.counts))]


@torch.no_grad()
def surface_triangles_device(slab_batch, circle_tol: float = 1e-4) -> SurfaceTriangles:
    """``surface_triangles`` on the device for the whole batch (``adf_surface_triangles``; the contract is
    in include/adsorbdiff_hip.h): the same tiling, the Delaunay triangles of the tiled x, y with a vertex in the central
    tile, as a set what scipy returns wherever the triangulation is unique.  Points within ``circle_tol`` (A) of a
    triangle's circumcircle count as co-circular; such a polygon is split as a fan from its vertex of least x (then y).
    No scipy, no loop over slabs; one host read (the per-slab counts)."""
    circle_tol = float(circle_tol)
    if not (0.0 <= circle_tol < math.inf):
        raise ValueError(f"circle_tol = {circle_tol}: finite and not negative expected")
    if getattr(slab_batch, "tags", None) is None:
        raise ValueError("slab_batch.tags is required (tag 1 marks the surface)")
    g = geometry(slab_batch, "surface_triangles_device", tags=True)
    lib = _lib.load()
    dev, B, N = g.dev, g.B, g.N
    rows = max(18 * N, 1)                                          # always enough: fewer than 2 * 9 n_top triangles per slab
    tri = torch.empty(rows, 3, 3, dtype=torch.float32, device=dev)
    index = torch.empty(rows, 3, dtype=torch.int32, device=dev)
    tri_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_surface_triangles(g.pos.data_ptr(), g.tags.data_ptr(), g.atom_offset.data_ptr(), g.cell.data_ptr(),
                                             N, B, C.c_double(circle_tol), rows, tri_off.data_ptr(), tri.data_ptr(),
                                             index.data_ptr(), stream(dev)))
    bounds = tri_off.tolist()                                      # the one host read
    return SurfaceTriangles(tri[:bounds[-1]], tri_off, index[:bounds[-1]], [b1 - b0 for b0, b1 in zip(bounds, bounds[1:])])


def _triangle_tables(slab_batch, triangles, B: int, dev):
    """What every entry point does with ``triangles=``: (tables, tri_offset, the per-slab counts as a host list).
    ``"device"`` (``surface_triangles_device``) or a ``SurfaceTriangles``: tri float32 [T,3,3] and tri_offset int32 [B+1]
    on ``dev``, as they are - no host copy, no upload.  None (``surface_triangles``: scipy, on the host) or per slab a
    ``[T,3,3]`` array: the float64 host tables and tri_offset None - the caller packs and uploads them."""
    if isinstance(triangles, str):
        if triangles != "device":
            raise ValueError(f"triangles = {triangles!r}: None, \"device\", a SurfaceTriangles or one [T,3,3] array per slab")
        triangles = surface_triangles_device(slab_batch)
    if isinstance(triangles, SurfaceTriangles):
        if len(triangles.counts) != B or int(triangles.tri_offset.numel()) != B + 1:
            raise ValueError(f"SurfaceTriangles of {len(triangles.counts)} slabs for a batch of {B}")
        return (triangles.tri.to(dev, torch.float32).contiguous(), triangles.tri_offset.to(dev, torch.int32).contiguous(),
                [int(c) for c in triangles.counts])
    if triangles is None:
        triangles = surface_triangles(slab_batch)
    triangles = [np.asarray(t, dtype=np.float64).reshape(-1, 3, 3) for t in triangles]
    if len(triangles) != B:
        raise ValueError(f"{len(triangles)} triangle tables for {B} slabs")
    return triangles, None, [int(t.shape[0]) for t in triangles]


class Sites(NamedTuple):
    """Selected sites, slab-major: ``pos`` float32 [S,3] and ``slab`` int64 [S] on the device; ``counts`` sites per slab
    and ``slab_natoms`` atoms per slab, both host lists (the one read-back of ``AdsorbatePlacer.sites``); ``candidates``
    (float32 [C,3]), ``keep`` (bool [C]) and ``cand_slab`` (int64 [C]): everything that was sampled."""
    pos: torch.Tensor
    slab: torch.Tensor
    counts: list
    slab_natoms: list
    candidates: Optional[torch.Tensor] = None
    keep: Optional[torch.Tensor] = None
    cand_slab: Optional[torch.Tensor] = None


class SurfaceSites(NamedTuple):
    """Heuristic sites (``heuristic_sites``), slab-major, then ontop, bridge, hollow, then candidate order.  As ``Sites``:
    ``pos`` float32 [S,3], ``slab`` int64 [S], the host lists ``counts`` and ``slab_natoms``.  Per site: ``kind`` int32 [S]
    (the index into ``SITE_KINDS``), ``multiplicity`` int32 [S] (its orbit size in the cell: the distinct candidates
    equivalent to it, itself included) and ``candidate`` int64 [S] (its row of the raw tables).  The raw tables, kind-major
    within a slab: ``candidates`` float32 [C,3], ``valid`` bool [C] (False: the hollow of an obtuse triangle), ``rep``
    int32 [C] (the row of the site a candidate fell to, -1 where invalid), ``first`` int32 [C] (the same after the
    near-duplicate pass alone) and ``seg_offset`` int32 [3B+1] (segment 3 b + kind owns rows ``seg_offset[3 b + kind] ..``).
    Everything but the two lists is on the device."""
    pos: torch.Tensor
    slab: torch.Tensor
    counts: list
    slab_natoms: list
    kind: torch.Tensor
    multiplicity: torch.Tensor
    candidate: torch.Tensor
    candidates: torch.Tensor
    valid: torch.Tensor
    rep: torch.Tensor
    first: torch.Tensor
    seg_offset: torch.Tensor


class ReducedSites(NamedTuple):
    """``reduce_sites``: the kept ``sites`` (a ``Sites``, in the order they came in), ``rep`` int64 [S_in] (per site that
    went in, the index among those of the kept site it fell to) and ``multiplicity`` int32 [S_out] per kept site."""
    sites: Sites
    rep: torch.Tensor
    multiplicity: torch.Tensor


def _resolve_symmetry(symmetry, slab_batch, B: int):
    if symmetry is None or isinstance(symmetry, SlabSymmetry):
        if symmetry is not None and symmetry.num_slabs != B:
            raise ValueError(f"symmetry of {symmetry.num_slabs} slabs for a batch of {B}")
        return symmetry
    if isinstance(symmetry, str) and symmetry == "auto":
        return "auto"
    raise ValueError(f"symmetry = {symmetry!r}: \"auto\", None or a SlabSymmetry")


def _check_tol(tol) -> float:
    tol = float(tol)
    if not (0.0 <= tol < math.inf):
        raise ValueError(f"tol = {tol}: finite and not negative expected")
    return tol


def _reduce(lib, dev, slab_batch, B, cand, valid, seg_off, seg_slab, G, symmetry, tol):
    """adf_reduce_sites on a candidate table: (first, rep, multiplicity, counts [G,2]) on the device."""
    if isinstance(symmetry, str):
        symmetry = find_symmetry(slab_batch)
    C_rows = int(cand.shape[0])
    cell = slab_batch.cell.to(dev, torch.float32).reshape(B, 9).contiguous()
    first = torch.full((C_rows,), -1, dtype=torch.int32, device=dev)
    rep = torch.full((C_rows,), -1, dtype=torch.int32, device=dev)
    mult = torch.zeros(C_rows, dtype=torch.int32, device=dev)
    counts = torch.zeros(G, 2, dtype=torch.int32, device=dev)
    if symmetry is None:
        op_off = rot = trans = None
        K = 0
    else:
        op_off = symmetry.op_offset.to(dev, torch.int32).contiguous()
        rot = symmetry.rot.to(dev, torch.float64).contiguous()
        trans = symmetry.trans.to(dev, torch.float64).contiguous()
        K = int(rot.shape[0])
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.adf_reduce_sites(cand.data_ptr(), ptr(valid), seg_off.data_ptr(), ptr(seg_slab), cell.data_ptr(),
                                        C_rows, G, B, ptr(op_off), ptr(rot), ptr(trans), K, C.c_double(tol),
                                        first.data_ptr(), rep.data_ptr(), mult.data_ptr(), counts.data_ptr(), stream(dev)))
    return first, rep, mult, counts


@torch.no_grad()
def heuristic_sites(slab_batch, triangles=None, symmetry="auto", tol: float = 0.05, positions=SITE_KINDS) -> SurfaceSites:
    """The ontop, bridge and hollow sites of every slab, reduced to one per class of equivalent sites (the
    contract is in include/adsorbdiff_hip.h).  ``triangles``: per slab a ``[T,3,3]`` array (None: ``surface_triangles``, on
    the host with scipy; ``"device"``: ``surface_triangles_device``; a ``SurfaceTriangles``: used as it is, on the device).
    ``symmetry``: ``"auto"`` - ``slab_symmetry.find_symmetry(slab_batch)``; a ``SlabSymmetry`` - used as given; None - only
    near-duplicates (closer than ``tol``, in A, modulo the in-plane lattice) are merged.  ``positions``: the kinds to
    return (the raw tables always hold all three).  All sites are returned: there is no shuffle and no ``num_sites``, as in the reference's mode ``"heuristic"``.
    Two launches; beyond what ``surface_triangles`` and ``find_symmetry`` do, one host read (the per-slab counts) and no
    loop over slabs or sites."""
    positions = (positions,) if isinstance(positions, str) else tuple(positions)
    if not positions or len(set(positions)) != len(positions) or any(p not in SITE_KINDS for p in positions):
        raise ValueError(f"positions = {positions!r}: a non-empty selection of {SITE_KINDS} expected")
    tol = _check_tol(tol)
    B = int(slab_batch.natoms.numel())
    symmetry = _resolve_symmetry(symmetry, slab_batch, B)
    if getattr(slab_batch, "tags", None) is None:
        raise ValueError("slab_batch.tags is required (tag 1 marks the surface)")
    triangles, tri_off, T = _triangle_tables(slab_batch, triangles, B, slab_batch.pos.device)
    g = geometry(slab_batch, "heuristic_sites", tags=True)
    lib = _lib.load()
    dev, N, natoms = g.dev, g.N, g.natoms
    Ttot = sum(T)
    if tri_off is None:                                           # host tables: packed and uploaded
        tri = torch.from_numpy(np.concatenate(triangles).astype(np.float32) if Ttot else np.zeros((1, 3, 3), np.float32))
        tri = tri.to(dev).contiguous()
        tri_off = torch.tensor(np.concatenate([[0], np.cumsum(T)]), dtype=torch.int32, device=dev)
    else:                                                         # the device's tables, as they are
        tri = triangles if Ttot else torch.zeros(1, 3, 3, dtype=torch.float32, device=dev)
    rows = max(N + 4 * Ttot, 1)                                   # an upper bound: the tag-1 counts stay on the device
    seg_off = torch.zeros(3 * B + 1, dtype=torch.int32, device=dev)
    cand = torch.zeros(rows, 3, dtype=torch.float32, device=dev)
    valid = torch.zeros(rows, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_surface_site_candidates(g.pos.data_ptr(), g.tags.data_ptr(), g.atom_offset.data_ptr(),
                                                   g.cell.data_ptr(), tri.data_ptr(), tri_off.data_ptr(), N, Ttot, B, rows,
                                                   seg_off.data_ptr(), cand.data_ptr(), valid.data_ptr(), stream(dev)))
    seg_slab = torch.repeat_interleave(torch.arange(B, dtype=torch.int32, device=dev), 3, output_size=3 * B).contiguous()
    first, rep, mult, seg_counts = _reduce(lib, dev, slab_batch, B, cand, valid, seg_off, seg_slab, 3 * B, symmetry, tol)
    wanted = torch.tensor([k in positions for k in SITE_KINDS], device=dev)
    per_slab = (seg_counts[:, 1].long().view(B, 3) * wanted.long()).sum(1)
    so = seg_off.long()
    counts, slab_natoms, n_cand = torch.stack([per_slab, natoms, so[3::3] - so[0:-1:3]]).tolist()   # the one host read
    S, Ctot = int(sum(counts)), int(sum(n_cand))
    row = torch.arange(rows, device=dev)
    seg = torch.searchsorted(so[1:].contiguous(), row, right=True).clamp(max=3 * B - 1)
    chosen = (rep.long() == row) & wanted[seg % 3]
    order = torch.sort((~chosen).long(), stable=True).indices[:S]   # the chosen rows, ascending
    return SurfaceSites(cand[order].contiguous(), (seg[order] // 3).contiguous(), counts, slab_natoms,
                        (seg[order] % 3).to(torch.int32), mult[order].contiguous(), order, cand[:Ctot], valid[:Ctot] != 0,
                        rep[:Ctot], first[:Ctot], seg_off)


# ------------------------------------------------------------------------------------------------ the placer
class AdsorbatePlacer:
    """Sites and placements for batches of slabs on one device.  ``radii`` / ``masses``: tables indexed by atomic number
    (None: ASE's ``covalent_radii`` / ``atomic_masses``)."""

    def __init__(self, radii=None, masses=None, device="cuda:0", seed: int = 0) -> None:
        radii = default_radii() if radii is None else radii      # before the device check: a missing ase is reported first
        masses = default_masses() if masses is None else masses
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("AdsorbatePlacer needs a ROCm device (the HIP path has no CPU fallback)")
        self.lib = _lib.load()
        self.radii = _table(radii, self.dev, "radius")
        self.masses = _table(masses, self.dev, "mass")
        self.seed = int(seed)

    # ---- draws
    def draws(self, keys, index) -> torch.Tensor:
        """float64 [n,8] rows of (seed, keys[i], index[i]); the columns are ``DRAW_COLUMNS``."""
        keys = torch.as_tensor(keys).reshape(-1)
        if keys.dtype != torch.int64:
            raise ValueError(f"keys: int64 expected, got {keys.dtype}")
        keys = keys.to(self.dev).contiguous()
        index = i32(index, self.dev).reshape(-1)
        n = int(keys.numel())
        if int(index.numel()) != n:
            raise ValueError(f"{n} keys, {int(index.numel())} indices")
        out = torch.empty(n, 8, dtype=torch.float64, device=self.dev)
        seed = self.seed & 0xFFFFFFFFFFFFFFFF
        seed = seed - (1 << 64) if seed >= (1 << 63) else seed
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.adf_place_draws(seed, keys.data_ptr(), index.data_ptr(), n, out.data_ptr(), stream(self.dev)))
        return out

    def _draw_table(self, draws, n: int) -> torch.Tensor:
        if not torch.is_tensor(draws):
            draws = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float64))
        draws = draws.to(self.dev, torch.float64).contiguous()
        if tuple(draws.shape) != (n, 8):
            raise ValueError(f"draws: [{n}, 8] expected, got {list(draws.shape)}")
        return draws

    # ---- sites
    @torch.no_grad()
    def sites(self, slab_batch, num_sites: int, triangles=None, draws=None) -> Sites:
        """Up to ``num_sites`` sites per slab (fewer where fewer candidates fall into the central cell, as in the
        reference).  ``triangles``: per slab a ``[T,3,3]`` array (None: ``surface_triangles``; ``"device"`` or a
        ``SurfaceTriangles``: ``surface_triangles_device``'s tables, used on the device as they are); ``draws``: [C,8] rows for the
        C = sum_b T_b ceil(2 num_sites / T_b) candidates in slab-major, triangle-major order.  The kept candidates of a slab
        are ordered by ascending selection key (ties: candidate index) and the first ``num_sites`` are taken; this
        replaces the reference's ``np.random.shuffle``.  One host read: the per-slab counts."""
        num_sites = int(num_sites)
        if num_sites < 1:
            raise ValueError(f"num_sites = {num_sites}")
        dev = self.dev
        B = int(slab_batch.natoms.numel())
        triangles, tri_off, T = _triangle_tables(slab_batch, triangles, B, dev)
        if min(T) == 0:
            raise ValueError(f"slab {T.index(0)} has no triangle")
        per = [int(math.ceil(2.0 * num_sites / t)) for t in T]
        n_cand = [t * p for t, p in zip(T, per)]
        Ctot = sum(n_cand)
        if tri_off is None:                                       # host tables: packed and uploaded
            tri = torch.from_numpy(np.concatenate(triangles).astype(np.float32)).to(dev).contiguous()
            tri_off = torch.tensor(np.concatenate([[0], np.cumsum(T)]), dtype=torch.int32, device=dev)
        else:                                                     # the device's tables, as they are
            tri = triangles
        per_t = torch.tensor(per, dtype=torch.int32, device=dev)
        cand_counts = torch.tensor(n_cand, dtype=torch.int64, device=dev)
        cand_off = offsets(cand_counts)
        cand_slab = torch.repeat_interleave(torch.arange(B, device=dev), cand_counts, output_size=Ctot)
        local = torch.arange(Ctot, device=dev) - cand_off.long()[cand_slab]
        if draws is None:
            draws = self.draws(noise_keys(slab_batch).to(dev)[cand_slab], local)
        draws = self._draw_table(draws, Ctot)
        cell = slab_batch.cell.to(dev, torch.float32).reshape(B, 9).contiguous()
        cand = torch.empty(Ctot, 3, dtype=torch.float32, device=dev)
        keep = torch.empty(Ctot, dtype=torch.int32, device=dev)
        slab32 = cand_slab.to(torch.int32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(self.lib.adf_place_site_candidates(tri.data_ptr(), tri_off.data_ptr(), per_t.data_ptr(),
                                                          cand_off.data_ptr(), slab32.data_ptr(), cell.data_ptr(),
                                                          draws.data_ptr(), B, Ctot, cand.data_ptr(), keep.data_ptr(),
                                                          stream(dev)))
        keep = keep != 0
        # order: slab, kept first, selection key, candidate index (two stable sorts)
        by_key = torch.sort(draws[:, 2], stable=True).indices
        group = cand_slab[by_key] * 2 + (~keep[by_key]).long()
        order = by_key[torch.sort(group, stable=True).indices]
        rank = torch.arange(Ctot, device=dev) - cand_off.long()[cand_slab[order]]
        chosen = keep[order] & (rank < num_sites)
        counts_dev = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, cand_slab[order], chosen.long())
        both = torch.stack([counts_dev, slab_batch.natoms.to(dev).reshape(-1).long()]).tolist()   # the one host read
        counts, slab_natoms = both
        S = int(sum(counts))
        first = order[torch.sort((~chosen).long(), stable=True).indices[:S]]   # the chosen ones, in order
        return Sites(cand[first].contiguous(), cand_slab[first].contiguous(), counts, slab_natoms, cand, keep, cand_slab)

    def _as_sites(self, slab_batch, sites) -> Sites:
        B = int(slab_batch.natoms.numel())
        if isinstance(sites, (Sites, SurfaceSites)):
            return sites
        natoms = slab_batch.natoms.reshape(-1).tolist()
        if isinstance(sites, (list, tuple)) and len(sites) == 2 and torch.is_tensor(sites[1]) and sites[1].dim() == 1 \
                and torch.is_tensor(sites[0]) and sites[0].dim() == 2:
            pos = sites[0].to(self.dev, torch.float32).reshape(-1, 3)
            slab = sites[1].to(self.dev).long().reshape(-1)
            if int(slab.numel()) != int(pos.shape[0]):
                raise ValueError("sites: positions and slab ids differ in length")
            order = torch.sort(slab, stable=True).indices
            pos, slab = pos[order].contiguous(), slab[order].contiguous()
            counts = torch.bincount(slab, minlength=B).tolist()
            if len(counts) != B or (slab.numel() and int(slab.min()) < 0):
                raise ValueError(f"sites: slab ids outside [0, {B})")
            return Sites(pos, slab, counts, natoms)
        if isinstance(sites, (list, tuple)):
            if len(sites) != B:
                raise ValueError(f"sites: {len(sites)} entries for {B} slabs")
            per = [torch.as_tensor(np.asarray(s.detach().cpu() if torch.is_tensor(s) else s, dtype=np.float64)).reshape(-1, 3)
                   for s in sites]
        else:
            arr = torch.as_tensor(np.asarray(sites.detach().cpu() if torch.is_tensor(sites) else sites, dtype=np.float64))
            if B != 1:
                raise ValueError("sites: one [n,3] array per slab is needed for a batch of several slabs")
            per = [arr.reshape(-1, 3)]
        counts = [int(s.shape[0]) for s in per]
        pos = torch.cat(per).to(self.dev, torch.float32).contiguous()
        slab = torch.repeat_interleave(torch.arange(B), torch.tensor(counts)).to(self.dev)
        return Sites(pos, slab, counts, natoms)

    # ---- heuristic sites and the reduction of any sites
    def heuristic_sites(self, slab_batch, triangles=None, symmetry="auto", tol: float = 0.05, positions=SITE_KINDS) -> SurfaceSites:
        """The module's ``heuristic_sites`` (which needs no radii or masses)."""
        return heuristic_sites(slab_batch, triangles, symmetry, tol, positions)

    @torch.no_grad()
    def reduce_sites(self, slab_batch, sites, symmetry="auto", tol: float = 0.05) -> ReducedSites:
        """The reduction of ``heuristic_sites`` on any sites - those of ``sites()``, or whatever ``place(sites=)`` takes -
        all of one kind: per slab, in the order given, a site is kept unless a kept one before it lies within ``tol`` of it,
        first as it is, then under the slab's operations (``symmetry`` as in ``heuristic_sites``).  One host read."""
        tol = _check_tol(tol)
        B = int(slab_batch.natoms.numel())
        symmetry = _resolve_symmetry(symmetry, slab_batch, B)
        st = self._as_sites(slab_batch, sites)
        S = int(st.pos.shape[0])
        if S == 0:
            raise ValueError("reduce_sites: no site")
        dev = self.dev
        cand = st.pos.to(dev, torch.float32).contiguous()
        seg_off = torch.tensor(np.concatenate([[0], np.cumsum(st.counts)]), dtype=torch.int32, device=dev)
        _, rep, mult, seg_counts = _reduce(self.lib, dev, slab_batch, B, cand, None, seg_off, None, B, symmetry, tol)
        counts = seg_counts[:, 1].tolist()                          # the one host read
        kept = rep.long() == torch.arange(S, device=dev)
        order = torch.sort((~kept).long(), stable=True).indices[:sum(counts)]
        new_index = torch.cumsum(kept.long(), 0) - 1
        slab = st.slab.to(dev)
        return ReducedSites(Sites(cand[order].contiguous(), slab[order].contiguous(), counts, list(st.slab_natoms)),
                            new_index[rep.long()], mult[order].contiguous())

    # ---- placements
    @torch.no_grad()
    def place(self, slab_batch, adsorbates, sites, num_augmentations_per_site: int = 1, interstitial_gap: float = 0.1,
              mode: str = "random", binding_indices=None, draws=None) -> Batch:
        """Place ``adsorbates`` on ``sites``: a collated ``Batch`` of all placements, slab-major, then site, then
        augmentation.  ``adsorbates``: one ``(Z, pos)`` for all slabs or one per slab; ``sites``: what ``sites()`` returned,
        or per slab an [n,3] array, or ``(pos [S,3], slab [S])`` tensors; ``binding_indices`` (heuristic placement): one
        list of atom indices, or one per slab; ``draws``: [P,8] rows, one per placement.  The batch carries ``site_group``
        (the slab of every placement) and ``site_index`` (int32 [P]: its number within that slab); with the ``SurfaceSites``
        of ``heuristic_sites`` also ``site_kind`` and ``site_multiplicity`` (int32 [P]).  ``mode="heuristic"`` is refused
        here: that is ``place_adsorbates_heuristic``."""
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(MODES)} (the reference's mode \"heuristic\" is "
                             "place_adsorbates_heuristic / AdsorbateSlabConfig.heuristic, or sites=heuristic_sites(...) "
                             "with mode=\"random_site_heuristic_placement\")")
        gap = float(interstitial_gap)
        if not (0.0 <= gap < 5.0):
            raise ValueError(f"interstitial_gap = {gap}: 0 <= gap < 5 expected")
        n_aug = int(num_augmentations_per_site)
        if n_aug < 1:
            raise ValueError(f"num_augmentations_per_site = {n_aug}")
        if mode != "random" and binding_indices is None:
            raise ValueError(f"mode {mode!r} places the binding atom on the site: binding_indices= is required")
        dev = self.dev
        B = int(slab_batch.natoms.numel())
        st = self._as_sites(slab_batch, sites)
        S = int(st.pos.shape[0])
        if S == 0:
            raise ValueError("place: no site")
        P = S * n_aug
        # adsorbates as CSR over the slabs
        if isinstance(adsorbates, (list, tuple)) and len(adsorbates) == 2 and not isinstance(adsorbates[0], (list, tuple)) \
                and np.asarray(adsorbates[0]).ndim == 1 and np.asarray(adsorbates[1]).ndim == 2:
            adsorbates = [adsorbates] * B
        if len(adsorbates) != B:
            raise ValueError(f"{len(adsorbates)} adsorbates for {B} slabs")
        ads_Z = [np.asarray(a[0]).astype(np.int64).reshape(-1) for a in adsorbates]
        ads_P = [np.asarray(a[1], dtype=np.float64).reshape(-1, 3) for a in adsorbates]
        n_ads = [len(z) for z in ads_Z]
        if min(n_ads) == 0 or any(len(z) != len(p) for z, p in zip(ads_Z, ads_P)):
            raise ValueError("adsorbates: (Z [n], pos [n,3]) with n >= 1 expected")
        adsZ_t = torch.from_numpy(np.concatenate(ads_Z)).to(dev)
        adsZ32 = adsZ_t.to(torch.int32).contiguous()
        adsP_t = torch.from_numpy(np.concatenate(ads_P).astype(np.float32)).to(dev).contiguous()
        n_ads_t = torch.tensor(n_ads, dtype=torch.int64, device=dev)
        ads_off = offsets(n_ads_t)
        # placements
        slab_of = torch.repeat_interleave(st.slab, n_aug, output_size=P)
        site = torch.repeat_interleave(st.pos, n_aug, dim=0, output_size=P).contiguous()
        site_off = offsets(torch.tensor(st.counts, dtype=torch.int64, device=dev)).long() * n_aug
        local = torch.arange(P, device=dev) - site_off[slab_of]
        if draws is None:
            draws = self.draws(noise_keys(slab_batch).to(dev)[slab_of], local)
        draws = self._draw_table(draws, P)
        bind = None
        if mode != "random":
            if len(binding_indices) > 0 and not isinstance(binding_indices[0], (list, tuple, np.ndarray)):
                binding_indices = [binding_indices] * B
            if len(binding_indices) != B or min(len(x) for x in binding_indices) == 0:
                raise ValueError("binding_indices: one non-empty list of atom indices, or one per slab")
            for x, n in zip(binding_indices, n_ads):
                if min(x) < 0 or max(x) >= n:
                    raise ValueError(f"binding index outside the adsorbate ({n} atoms)")
            n_b = torch.tensor([len(x) for x in binding_indices], dtype=torch.int64, device=dev)
            flat = torch.tensor([int(i) for x in binding_indices for i in x], dtype=torch.int32, device=dev)
            pick = torch.minimum((draws[:, 6] * n_b[slab_of].double()).floor().long(), n_b[slab_of] - 1)
            bind = flat[offsets(n_b).long()[slab_of] + pick].contiguous()
        # the collated output: slab rows gathered, adsorbate rows written by the kernel
        n_slab_t = torch.tensor(st.slab_natoms, dtype=torch.int64, device=dev)
        natoms_p = (n_slab_t + n_ads_t)[slab_of]
        N = sum(c * n_aug * (ns + na) for c, ns, na in zip(st.counts, st.slab_natoms, n_ads))
        off_p = offsets(natoms_p).long()
        batch_idx = torch.repeat_interleave(torch.arange(P, device=dev), natoms_p, output_size=N)
        loc = torch.arange(N, device=dev) - off_p[batch_idx]
        sys_slab = slab_of[batch_idx]
        is_slab = loc < n_slab_t[sys_slab]
        slab_off = offsets(n_slab_t)
        src = torch.where(is_slab, slab_off.long()[sys_slab] + loc, torch.zeros_like(loc))
        asrc = torch.where(is_slab, torch.zeros_like(loc), ads_off.long()[sys_slab] + loc - n_slab_t[sys_slab])
        slab_pos = slab_batch.pos.detach().to(dev, torch.float32).contiguous()
        Nslab = int(slab_pos.shape[0])
        if Nslab != sum(st.slab_natoms):
            raise ValueError(f"slab_batch.pos has {Nslab} rows, natoms sum to {sum(st.slab_natoms)}")
        slab_Z = slab_batch.atomic_numbers.to(dev)
        pos = slab_pos[src].contiguous() if Nslab else torch.zeros(N, 3, dtype=torch.float32, device=dev)
        out_row = (off_p[:P] + n_slab_t[slab_of]).to(torch.int32).contiguous()
        cell = slab_batch.cell.to(dev, torch.float32).reshape(B, 9).contiguous()
        slabZ32 = i32(slab_Z, dev)
        d = desc(slab_pos, cell, slabZ32, slab_off, B, Nslab)
        pbc = pbc_rows(slab_batch, B, dev)
        slab32 = slab_of.to(torch.int32).contiguous()
        sn = torch.empty(P, dtype=torch.float64, device=dev)
        nc = torch.empty(P, dtype=torch.int32, device=dev)
        meta = torch.empty(P, 4, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self.lib.adf_place_adsorbates(
                C.byref(d), slab32.data_ptr(), site.data_ptr(), draws.data_ptr(), ads_off.data_ptr(), adsP_t.data_ptr(),
                adsZ32.data_ptr(), self.radii.data_ptr(), int(self.radii.numel()), self.masses.data_ptr(),
                int(self.masses.numel()), C.c_float(gap), MODES[mode], None if bind is None else bind.data_ptr(),
                pbc.data_ptr(), P, out_row.data_ptr(), N, pos.data_ptr(), sn.data_ptr(), nc.data_ptr(), meta.data_ptr(),
                stream(dev)))
        out = Batch()
        out.pos = pos
        out.atomic_numbers = torch.where(is_slab, slab_Z[src].long(), adsZ_t[asrc]).to(slab_Z.dtype) if Nslab \
            else adsZ_t[asrc].to(slab_Z.dtype)
        tags = getattr(slab_batch, "tags", None)
        if tags is None:
            raise ValueError("slab_batch.tags is required (tag 1 marks the surface)")
        tags = tags.to(dev)
        out.tags = torch.where(is_slab, tags[src], torch.full_like(tags[src], 2)) if Nslab else torch.full((N,), 2, device=dev)
        fixed = getattr(slab_batch, "fixed", None)
        if fixed is not None:
            fixed = fixed.to(dev)
            out.fixed = torch.where(is_slab, fixed[src], torch.zeros_like(fixed[src])) if Nslab \
                else torch.zeros(N, dtype=torch.long, device=dev)
        out.cell = slab_batch.cell.to(dev).reshape(B, 3, 3)[slab_of]
        out.natoms = natoms_p
        out.batch = batch_idx
        out.pbc = torch.tensor([True, True, False], device=dev).expand(P, 3).contiguous()   # as the reference sets it (:252)
        sid = getattr(slab_batch, "sid", None)
        if sid is not None and len(sid) == B:
            out.sid = [sid[b] for b, c in enumerate(st.counts) for _ in range(c * n_aug)]
        out.site_group = slab_of
        # the placement's number within its slab: what its own draws are keyed by, and what the sampler's keyed noise
        # (denoising_pos_params["noise_seed"]) tells the replicas of one slab apart by - they share a sid
        out.site_index = local.to(torch.int32)
        if getattr(slab_batch, "noise_key", None) is not None:
            out.noise_key = noise_keys(slab_batch).to(dev)[slab_of]
        out.site = site
        out.xyz_angles = meta
        out.scaled_normal = sn
        out.n_combos = nc
        if bind is not None:
            out.binding_idx = bind
        if isinstance(st, SurfaceSites):
            out.site_kind = torch.repeat_interleave(st.kind, n_aug, output_size=P)
            out.site_multiplicity = torch.repeat_interleave(st.multiplicity, n_aug, output_size=P)
        return out


def place_adsorbates(slab_batch, adsorbates, num_sites: int, num_augmentations_per_site: int = 1,
                     interstitial_gap: float = 0.1, mode: str = "random", binding_indices=None, radii=None, masses=None,
                     triangles=None, sites=None, seed: int = 0, device=None, placer: AdsorbatePlacer = None) -> Batch:
    """Sites and placements in one call: ``AdsorbatePlacer(...).sites`` (unless ``sites=`` are given) and ``.place``."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    if not (0.0 <= float(interstitial_gap) < 5.0):
        raise ValueError(f"interstitial_gap = {interstitial_gap}: 0 <= gap < 5 expected")
    if placer is None:
        placer = AdsorbatePlacer(radii, masses, device=slab_batch.pos.device if device is None else device, seed=seed)
    if sites is None:
        sites = placer.sites(slab_batch, num_sites, triangles=triangles)
    return placer.place(slab_batch, adsorbates, sites, num_augmentations_per_site, interstitial_gap, mode, binding_indices)


def place_adsorbates_heuristic(slab_batch, adsorbates, binding_indices, num_augmentations_per_site: int = 1,
                               interstitial_gap: float = 0.1, radii=None, masses=None, triangles=None, symmetry="auto",
                               tol: float = 0.05, positions=SITE_KINDS, seed: int = 0, device=None,
                               placer: AdsorbatePlacer = None) -> Batch:
    """The reference's mode ``"heuristic"`` (:113-116, 185-194, 208, 223) for a batch: ``heuristic_sites`` - every ontop,
    bridge and hollow site, one per class of equivalent sites - and on each of them ``place`` with
    ``mode="random_site_heuristic_placement"``, the rule the reference applies there.  The batch also carries ``site_kind``
    and ``site_multiplicity`` per placement.  (``place_adsorbates(mode="heuristic")`` stays a ``ValueError``.)"""
    if not (0.0 <= float(interstitial_gap) < 5.0):
        raise ValueError(f"interstitial_gap = {interstitial_gap}: 0 <= gap < 5 expected")
    if placer is None:
        placer = AdsorbatePlacer(radii, masses, device=slab_batch.pos.device if device is None else device, seed=seed)
    sites = placer.heuristic_sites(slab_batch, triangles, symmetry, tol, positions)
    return placer.place(slab_batch, adsorbates, sites, num_augmentations_per_site, interstitial_gap,
                        "random_site_heuristic_placement", binding_indices)


# ------------------------------------------------------------------------------------------------ overlap
@torch.no_grad()
def interstitial_distances(batch, radii=None, masses=None) -> torch.Tensor:
    """float32 [B] on the device: per system the least ``|p_a - p_s| - R_a - R_s`` over (surface atom of tag 1, adsorbate
    atom of tag 2), ``+inf`` without such a pair (``get_interstitial_distances``, :511-559, reduced to its minimum)."""
    radii = default_radii() if radii is None else radii
    masses = default_masses() if masses is None else masses
    g = geometry(batch, "interstitial_distances", Z=True, tags=True, pbc=True)
    lib = _lib.load()
    dev = g.dev
    r, m = _table(radii, dev, "radius"), _table(masses, dev, "mass")
    d = desc(g.pos, g.cell, g.Z, g.atom_offset, g.B, g.N)
    out = torch.empty(g.B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.adf_interstitial_distances(C.byref(d), g.tags.data_ptr(), r.data_ptr(), int(r.numel()), m.data_ptr(),
                                                  int(m.numel()), g.pbc.data_ptr(), out.data_ptr(), stream(dev)))
    return out


def there_is_overlap(batch, radii=None, masses=None) -> torch.Tensor:
    """bool [B]: some surface atom and adsorbate atom are closer than the sum of their radii (:562-575)."""
    return ~(interstitial_distances(batch, radii, masses) >= 0)


# ------------------------------------------------------------------------------------------------ the reference's interface
def _get(obj, name):
    getter = getattr(obj, "get_" + name, None)
    return getter() if callable(getter) else getattr(obj, name)


def _atoms_batch(atoms, dev) -> Batch:
    b = Batch()
    pos = np.asarray(_get(atoms, "positions"), dtype=np.float64).reshape(-1, 3)
    b.pos = torch.as_tensor(pos, dtype=torch.float32, device=dev)
    b.cell = torch.as_tensor(np.asarray(atoms.cell, dtype=np.float64).reshape(1, 3, 3), dtype=torch.float32, device=dev)
    b.atomic_numbers = torch.as_tensor(np.asarray(atoms.numbers), dtype=torch.long, device=dev)
    b.tags = torch.as_tensor(np.asarray(_get(atoms, "tags")), dtype=torch.long, device=dev)
    b.fixed = torch.zeros(len(pos), dtype=torch.long, device=dev)
    b.natoms = torch.tensor([len(pos)], dtype=torch.long, device=dev)
    b.batch = torch.zeros(len(pos), dtype=torch.long, device=dev)
    pbc = getattr(atoms, "pbc", None)
    if pbc is not None:
        b.pbc = torch.as_tensor(np.broadcast_to(np.asarray(pbc, dtype=bool), (3,)).copy()).reshape(1, 3)
    return b


def _one_slab_triangles(triangles):
    """``triangles=`` of the one-structure interface: None, ``"device"`` and a ``SurfaceTriangles`` pass, a ``[T,3,3]``
    array becomes the list of one table."""
    return triangles if triangles is None or isinstance(triangles, (str, SurfaceTriangles)) else [triangles]


class AdsorbateSlabConfig:
    """The reference's interface (:22-97) on the batched call, with its keyword names.  ``slab.atoms`` and
    ``adsorbate.atoms`` are duck-typed (``positions`` / ``get_positions()``, ``cell``, ``numbers``, ``tags`` /
    ``get_tags()``, ``pbc``); ``adsorbate.binding_indices`` is read in the heuristic-placement mode.  Exposes ``sites``
    ([S,3] numpy), ``batch`` (the collated placements) and ``metadata_list`` (``{"site", "xyz_angles": [zrot, rotvec]}``
    per placement).  ``triangles``: one ``[T,3,3]`` table, ``"device"`` or a ``SurfaceTriangles`` (None: scipy on the
    host).  ASE ``atoms_list`` objects are not built (ASE is not a dependency)."""

    def __init__(self, slab, adsorbate, num_sites: int = 1, num_augmentations_per_site: int = 1,
                 interstitial_gap: float = 0.1, mode: str = "random", sites=None, radii=None, masses=None,
                 triangles=None, device="cuda:0", seed: int = 0):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
        if not (0.0 <= float(interstitial_gap) < 5.0):
            raise ValueError(f"interstitial_gap = {interstitial_gap}: 0 <= gap < 5 expected")
        self.slab, self.adsorbate = slab, adsorbate
        self.num_sites, self.num_augmentations_per_site = num_sites, num_augmentations_per_site
        self.interstitial_gap, self.mode = interstitial_gap, mode
        placer = AdsorbatePlacer(radii, masses, device=device, seed=seed)
        sb = _atoms_batch(slab.atoms, placer.dev)
        if sites is None:
            st = placer.sites(sb, num_sites, triangles=_one_slab_triangles(triangles))
        else:
            st = [np.asarray(sites, dtype=np.float64).reshape(-1, 3)]
        self._place(placer, sb, st, mode)

    @classmethod
    def heuristic(cls, slab, adsorbate, num_augmentations_per_site: int = 1, interstitial_gap: float = 0.1, radii=None,
                  masses=None, triangles=None, symmetry="auto", tol: float = 0.05, positions=SITE_KINDS, device="cuda:0",
                  seed: int = 0):
        """The reference's ``mode="heuristic"`` for one structure: every site of ``heuristic_sites``, heuristic placement on
        each.  Also exposes ``surface_sites`` (the ``SurfaceSites``).  The constructor keeps refusing that mode string."""
        if not (0.0 <= float(interstitial_gap) < 5.0):
            raise ValueError(f"interstitial_gap = {interstitial_gap}: 0 <= gap < 5 expected")
        self = cls.__new__(cls)
        self.slab, self.adsorbate = slab, adsorbate
        self.num_sites, self.num_augmentations_per_site = None, num_augmentations_per_site
        self.interstitial_gap, self.mode = interstitial_gap, "heuristic"
        placer = AdsorbatePlacer(radii, masses, device=device, seed=seed)
        sb = _atoms_batch(slab.atoms, placer.dev)
        st = placer.heuristic_sites(sb, _one_slab_triangles(triangles), symmetry, tol, positions)
        self.surface_sites = st
        self._place(placer, sb, st, "random_site_heuristic_placement")
        return self

    def _place(self, placer, sb, st, mode):
        a = self.adsorbate.atoms
        ads = (np.asarray(a.numbers), np.asarray(_get(a, "positions"), dtype=np.float64).reshape(-1, 3))
        binding = None if mode == "random" else list(getattr(self.adsorbate, "binding_indices"))
        self.batch = placer.place(sb, ads, st, self.num_augmentations_per_site, self.interstitial_gap, mode, binding)
        self.sites = (st.pos if isinstance(st, (Sites, SurfaceSites)) else torch.as_tensor(st[0])).detach().cpu().double().numpy()
        site = self.batch.site.detach().cpu().double().numpy()
        meta = self.batch.xyz_angles.detach().cpu().numpy()
        self.metadata_list = [{"site": site[p], "xyz_angles": [float(meta[p, 0]), meta[p, 1:4].copy()]}
                              for p in range(site.shape[0])]
