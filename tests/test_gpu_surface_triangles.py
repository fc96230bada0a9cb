"""GPU tests of the device triangulation (csrc/triangulate.hip; placement.surface_triangles_device and ``triangles="device"``;
DESIGN.md 4l).  Where the triangulation is unique the table must equal what scipy.spatial.Delaunay kept, recorded in
tests/golden/surface_triangles.npz (no scipy here): the index rows exactly, the float32 vertices bit for bit.  On the perfect
rectangular lattices, where it is not, every triangle must be admissible for the float64 oracle of
tests/helpers_surface_triangles.py, the table must be the contract's fan, and the invariants that need no oracle must hold."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import placement as PL
from tests import helpers_heuristic_sites as HH
from tests import helpers_placement as HP
from tests import helpers_slab_symmetry as HS
from tests import helpers_surface_triangles as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GENERIC = ("generic3_0", "generic3_1", "generic3_2")


def fixture_cases(names):
    fx = H.load_fixture()
    return [fx[n] for n in names]


def slab_rows(st, b):
    """(index int64 [T,3], tri float32 [T,3,3]) of slab b."""
    off = st.tri_offset.cpu().numpy().astype(np.int64)
    return st.index[off[b]:off[b + 1]].cpu().numpy().astype(np.int64), st.tri[off[b]:off[b + 1]].cpu()


def slab_bits(st, b):
    idx, tri = slab_rows(st, b)
    return torch.from_numpy(idx), tri.view(torch.int32)


@functools.lru_cache(maxsize=None)
def generic_run():
    return PL.surface_triangles_device(H.batch_of(fixture_cases(GENERIC), DEV))


def check_against_fixture(st, b, fx):
    idx, tri = slab_rows(st, b)
    assert idx.shape == fx["index"].shape and (idx == fx["index"]).all()
    assert tri.dtype == torch.float32 and torch.equal(tri.view(torch.int32), torch.from_numpy(fx["vertices"]).view(torch.int32))
    pts, n_top = H.tiled_points(fx["pos"], fx["tags"], fx["cell"])
    H.check_table(pts[:, :2], n_top, idx)                            # a the least index, counter-clockwise, ascending
    assert st.counts[b] == len(fx["index"])


# 1
def test_generic_batch_equals_the_recorded_scipy_tables():
    st = generic_run()
    cases = fixture_cases(GENERIC)
    for b, fx in enumerate(cases):
        check_against_fixture(st, b, fx)
    T = [len(fx["index"]) for fx in cases]
    assert st.counts == T and st.tri_offset.tolist() == np.concatenate([[0], np.cumsum(T)]).tolist()
    assert st.tri.shape == (sum(T), 3, 3) and st.index.shape == (sum(T), 3)
    assert st.tri_offset.dtype == torch.int32 and st.index.dtype == torch.int32 and st.tri.is_cuda and st.index.is_cuda
    host = st.to_list()
    assert [t.shape for t in host] == [(t, 3, 3) for t in T] and host[0].dtype == np.float64


# 2
def test_perfect_hexagonal_lattice_equals_the_recorded_scipy_table():
    fx = H.load_fixture()["111_3x3x4"]
    check_against_fixture(PL.surface_triangles_device(H.batch_of([fx], DEV)), 0, fx)


# 3
def test_rectangular_lattices_get_the_fan_with_parallel_diagonals():
    st = PL.surface_triangles_device(H.batch_of([H.lattice(n) for n in H.DEGENERATE], DEV))
    for b, name in enumerate(H.DEGENERATE):
        xy, n_top, res = H.oracle(name)
        idx, _ = slab_rows(st, b)
        admissible = {tuple(t) for t in H.rows_of(res, "admissible", xy)}
        assert all(tuple(t) in admissible for t in idx), name
        H.check_table(xy, n_top, idx)                                # star closed within 1e-9, every area > 0
        d = H.longest_edge_directions(xy, idx)
        assert np.abs(d - d[0]).max() < 1e-6, name                   # every rectangle is split along the same diagonal
        want = H.expected(xy, n_top, res=res)
        assert idx.shape == want.shape and (idx == want).all(), name


# 4
def test_heuristic_sites_on_device_triangles_gives_the_known_counts():
    names = list(H.LATTICES)
    st = PL.heuristic_sites(HH.slab_batch(names, DEV), triangles="device")
    for b, name in enumerate(names):
        kinds = st.kind[st.slab == b].cpu().numpy()
        assert tuple(int((kinds == k).sum()) for k in range(3)) == HH.TABLE[name][1], name
    assert st.multiplicity[st.slab == names.index("111_3x3x4")].tolist() == [9, 27, 9, 9]


def site_bits(st):
    return [t.cpu() for t in (st.pos.view(torch.int32), st.slab, st.kind, st.multiplicity, st.candidate,
                              st.candidates.view(torch.int32), st.valid, st.rep, st.first, st.seg_offset)] + [st.counts, st.slab_natoms]


def test_heuristic_sites_on_device_triangles_equals_the_host_tables():
    cases = fixture_cases(GENERIC)
    sb = H.batch_of(cases, DEV)
    host = [fx["vertices"].astype(np.float64) for fx in cases]      # scipy's triangles, in the device's order
    for tri in ("device", generic_run()):
        a, b = PL.heuristic_sites(sb, tri, symmetry=None), PL.heuristic_sites(sb, host, symmetry=None)
        assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(site_bits(a), site_bits(b)))
        assert sum(a.counts) > 0


# 5
def test_placer_sites_on_device_triangles_equals_the_table_passed_back():
    sb = H.batch_of(fixture_cases(GENERIC), DEV)
    placer = PL.AdsorbatePlacer(HP.synthetic_radii(), HP.synthetic_masses(), device=DEV, seed=3)
    a = placer.sites(sb, 4, triangles="device")
    b = placer.sites(sb, 4, triangles=generic_run().to_list())
    c = placer.sites(sb, 4, triangles=generic_run())
    for other in (b, c):
        for x, y in zip((a.pos, a.slab, a.candidates, a.keep, a.cand_slab), (other.pos, other.slab, other.candidates, other.keep,
                                                                             other.cand_slab)):
            assert torch.equal(x, y)
        assert a.counts == other.counts and a.slab_natoms == other.slab_natoms
    assert len(a.counts) == 3 and max(a.counts) <= 4 and sum(a.counts) > 0


# 6
def test_a_slab_gets_the_same_rows_alone_reversed_and_twice():
    cases = fixture_cases(GENERIC)
    st = generic_run()
    again = PL.surface_triangles_device(H.batch_of(cases, DEV))
    rev = PL.surface_triangles_device(H.batch_of(cases[::-1], DEV))
    for b, fx in enumerate(cases):
        alone = PL.surface_triangles_device(H.batch_of([fx], DEV))
        for other, ob in ((again, b), (rev, len(cases) - 1 - b), (alone, 0)):
            assert all(torch.equal(x, y) for x, y in zip(slab_bits(st, b), slab_bits(other, ob)))


# 7
def raw_call(cases, capacity, circle_tol=H.CIRCLE_TOL, guard=4, offsets=None):
    """adf_surface_triangles on tables of ``capacity`` rows followed by ``guard`` rows of a sentinel: (status, tri_offset,
    tri, index) with the guard rows included."""
    sb = H.batch_of(cases, DEV)
    B, N = len(cases), int(sb.pos.shape[0])
    pos, tags = sb.pos.float().contiguous(), sb.tags.to(torch.int32).contiguous()
    off = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    off[1:] = torch.cumsum(sb.natoms.reshape(-1), 0).to(torch.int32)
    if offsets is not None:
        off = torch.tensor(offsets, dtype=torch.int32, device=DEV)
    cell = sb.cell.float().reshape(B, 9).contiguous()
    tri = torch.full((capacity + guard, 3, 3), -77.0, dtype=torch.float32, device=DEV)
    index = torch.full((capacity + guard, 3), -77, dtype=torch.int32, device=DEV)
    tri_off = torch.full((B + 1 + guard,), -77, dtype=torch.int32, device=DEV)
    status = L.load().adf_surface_triangles(pos.data_ptr(), tags.data_ptr(), off.data_ptr(), cell.data_ptr(), N, B,
                                           C.c_double(circle_tol), capacity, tri_off.data_ptr(), tri.data_ptr(), index.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, tri_off.cpu(), tri.cpu(), index.cpu()


def no_top():
    c = dict(H.generic3()[1])
    c["tags"] = np.zeros_like(c["tags"])
    return c


def collinear():
    """Both tiling vectors along x and the tag-1 atoms on that line: every tiled point is collinear."""
    pos = np.array([[0.3, 0.0, 9.0], [0.4, 0.0, 12.0], [1.6, 0.0, 12.0]], np.float32)
    return dict(pos=pos, Z=np.full(3, 29, np.int64), tags=np.array([0, 1, 1]),
                cell=np.array([[3.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 0.0, 20.0]], np.float32))


def one_in_plane_vector():
    """Only the first row of the cell has an in-plane component: there is no second tiling vector."""
    return dict(collinear(), cell=np.array([[3.0, 0.0, 0.0], [0.0, 0.0, 5.0], [0.0, 0.0, 20.0]], np.float32))


def test_errors_leave_the_tables_alone():
    good = list(H.generic3())
    T = sum(generic_run().counts)
    status, off, tri, index = raw_call(good, T)                      # exactly enough rows: fine, and nothing past them
    assert status == L.ADF_OK and off[:4].tolist() == generic_run().tri_offset.tolist()
    assert (tri[T:] == -77).all() and (index[T:] == -77).all() and (off[4:] == -77).all() and (index[:T] >= 0).all()
    for cases, capacity, tol, what in (([good[0], no_top(), good[2]], 18 * 40, H.CIRCLE_TOL, b"tag 1"),
                                       ([good[0], collinear()], 18 * 40, H.CIRCLE_TOL, b"collinear"),
                                       ([good[0], one_in_plane_vector()], 18 * 40, H.CIRCLE_TOL,
                                        b"surface_triangles: a cell has fewer than two in-plane lattice vectors (or a non-finite one)"),
                                       (good, T - 1, H.CIRCLE_TOL, b"more triangles"),
                                       (good, T, -1e-4, b"circle_tol")):
        status, off, tri, index = raw_call(cases, capacity, tol)
        assert status == L.ADF_EINVAL and what in L.load().adf_last_error(), what
        assert (tri == -77).all() and (index == -77).all(), what     # nothing is written, the guard rows least of all
        assert (off[len(cases) + 1:] == -77).all(), what
    # offsets that descend, or run past the atoms: refused by the first kernel, before an atom is read through them
    n0, n1 = len(good[0]["Z"]), len(good[1]["Z"])
    for offsets in ([0, n0 + n1, n0], [0, n0, n0 + n1 + 1], [-1, n0, n0 + n1]):
        status, off, tri, index = raw_call(good[:2], 18 * 40, offsets=offsets)
        assert status == L.ADF_EINVAL, offsets
        assert b"surface_triangles: atom offsets not ascending or outside [0, N]" in L.load().adf_last_error(), offsets
        assert (tri == -77).all() and (index == -77).all(), offsets
    with pytest.raises(ValueError, match="tag 1"):
        PL.surface_triangles_device(H.batch_of([good[0], no_top()], DEV))
    with pytest.raises(ValueError, match="collinear"):
        PL.heuristic_sites(H.batch_of([collinear()], DEV), triangles="device", symmetry=None)


# 8
def test_a_slab_of_more_points_than_a_wave_has_lanes():
    """fcc(111) 7x7x4: 441 tiled points, seven rounds of a wave.  A perfect p x p triangular lattice keeps 2 p^2 + 4 p
    triangles (helpers_surface_triangles.hex_count: two per central point and a ring of 4 p): 2 * 49 + 28 = 126."""
    c = H.lattice("111_7x7x4")
    st = PL.surface_triangles_device(H.batch_of([c], DEV))
    pts, n_top = H.tiled_points(c["pos"], c["tags"], c["cell"])
    idx, tri = slab_rows(st, 0)
    assert n_top == 49 and len(idx) == H.hex_count(7) == 2 * 49 + 28
    H.check_table(pts[:, :2], n_top, idx)
    assert torch.equal(tri.view(torch.int32), torch.from_numpy(pts[idx].astype(np.float32)).view(torch.int32))


def test_a_slab_whose_points_do_not_fit_the_staging_buffer():
    """One fcc(111) layer of 22 x 22 atoms, all of tag 1: 4356 tiled points, more than are staged in LDS (4000): the walk
    reads them from global memory.  The same count rule and invariants."""
    pos, Z, cell = HS.fcc("111", 22, 22, 1)
    c = dict(pos=pos, Z=Z, cell=cell, tags=np.ones(len(Z), np.int64))
    st = PL.surface_triangles_device(H.batch_of([c], DEV))
    pts, n_top = H.tiled_points(c["pos"], c["tags"], c["cell"])
    idx, _ = slab_rows(st, 0)
    assert n_top == 484 and len(pts) > 4000 and len(idx) == H.hex_count(22)
    H.check_table(pts[:, :2], n_top, idx)
