"""GPU tests of the heuristic site finder (csrc/sites.hip; placement.heuristic_sites, reduce_sites,
place_adsorbates_heuristic) against the float64 oracle of tests/helpers_heuristic_sites.py and the
crystallographic known answers.  The oracle's decision margins are asserted first (no pair distance in (tol / 10, 10 tol), no
corner cosine in (1e-6, 1e-4)); then the kept candidates, ``rep``, ``first``, ``valid``, ``kind`` and ``multiplicity`` must be
the oracle's exactly and the positions agree to a reduce-distance of 1e-5 A."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import placement as PL
from adsorbdiff_amd import slab_symmetry as SY
from tests import helpers_heuristic_sites as H
from tests import helpers_placement as HP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADII, MASSES = HP.synthetic_radii(), HP.synthetic_masses()
TABLE_NAMES = list(H.TABLE)


def find(names, symmetry="auto", **kw):
    return PL.heuristic_sites(H.slab_batch(names, DEV), H.triangles(names), symmetry=symmetry, **kw)


def per_slab(st, b):
    """The tables of slab b with slab-local candidate indices, and its sites."""
    off = st.seg_offset.cpu().numpy().astype(np.int64)
    c0, c1 = off[3 * b], off[3 * b + 3]
    local = lambda t: np.where(t >= 0, t - c0, -1)
    m = (st.slab == b).cpu().numpy()
    return dict(candidates=st.candidates[c0:c1].cpu().numpy(), valid=st.valid[c0:c1].cpu().numpy(),
                rep=local(st.rep[c0:c1].cpu().numpy().astype(np.int64)), first=local(st.first[c0:c1].cpu().numpy().astype(np.int64)),
                segments=[(int(off[3 * b + k] - c0), int(off[3 * b + k + 1] - c0)) for k in range(3)],
                kept=st.candidate.cpu().numpy()[m] - c0, kind=st.kind.cpu().numpy()[m],
                multiplicity=st.multiplicity.cpu().numpy()[m], pos=st.pos.cpu().numpy()[m])


def check(st, b, want, cell):
    got = per_slab(st, b)
    assert got["segments"] == want["segments"]
    assert (got["valid"] == want["valid"]).all()
    err = H.position_error(got["candidates"], want["candidates"], cell)
    assert err <= H.POS_ATOL, err
    assert (got["first"] == want["first"]).all() and (got["rep"] == want["rep"]).all()
    assert got["kept"].tolist() == want["kept"].tolist()
    assert got["kind"].tolist() == want["kind"][want["kept"]].tolist()
    assert got["multiplicity"].tolist() == want["multiplicity"][want["kept"]].tolist()
    assert (got["pos"] == got["candidates"][got["kept"]]).all()
    assert st.counts[b] == len(want["kept"])
    return err


def bits(st):
    return [t.cpu() for t in (st.pos.view(torch.int32), st.slab, st.kind, st.multiplicity, st.candidate, st.candidates.view(torch.int32),
                              st.valid, st.rep, st.first, st.seg_offset)] + [st.counts, st.slab_natoms]


def same(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(bits(a), bits(b)))


@functools.lru_cache(maxsize=None)
def table_run():
    return find(TABLE_NAMES)


def test_known_answers_in_one_ragged_batch():
    st = table_run()
    worst = 0.0
    for b, name in enumerate(TABLE_NAMES):
        want = H.oracle(name)                                        # margins asserted
        worst = max(worst, check(st, b, want, H.case(name)["cell"]))
        kinds = st.kind[st.slab == b].cpu().numpy()
        assert tuple(int((kinds == k).sum()) for k in range(3)) == H.TABLE[name][1], name
    print("largest position error", worst)
    assert st.slab_natoms == [len(H.case(n)["Z"]) for n in TABLE_NAMES]
    assert st.pos.dtype == torch.float32 and st.kind.dtype == torch.int32 and st.slab.dtype == torch.int64
    m = st.multiplicity[st.slab == TABLE_NAMES.index("111_3x3x4")].tolist()
    assert m == [9, 27, 9, 9]
    # fcc(100): right triangles, the hollow segment holds invalid slots only
    got = per_slab(st, TABLE_NAMES.index("100_2x2x3"))
    s0, s1 = got["segments"][2]
    assert s1 > s0 and not got["valid"][s0:s1].any() and (got["rep"][s0:s1] == -1).all()


def test_identity_pass_alone_and_supplied_symmetry():
    names = [n for n in TABLE_NAMES if H.TABLE[n][2] is not None]
    sb, tri = H.slab_batch(names, DEV), H.triangles(names)
    alone = PL.heuristic_sites(sb, tri, symmetry=None)
    for b, name in enumerate(names):
        check(alone, b, H.oracle(name, symmetric=False), H.case(name)["cell"])
        kinds = alone.kind[alone.slab == b].cpu().numpy()
        assert tuple(int((kinds == k).sum()) for k in range(3)) == H.TABLE[name][2]
    assert bool((alone.multiplicity == 1).all()) and torch.equal(alone.rep, alone.first)
    ident = PL.heuristic_sites(sb, tri, symmetry=SY.SlabSymmetry.identity(sb.natoms, DEV))
    assert same(alone, ident)
    sym = SY.find_symmetry(sb)
    assert same(PL.heuristic_sites(sb, tri, symmetry=sym), PL.heuristic_sites(sb, tri, symmetry="auto"))
    assert not same(PL.heuristic_sites(sb, tri, symmetry=sym), alone)


def test_variants_against_the_oracle():
    names = list(H.VARIANTS)
    st = find(names)
    for b, name in enumerate(names):
        check(st, b, H.oracle(name), H.case(name)["cell"])
    b = names.index("rattled")
    assert st.counts[b] == 9 + 27 + 18 and bool((st.multiplicity[st.slab == b] == 1).all())


def test_more_candidates_and_operations_than_a_block_or_a_tile():
    """fcc(111) 7x7x4: 486 raw bridge candidates (two rounds of the 256 threads) and 294 operations (three tiles of 128)."""
    name = "111_7x7x4"
    sb = H.slab_batch([name], DEV)
    sym = SY.find_symmetry(sb)
    assert sym.counts == [294]
    st = PL.heuristic_sites(sb, H.triangles([name]), symmetry=sym)
    want = H.sites(H.case(name), ops=H.device_ops(sym, 0))
    H.assert_margins(want)
    assert want["segments"][1][1] - want["segments"][1][0] == 486
    check(st, 0, want, H.case(name)["cell"])
    assert st.kind.tolist() == [0, 1, 2, 2] and st.multiplicity.tolist() == [49, 147, 49, 49]


def test_more_kept_sites_than_any_staging():
    """19 x 18 surface cells, the identity pass only: 1026 kept bridge sites out of 2520 raw ones."""
    name = H.HS.LARGE_SLAB[0]
    st = find([name], symmetry=None)
    want = H.sites(H.case(name), ops=None)
    H.assert_margins(want)
    assert H.site_counts(want) == (342, 1026, 684)
    check(st, 0, want, H.case(name)["cell"])


def test_a_slab_gets_the_same_bits_anywhere():
    names = ["111_2x2x3", "100_2x2x3", "111_3x3x4", "110_1x1x2"]
    whole = find(names)
    rev = find(names[::-1])
    halves = [find(names[:2]), find(names[2:])]
    for b, name in enumerate(names):
        ref = per_slab(find([name]), 0)
        for st, k in ((whole, b), (rev, len(names) - 1 - b), (halves[b // 2], b % 2)):
            got = per_slab(st, k)
            for key in ref:
                a, c = np.asarray(ref[key]), np.asarray(got[key])
                assert a.shape == c.shape and (a.view(np.int32) == c.view(np.int32) if a.dtype == np.float32 else a == c).all(), (name, key)
    only = find(names, positions=("bridge",))
    assert bool((only.kind == 1).all()) and only.counts == [int(((whole.slab == b) & (whole.kind == 1)).sum()) for b in range(4)]
    assert torch.equal(only.pos, whole.pos[whole.kind == 1]) and torch.equal(only.rep, whole.rep)


# ------------------------------------------------------------------------------------------------ reduce_sites
def orbit_case(name, base, seed):
    """Images of the base points (fractional in-plane coordinates, height) under randomly chosen operations of the slab plus
    lattice translates, the base points first."""
    c = H.case(name)
    rng = np.random.default_rng(seed)
    cell = c["cell"].astype(np.float64)
    top = float(c["pos"][:, 2].max())
    pts = [np.array([f[0], f[1], 0.0]) @ cell + [0, 0, top + f[2]] for f in base]
    out = list(pts)
    for k in range(6 * len(base)):
        o = c["ops"][int(rng.integers(len(c["ops"])))]
        i, j = rng.integers(-2, 3, 2)
        out.append(o["R"] @ pts[k % len(base)] + o["t"] + i * cell[0] + j * cell[1])
    return np.asarray(out, np.float32)


# general positions whose images under the operations of both slabs stay 0.58 A apart (searched on the host); the heights
# keep the three orbits 0.8 A apart whatever the operation
BASES = [(0.55698, 0.66233, 1.0), (0.44744, 0.33211, 1.8), (0.05244, 0.16511, 2.6)]


def test_reduce_sites_collapses_orbits():
    names = ["111_2x2x3", "100_2x2x3"]
    pts = [orbit_case(n, BASES, 5 + k) for k, n in enumerate(names)]
    sb = H.slab_batch(names, DEV)
    placer = PL.AdsorbatePlacer(RADII, MASSES, device=DEV)
    red = placer.reduce_sites(sb, [torch.from_numpy(p) for p in pts])
    start = 0
    for b, name in enumerate(names):
        c = H.case(name)
        n = len(pts[b])
        want = H.reduce(pts[b], np.ones(n, bool), [(0, n)], c["cell"], c["ops"])
        H.assert_margins(want)
        assert want["kept"].tolist() == [0, 1, 2] and (want["rep"] == np.arange(n) % 3).all()
        assert red.sites.counts[b] == 3
        assert (red.rep[start:start + n].cpu().numpy() - 3 * b == want["rep"]).all()
        assert red.multiplicity[3 * b:3 * b + 3].tolist() == want["multiplicity"][:3].tolist()
        assert (red.sites.pos[3 * b:3 * b + 3].cpu().numpy() == pts[b][:3]).all()
        start += n
    assert red.sites.slab.tolist() == [0, 0, 0, 1, 1, 1]
    # without the operations only the lattice translates of one image merge
    plain = placer.reduce_sites(sb, [torch.from_numpy(p) for p in pts], symmetry=None)
    for b, name in enumerate(names):
        n = len(pts[b])
        want = H.reduce(pts[b], np.ones(n, bool), [(0, n)], H.case(name)["cell"], None)
        H.assert_margins(want)
        assert plain.sites.counts[b] == len(want["kept"]) > 3
    # the random sites of sites() go through as well: fewer or as many come back, each its own representative or a merged one
    tri = H.triangles(names)
    rnd = placer.sites(sb, 20, triangles=tri)
    out = placer.reduce_sites(sb, rnd)
    assert all(a <= b for a, b in zip(out.sites.counts, rnd.counts)) and int(out.multiplicity.sum()) <= sum(rnd.counts)
    assert int(out.rep.max()) == sum(out.sites.counts) - 1


# ------------------------------------------------------------------------------------------------ placements
def test_place_adsorbates_heuristic():
    names = ["111_3x3x4", "100_2x2x3"]
    sb, tri = H.slab_batch(names, DEV), H.triangles(names)
    ads = (np.array([6, 8]), np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.15]]))
    n_aug = 2
    placer = PL.AdsorbatePlacer(RADII, MASSES, device=DEV, seed=3)
    out = PL.place_adsorbates_heuristic(sb, ads, [0], num_augmentations_per_site=n_aug, triangles=tri, placer=placer)
    st = placer.heuristic_sites(sb, tri)
    S = sum(st.counts)
    assert st.counts == [4, 3] and int(out.natoms.numel()) == S * n_aug
    assert out.site_kind.tolist() == [k for k in st.kind.tolist() for _ in range(n_aug)]
    assert out.site_multiplicity.tolist() == [m for m in st.multiplicity.tolist() for _ in range(n_aug)]
    assert out.site_group.tolist() == [s for s in st.slab.tolist() for _ in range(n_aug)]
    # the binding atom over its site, in the plane (the normal is z here)
    pos = out.pos.cpu().numpy().astype(np.float64)
    off = np.concatenate([[0], np.cumsum(out.natoms.cpu().numpy())])
    n_slab = np.asarray(st.slab_natoms)[out.site_group.cpu().numpy()]
    bind = pos[off[:-1] + n_slab + out.binding_idx.cpu().numpy()]
    site = out.site.cpu().numpy().astype(np.float64)
    ulp = float(np.spacing(np.float32(np.abs(pos).max())))
    assert np.abs(bind[:, :2] - site[:, :2]).max() <= ulp
    assert (bind[:, 2] > site[:, 2]).all()
    d = PL.interstitial_distances(out, RADII, MASSES)
    assert tuple(d.shape) == (S * n_aug,) and bool(torch.isfinite(d).all())
    again = placer.place(sb, ads, st, n_aug, 0.1, "random_site_heuristic_placement", [0])
    for key in ("pos", "atomic_numbers", "tags", "natoms", "batch", "site", "scaled_normal", "xyz_angles", "site_kind",
                "site_multiplicity", "site_index"):
        a, b = getattr(out, key), getattr(again, key)
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), key
    with pytest.raises(ValueError, match="place_adsorbates_heuristic"):
        placer.place(sb, ads, st, mode="heuristic")


class _Atoms:
    def __init__(self, numbers, positions, cell=None, tags=None):
        self.numbers, self.positions, self.cell, self.tags = numbers, positions, cell, tags
        self.pbc = (True, True, False)


class _Holder:
    def __init__(self, atoms, binding_indices=None):
        self.atoms, self.binding_indices = atoms, binding_indices


def test_adsorbate_slab_config_heuristic():
    c = H.case("111_2x2x3")
    slab = _Holder(_Atoms(c["Z"], c["pos"], c["cell"], c["tags"]))
    ads = _Holder(_Atoms(np.array([6, 8]), np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.15]]), tags=np.array([2, 2])), [0])
    cfg = PL.AdsorbateSlabConfig.heuristic(slab, ads, triangles=c["tri"], radii=RADII, masses=MASSES, device=DEV)
    assert cfg.mode == "heuristic" and cfg.sites.shape == (4, 3) and len(cfg.metadata_list) == 4
    assert cfg.surface_sites.kind.tolist() == [0, 1, 2, 2] and cfg.batch.site_kind.tolist() == [0, 1, 2, 2]
    with pytest.raises(ValueError):
        PL.AdsorbateSlabConfig(slab, ads, mode="heuristic", radii=RADII, masses=MASSES, device=DEV)


# ------------------------------------------------------------------------------------------------ malformed input
def _reduce_raw(seg, C_rows, slab=None, op_off=None, K=0):
    lib = L.load()
    dev = torch.device(DEV)
    G = len(seg) - 1
    cand = torch.zeros(max(C_rows, 1), 3, device=dev)
    seg_t = torch.tensor(seg, dtype=torch.int32, device=dev)
    slab_t = None if slab is None else torch.tensor(slab, dtype=torch.int32, device=dev)
    cell = torch.eye(3, device=dev).reshape(1, 9).repeat(2, 1).contiguous() * 5
    out = [torch.full((max(C_rows, 1),), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    counts = torch.full((G, 2), -7, dtype=torch.int32, device=dev)
    op_t = None if op_off is None else torch.tensor(op_off, dtype=torch.int32, device=dev)
    rot = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(max(K, 1), 1).contiguous()
    trans = torch.zeros(max(K, 1), 3, dtype=torch.float64, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    status = lib.adf_reduce_sites(cand.data_ptr(), None, seg_t.data_ptr(), ptr(slab_t), cell.data_ptr(), C_rows, G, 2, ptr(op_t),
                                  rot.data_ptr() if op_t is not None else None, trans.data_ptr() if op_t is not None else None, K,
                                  C.c_double(0.05), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), counts.data_ptr(), None)
    torch.cuda.synchronize()
    return status, [o.cpu() for o in out], counts.cpu()


def test_malformed_offsets_are_refused_not_read_past():
    lib = L.load()
    status, out, counts = _reduce_raw([0, 3, 5], 5)
    assert status == L.ADF_OK and counts.tolist() == [[1, 1], [1, 1]] and out[1].tolist() == [0, 0, 0, 3, 3]
    for seg, kw in (([0, 5, 3], {}), ([0, 3, 9], {}), ([-1, 3, 5], {}), ([0, 3, 5], dict(slab=[0, 2])),
                    ([0, 3, 5], dict(op_off=[0, 1, 3], K=2)), ([0, 3, 5], dict(op_off=[0, 0, 1], K=1))):
        status, out, counts = _reduce_raw(seg, 5, **kw)
        assert status == L.ADF_EINVAL, (seg, kw)
        assert b"malformed offsets" in lib.adf_last_error()
        bad = [g for g in range(2) if counts[g].tolist() == [0, 0]]
        assert len(bad) == 1, (seg, kw)
        written = np.zeros(5, bool)                                  # the rows of the segment that was accepted
        written[seg[1 - bad[0]]:seg[2 - bad[0]]] = True
        assert all(bool((o[~written] == -7).all()) and bool((o[written] != -7).all()) for o in out), (seg, kw)
    with pytest.raises(ValueError, match="malformed offsets"):
        L.check(L.ADF_EINVAL)
    # the candidate stage: atoms past the array, tables too small, a null pointer (refused before anything is launched)
    names = ["111_1x1x3"]
    sb = H.slab_batch(names, DEV)
    tri = torch.from_numpy(H.triangles(names)[0].astype(np.float32)).to(DEV).contiguous()
    T, N = int(tri.shape[0]), int(sb.pos.shape[0])
    tags = sb.tags.to(torch.int32).contiguous()
    cell = sb.cell.reshape(1, 9).contiguous()
    tri_off = torch.tensor([0, T], dtype=torch.int32, device=DEV)

    def candidates(atom_off, rows, pos_ptr="pos", cell=cell):
        a = torch.tensor(atom_off, dtype=torch.int32, device=DEV)
        seg = torch.full((4,), -7, dtype=torch.int32, device=DEV)
        cand = torch.full((N + 4 * T, 3), -7.0, device=DEV)
        valid = torch.full((N + 4 * T,), -7, dtype=torch.int32, device=DEV)
        s = lib.adf_surface_site_candidates(sb.pos.data_ptr() if pos_ptr else None, tags.data_ptr(), a.data_ptr(), cell.data_ptr(),
                                            tri.data_ptr(), tri_off.data_ptr(), N, T, 1, rows, seg.data_ptr(), cand.data_ptr(),
                                            valid.data_ptr(), None)
        torch.cuda.synchronize()
        return s, seg.cpu().tolist(), cand.cpu(), valid.cpu()

    s, seg, cand, valid = candidates([0, N], N + 4 * T)
    assert s == L.ADF_OK and seg == [0, 1, 1 + 3 * T, 1 + 4 * T] and bool((valid[:seg[3]] == 1).all()) and bool((valid[seg[3]:] == -7).all())
    for atom_off, rows in (([0, N + 1], N + 4 * T), ([2, 1], N + 4 * T), ([0, N], 4 * T)):
        s, seg, cand, valid = candidates(atom_off, rows)
        assert s == L.ADF_EINVAL and b"malformed offsets" in lib.adf_last_error()
        assert bool((valid == -7).all()) and bool((cand == -7).all())                # no candidate was written
    # a cell whose first two rows are parallel: the frame is refused before a candidate is computed in it
    flat = cell.clone()
    flat[0, 3:6] = 2.0 * flat[0, 0:3]
    s, seg, cand, valid = candidates([0, N], N + 4 * T, cell=flat)
    assert s == L.ADF_EINVAL and b"surface_site_candidates: the first two rows of a cell span no finite area" in lib.adf_last_error()
    assert bool((valid == -7).all()) and bool((cand == -7).all())
    s, seg, cand, valid = candidates([0, N], N + 4 * T, pos_ptr=None)
    assert s == L.ADF_EINVAL and b"null argument" in lib.adf_last_error()
    assert seg == [-7] * 4 and bool((valid == -7).all())
