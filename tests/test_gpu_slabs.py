"""GPU tests of slab cutting (csrc/slabcut.hip; adsorbdiff_amd/slabs.py) against the independent float64
oracle of tests/helpers_slabs.py - which asserts its decision margins before anything is compared - and against the
invariants (a)-(g) of a correct slab.  The whole case table (35 (bulk, h) pairs, at most 20 atoms per unit slab) is ONE
batch, cut once per module.  Parity with pymatgen unpinned."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import placement as PL
from adsorbdiff_amd import slabs as SL
from adsorbdiff_amd.data import Batch
from tests import helpers_placement as HP
from tests import helpers_slabs as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POS_ATOL = 1e-9                 # A: the bound the surface-tag tests hold float64 geometry to
CRYSTALS = H.crystals()
NAMES, PAIRS = H.all_pairs()
MASSES = HP.synthetic_masses(n=119)


def bulk_batch(names):
    b = Batch()
    b.pos = torch.cat([torch.from_numpy(CRYSTALS[n]["pos"]) for n in names]).to(DEV)
    b.cell = torch.stack([torch.from_numpy(CRYSTALS[n]["cell"]) for n in names]).to(DEV)
    b.atomic_numbers = torch.cat([torch.from_numpy(CRYSTALS[n]["Z"]) for n in names]).to(DEV)
    b.natoms = torch.tensor([len(CRYSTALS[n]["Z"]) for n in names], device=DEV)
    return b


def millers_of(names):
    return [[h for n, h in PAIRS if n == name] for name in names]


@functools.lru_cache(maxsize=None)
def device_run(order=tuple(NAMES)):
    return SL.compute_slabs(bulk_batch(order), specific_millers=millers_of(order))


@functools.lru_cache(maxsize=None)
def oracle(name, h):
    return H.cut_slabs(CRYSTALS[name], h)


def per_pair(out, order=tuple(NAMES)):
    """{(name, h): list of slabs as the oracle's dicts} from a device result."""
    b = out.batch
    off = np.concatenate([[0], np.cumsum(b.natoms.cpu().numpy())])
    pos, Z, cell = out.pos64.cpu().numpy(), b.atomic_numbers.cpu().numpy(), out.cell64.cpu().numpy()
    mil, shift, top, bi = b.millers.cpu().numpy(), b.shift.cpu().numpy(), b.top.cpu().numpy(), b.bulk_index.cpu().numpy()
    slabs = [{"pos": pos[off[s]:off[s + 1]], "Z": Z[off[s]:off[s + 1]], "cell": cell[s], "millers": tuple(int(x) for x in mil[s]),
              "shift": float(shift[s]), "top": bool(top[s]), "bulk": int(bi[s])} for s in range(len(shift))]
    got, at = {}, 0
    for bidx, name in enumerate(order):
        for h in [h for n, h in PAIRS if n == name]:
            n_expected = len(oracle(name, h)[0])
            got[(name, h)] = slabs[at:at + n_expected]
            assert all(s["bulk"] == bidx for s in got[(name, h)])
            at += n_expected
    assert at == len(slabs)
    return got


def test_slabs_agree_with_the_oracle():
    out = device_run()
    got = per_pair(out)
    worst = 0.0
    for (name, h), mine in got.items():
        want = oracle(name, h)[0]
        assert len(mine) == len(want), (name, h)
        for a, b in zip(mine, want):
            assert a["millers"] == b["millers"] and a["top"] == b["top"] and a["Z"].tolist() == b["Z"].tolist(), (name, h)
            err = max(np.abs(a["pos"] - b["pos"]).max(), abs(a["shift"] - b["shift"]), np.abs(a["cell"] - b["cell"]).max())
            worst = max(worst, err)
            assert err <= POS_ATOL, (name, h, err)
    print(f"slabs: {len(got)} pairs, {int(out.batch.natoms.numel())} slabs, worst |device - oracle| = {worst:.3e} A")
    b = out.batch
    assert torch.equal(b.pos, out.pos64.float()) and torch.equal(b.cell, out.cell64.float())
    assert b.pos.dtype == torch.float32 and b.shift.dtype == torch.float64 and b.top.dtype == torch.bool
    assert b.pbc.tolist() == [[1, 1, 0]] * int(b.natoms.numel()) and int(b.natoms.sum()) == int(b.pos.shape[0])
    assert b.batch.tolist() == np.repeat(np.arange(len(b.natoms)), b.natoms.cpu().numpy()).tolist()


def test_invariants_hold_on_device_output():
    got = per_pair(device_run())
    for (name, h), mine in got.items():
        facts = oracle(name, h)[1]                                      # d, n_slab, the frame and the translation count only
        tops = {s["shift"]: s for s in mine if s["top"]}
        assert [s["top"] for s in mine] == sorted((s["top"] for s in mine), reverse=True)
        assert [s["shift"] for s in mine if s["top"]] == sorted(tops) and all(0.0 <= s["shift"] < facts["d"] for s in mine)
        for s in mine:
            H.check_invariants(CRYSTALS[name], s, facts, partner=None if s["top"] else tops[s["shift"]])


@pytest.mark.parametrize("max_miller", [1, 2])
def test_distinct_millers_equal_the_oracle(max_miller):
    millers, off, n_ops = SL.distinct_millers(bulk_batch(NAMES), max_miller)
    millers, off = millers.cpu().numpy(), off.cpu().numpy()
    assert millers.dtype == np.int32 and off[0] == 0 and off[-1] == len(millers)
    for b, name in enumerate(NAMES):
        want, order = H.distinct_millers(CRYSTALS[name], max_miller)
        assert [tuple(r) for r in millers[off[b]:off[b + 1]].tolist()] == want, name
        assert int(n_ops[b]) == order == H.MILLER_TABLE[name][0], name
        assert len(want) == H.MILLER_TABLE[name][max_miller]


def bits(out):
    b = out.batch
    return [out.pos64.view(torch.int64), out.cell64.view(torch.int64), b.pos.view(torch.int32), b.cell.view(torch.int32),
            b.atomic_numbers, b.natoms, b.millers, b.shift.view(torch.int64), b.top]


def test_bit_equality_alone_again_and_reversed():
    full = device_run()
    again = SL.compute_slabs(bulk_batch(NAMES), specific_millers=millers_of(NAMES))
    assert all(torch.equal(a, b) for a, b in zip(bits(full), bits(again))) and torch.equal(full.batch.bulk_index, again.batch.bulk_index)
    rev = device_run(tuple(NAMES[::-1]))
    fb, rb = full.batch.bulk_index.cpu().numpy(), rev.batch.bulk_index.cpu().numpy()

    def rows(out, slabs):
        sizes = out.batch.natoms.cpu().numpy()
        off = np.concatenate([[0], np.cumsum(sizes)])
        atoms = torch.tensor(np.concatenate([np.arange(off[s], off[s + 1]) for s in slabs]), device=DEV)
        sl = torch.tensor(slabs, device=DEV)
        return [t[atoms if i in (0, 2, 4) else sl] for i, t in enumerate(bits(out))]      # per atom: pos64, pos, species

    for b, name in enumerate(NAMES):
        mine = rows(full, np.nonzero(fb == b)[0])
        other = rows(rev, np.nonzero(rb == len(NAMES) - 1 - b)[0])
        assert all(torch.equal(x, y) for x, y in zip(mine, other)), name
        alone = SL.compute_slabs(bulk_batch([name]), specific_millers=millers_of([name]))
        assert all(torch.equal(x, y) for x, y in zip(mine, bits(alone))), name
    # from the distinct indices: the same slabs as asking for those indices
    auto = SL.compute_slabs(bulk_batch(["cscl"]), max_miller=1)
    asked = SL.compute_slabs(bulk_batch(["cscl"]), specific_millers=[(1, 1, 1), (1, 1, 0), (1, 0, 0)])
    assert all(torch.equal(x, y) for x, y in zip(bits(auto), bits(asked))) and int(auto.batch.natoms.numel()) == 9


# ---- refusals, through the raw entries, with guard rows
GUARD = 7


def _raw(names, pairs, cells=None):
    """Device arguments of adf_slab_cut_count for `pairs` = [(bulk, (h, k, l))]."""
    b = bulk_batch(names)
    g = SL._bulks(b, "test")
    cell = g.cell if cells is None else torch.tensor(np.asarray(cells, np.float64).reshape(len(names), 9), device=DEV)
    pb = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=DEV)
    pm = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=DEV)
    seg = torch.zeros(len(pairs) + 1, dtype=torch.int64, device=DEV)
    seg[1:] = torch.cumsum(g.natoms[pb.long()], 0)
    return g, cell, pb, pm, seg


def _count(g, cell, pb, pm, seg, sizes=(7.0, 20.0, 0.3, 1e-3)):
    lib = L.load()
    P, A = int(pb.numel()), int(seg[-1])
    nbytes = int(lib.adf_slab_cut_scratch(A, P))
    scratch = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    counts = torch.full((3 * P + GUARD,), -77, dtype=torch.int32, device=DEV)
    host = torch.full((3 * P + GUARD,), -77, dtype=torch.int32)
    with torch.cuda.device(DEV):
        st = lib.adf_slab_cut_count(g.pos.data_ptr(), cell.data_ptr(), g.Z.data_ptr(), g.atom_offset.data_ptr(), g.N, g.B,
                                    pb.data_ptr(), pm.data_ptr(), seg.data_ptr(), P, A, *(C.c_double(v) for v in sizes),
                                    scratch.data_ptr(), counts.data_ptr(), host.data_ptr(), SL.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert (scratch[nbytes:] == 0x5A).all() and (counts[3 * P:] == -77).all() and (host[3 * P:] == -77).all()
    return st, lib.adf_last_error().decode(), scratch, counts, host, nbytes


def test_refusals_per_bulk_name_the_bulk():
    names = ["fcc_cu", "cscl", "bcc_fe"]
    good = [(0, (1, 1, 1)), (1, (1, 0, 0)), (2, (1, 1, 0))]
    st, _, _, counts, host, _ = _count(*_raw(names, good))
    assert st == L.ADF_OK and host[:9].view(3, 3)[:, 2].tolist() == [0, 0, 0] and torch.equal(counts.cpu(), host)
    clean = host[:9].clone()
    # h = (0,0,0) for the second bulk
    st, msg, _, _, host, _ = _count(*_raw(names, [good[0], (1, (0, 0, 0)), good[2]]))
    assert st == L.ADF_EINVAL and "bulk 1" in msg and "(0,0,0)" in msg
    assert host[3:6].tolist() == [0, 0, 1] and host[:3].tolist() == clean[:3].tolist() and host[6:9].tolist() == clean[6:9].tolist()
    with pytest.raises(ValueError, match="bulk 1"):
        SL.compute_slabs(bulk_batch(names), specific_millers=[[(1, 1, 1)], [(0, 0, 0)], [(1, 1, 0)]])
    # a singular and a left-handed cell for the third bulk; its atoms are not read (NaN positions change nothing), the
    # others' counts are those of the clean run
    cells = np.stack([CRYSTALS[n]["cell"] for n in names])
    for bad_cell in (np.array([[2.87, 0, 0], [0, 2.87, 0], [2.87, 2.87, 0]]), cells[2][[1, 0, 2]],
                     np.array([[np.inf, 0, 0], [0, 2.87, 0], [0, 0, 2.87]])):
        c = cells.copy()
        c[2] = bad_cell
        g, cell, pb, pm, seg = _raw(names, good, c)
        pos = g.pos.clone()
        pos[-2:] = float("nan")
        st, msg, _, _, host, _ = _count(g._replace(pos=pos), cell, pb, pm, seg)
        assert st == L.ADF_EINVAL and "bulk 2" in msg and "cell" in msg
        assert host[6:9].tolist() == [0, 0, 2] and host[:6].tolist() == clean[:6].tolist()
    b = bulk_batch(names)
    b.cell[2] = b.cell[2][[1, 0, 2]]
    with pytest.raises(ValueError, match="bulk 2"):
        SL.distinct_millers(b)


def test_refusals_of_arguments():
    names = ["fcc_cu"]
    args = _raw(names, [(0, (1, 1, 1))])
    for k in range(4):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            sizes = [7.0, 20.0, 0.3, 1e-3]
            sizes[k] = v
            st, msg, scratch, counts, host, nbytes = _count(*args, sizes=tuple(sizes))
            assert st == L.ADF_EINVAL and "finite and positive" in msg
            assert (scratch == 0x5A).all() and (counts == -77).all() and (host == -77).all()     # nothing launched
    lib, g = L.load(), args[0]
    for mm in (0, 5, -1):
        nbytes = int(lib.adf_distinct_millers_scratch(g.N, g.B))
        scratch = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
        found = torch.full((3 + GUARD,), -77, dtype=torch.int32, device=DEV)
        host = torch.full((3 + GUARD,), -77, dtype=torch.int32)
        with torch.cuda.device(DEV):
            st = lib.adf_distinct_millers_count(g.pos.data_ptr(), g.cell.data_ptr(), g.Z.data_ptr(), g.atom_offset.data_ptr(), g.N,
                                                g.B, mm, C.c_double(1e-3), scratch.data_ptr(), found.data_ptr(), host.data_ptr(),
                                                SL.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        assert st == L.ADF_EINVAL and "max_miller" in lib.adf_last_error().decode()
        assert (scratch == 0x5A).all() and (found == -77).all() and (host == -77).all()


def test_capacity_refusal_writes_nothing():
    names = ["fcc_cu", "cscl"]
    g, cell, pb, pm, seg = _raw(names, [(0, (1, 1, 1)), (1, (1, 0, 0))])
    st, _, scratch, counts, host, nbytes = _count(g, cell, pb, pm, seg)
    assert st == L.ADF_OK
    hv = host[:6].view(2, 3).long()
    S, M = int(hv[:, 0].sum()), int((hv[:, 0] * hv[:, 1]).sum())
    assert (S, M) == (5, 4 + 4 * 6)
    slab_off = SL.offsets(counts[:6].view(2, 3)[:, 0])
    out_off = torch.zeros(3, dtype=torch.int64, device=DEV)
    out_off[1:] = torch.cumsum(hv[:, 0] * hv[:, 1], 0).to(DEV)
    lib = L.load()

    def fill(slab_cap, atom_cap, slab_off=slab_off, out_off=out_off):
        bufs = dict(pos64=torch.full((M + GUARD, 3), -7.0, dtype=torch.float64, device=DEV),
                    pos32=torch.full((M + GUARD, 3), -7.0, dtype=torch.float32, device=DEV),
                    Z=torch.full((M + GUARD,), -7, dtype=torch.int32, device=DEV),
                    cell=torch.full((S + GUARD, 9), -7.0, dtype=torch.float64, device=DEV),
                    millers=torch.full((S + GUARD, 3), -7, dtype=torch.int32, device=DEV),
                    shift=torch.full((S + GUARD,), -7.0, dtype=torch.float64, device=DEV),
                    top=torch.full((S + GUARD,), -7, dtype=torch.int32, device=DEV),
                    bulk=torch.full((S + GUARD,), -7, dtype=torch.int32, device=DEV),
                    natoms=torch.full((S + GUARD,), -7, dtype=torch.int32, device=DEV))
        with torch.cuda.device(DEV):
            st = lib.adf_slab_cut_fill(scratch.data_ptr(), pb.data_ptr(), seg.data_ptr(), slab_off.data_ptr(), out_off.data_ptr(), 2,
                                       int(seg[-1]), C.c_double(1e-3), slab_cap, atom_cap, *(t.data_ptr() for t in bufs.values()),
                                       SL.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return st, lib.adf_last_error().decode(), bufs

    untouched = lambda bufs: all(bool((t == -7).all()) for t in bufs.values())
    for caps in ((S - 1, M), (S, M - 1), (0, 0)):
        st, msg, bufs = fill(*caps)
        assert st == L.ADF_EOVERFLOW and "bulk" in msg and untouched(bufs), caps
    st, msg, bufs = fill(S, M, out_off=out_off + 1)                    # offsets that are not the count pass's
    assert st == L.ADF_EOVERFLOW and untouched(bufs)
    st, msg, bufs = fill(S, M)
    assert st == L.ADF_OK
    assert all(bool((t[(M if k in ("pos64", "pos32", "Z") else S):] == -7).all()) for k, t in bufs.items())   # the guard rows
    assert bufs["natoms"][:S].tolist() == [4, 6, 6, 6, 6] and bufs["top"][:S].tolist() == [1, 1, 1, 0, 0]
    assert not bool((bufs["pos64"][:M] == -7).any()) and bufs["bulk"][:S].tolist() == [0, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="capacity"):
        L.check(fill(S - 1, M)[0])


# ---- end to end: bulk -> slabs -> tags -> sites -> placement
def test_cut_and_tag_feeds_sites_and_placement():
    tiled = SL.cut_and_tag(bulk_batch(["fcc_cu", "cscl"]), specific_millers=[[(1, 1, 1)], [(1, 0, 0)]], min_ab=8.0, masses=MASSES)
    assert tiled.bulk_index.tolist() == [0, 1, 1, 1, 1] and tiled.top.tolist() == [True, True, True, False, False]
    assert tiled.millers.tolist() == [[1, 1, 1]] + [[1, 0, 0]] * 4
    length = torch.linalg.norm(tiled.cell.double(), dim=2)
    assert bool((length[:, :2] >= 8.0).all())
    off = np.concatenate([[0], np.cumsum(tiled.natoms.cpu().numpy())])
    pos, tags, Z = tiled.pos.cpu().numpy(), tiled.tags.cpu().numpy(), tiled.atomic_numbers.cpu().numpy()
    # fcc Cu (111): a p(4 x 4) tile of the four-layer slab; only the top layer is tagged
    n = int(np.ceil(8.0 / (3.61 / np.sqrt(2.0))))
    z, t = pos[off[0]:off[1], 2], tags[off[0]:off[1]]
    assert len(z) == 4 * n * n and t.sum() == n * n and (z[t == 1] > z[t == 0].max() + 1.0).all()
    assert tiled.fixed.tolist() == (tiled.tags == 0).long().tolist()
    cu = Batch.from_data_list(tiled.to_data_list()[:1])
    st = PL.heuristic_sites(cu)
    assert st.counts == [4] and st.kind.tolist() == [0, 1, 2, 2]
    assert st.multiplicity.tolist() == [n * n, 3 * n * n, n * n, n * n]
    ads = (np.array([6, 8]), np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.15]]))
    placed = PL.place_adsorbates_heuristic(tiled, ads, [0], radii=HP.synthetic_radii(), masses=MASSES)
    assert int(placed.natoms.numel()) == int(placed.site_group.numel()) > 4 and set(placed.site_group.tolist()) == {0, 1, 2, 3, 4}
    # CsCl (100): the two terminations differ in their top species; each flipped partner shows the other one
    top_species = [set(Z[off[s]:off[s + 1]][pos[off[s]:off[s + 1], 2] > pos[off[s]:off[s + 1], 2].max() - 0.5].tolist()) for s in range(1, 5)]
    assert all(len(s) == 1 for s in top_species)
    a, b, c, d = (s.pop() for s in top_species)
    assert {a, b} == {17, 55} and (c, d) == (b, a)
    assert all(bool((tags[off[s]:off[s + 1]] == 1).any()) for s in range(5))


def test_slab_and_bulk_classes():
    c = CRYSTALS["fcc_cu"]
    bulk = SL.Bulk(c["pos"], c["cell"], c["Z"], src_id="cu", device=DEV)
    slabs = SL.Slab.from_bulk_get_all_slabs(bulk, max_miller=1, masses=MASSES)
    batch = SL.compute_slabs(bulk.batch(), max_miller=1).batch
    assert len(slabs) == 3 == int(batch.natoms.numel())
    assert [s.millers for s in slabs] == [tuple(m) for m in batch.millers.tolist()] == [(1, 1, 1), (1, 1, 0), (1, 0, 0)]
    assert [s.shift for s in slabs] == batch.shift.tolist() and [s.top for s in slabs] == batch.top.tolist() == [True] * 3
    for s, n in zip(slabs, batch.natoms.tolist()):
        meta = s.get_metadata_dict()
        assert meta["slab_metadata"] == {"bulk_id": "cu", "millers": s.millers, "shift": s.shift, "top": True}
        assert len(s) % n == 0 and len(s) > n and s.has_surface_tagged() and meta["slab_batch"] is s.batch
    one = SL.Slab.from_bulk_get_specific_millers((1, 1, 0), bulk, masses=MASSES)
    assert len(one) == 1 and one[0].millers == (1, 1, 0) and torch.equal(one[0].batch.pos, slabs[1].batch.pos)
    picks = [SL.Slab.from_bulk_get_random_slab(bulk, max_miller=1, masses=MASSES, generator=torch.Generator().manual_seed(5)).millers
             for _ in range(2)]
    want = slabs[int(torch.randint(3, (1,), generator=torch.Generator().manual_seed(5)))].millers
    assert picks == [want, want]
