"""GPU tests of the surface tags (csrc/voronoi.hip; adsorbdiff_amd/surface_tags.py).  The device's coordination
numbers are held to 1e-9 against what qhull gave for the same points (tests/golden/voronoi_cn.npz: no scipy here) and against
the float64 oracle of tests/helpers_voronoi.py, whose margins (asserted first) leave no decision - a weight against
``weight_tol``, a coordination against the bulk minimum, a height against a threshold, a radius against ``far`` - within reach
of a rounding: ``nn``, the open flags and the tags must be equal.

Measured on an MI355X over all cases: 2.1e-11 at worst against the oracle, below 1.1e-11 against qhull except 4.4e-10 (cn) on
two atoms under the vacancy, which the oracle shows against qhull as well."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import placement as PL
from adsorbdiff_amd import surface_tags as ST
from tests import helpers_heuristic_sites as HH
from tests import helpers_voronoi as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(H.CASES)
BULK_NAMES = list(H.BULKS)


@functools.lru_cache(maxsize=None)
def all_cases_run():
    """voronoi_coordination on every case in one batch, each with its selection."""
    H.assert_margins()
    select = torch.from_numpy(np.concatenate([H.select_mask(n) for n in NAMES]))
    return ST.voronoi_coordination(H.batch_of([H.case(n) for n in NAMES], DEV), select=select)


def rows_of(vc, names, name):
    start = sum(len(H.case(n)["Z"]) for n in names[:names.index(name)])
    rows = slice(start, start + len(H.case(name)["Z"]))
    return tuple(t[rows].cpu() for t in vc)


def bits(*tensors):
    return [t.view(torch.int64) if t.dtype == torch.float64 else t for t in tensors]


@functools.lru_cache(maxsize=None)
def fcc_row():
    return torch.from_numpy(H.fcc_bulk_row())


def masses():
    return H.synthetic_masses()


# 1
@pytest.mark.parametrize("name", NAMES)
def test_coordination_equals_qhull_and_the_oracle(name):
    cn, om, nn, op = rows_of(all_cases_run(), NAMES, name)
    sel = H.select_mask(name)
    assert cn.dtype == torch.float64 and om.dtype == torch.float64 and nn.dtype == torch.int32 and op.dtype == torch.bool
    # rows outside the selection are as they were handed in
    assert torch.isnan(cn[~sel]).all() and torch.isnan(om[~sel]).all() and (nn[~sel] == 0).all() and not op[~sel].any()
    cn, om, nn, op = cn.numpy()[sel], om.numpy()[sel], nn.numpy()[sel], op.numpy()[sel]
    fx = H.load_fixture()[name]
    for what, (rcn, rom, rnn, rop) in (("qhull", (fx["cn"], fx["omega_max"], fx["nn"], fx["open"])), ("oracle", H.oracle_arrays(name))):
        assert (op == rop).all() and (nn == rnn).all(), what
        assert np.isnan(cn[op]).all() and np.isnan(om[op]).all() and (nn[op] == 0).all()
        d_cn, d_om = np.abs(cn - rcn)[~op].max(initial=0.0), np.abs(om - rom)[~op].max(initial=0.0)
        print(f"{name} against {what}: cn {d_cn:.2e} omega_max {d_om:.2e}")
        assert d_cn < H.ATOL and d_om < H.ATOL, what


# 2
@pytest.mark.parametrize("name,bulk,height,count", H.TAG_TABLE)
def test_tags_on_the_table(name, bulk, height, count):
    row = H.fcc_bulk_row() if bulk else None
    want = H.tags_of(name, row, height)
    H.assert_tag_margins(name, want, row)
    sb = H.batch_of([H.case(name)], DEV)
    sb.tags = torch.full_like(sb.tags, 7)                              # not read
    before = (sb.pos.clone(), sb.tags.clone(), sb.fixed.clone())
    out = ST.tag_surface_atoms(sb, bulk=None if row is None else fcc_row()[None], height=height, masses=masses())
    assert all(torch.equal(a, b) for a, b in zip(before, (sb.pos, sb.tags, sb.fixed))) and not hasattr(sb, "surface_cn")
    tags = out.tags.cpu().numpy()
    layer = H.layer_of(name)
    assert out.tags.dtype == torch.int64 and int(tags.sum()) == count and (tags == want["tags"]).all()
    assert torch.equal(out.fixed, (out.tags == 0).long())
    assert (tags[layer == layer.max()] == 0).all()                    # the bottom layer is never tagged: below the centre of mass
    ev = want["evaluated"]
    cn, op = out.surface_cn.cpu().numpy(), out.surface_open.cpu().numpy()
    assert np.isnan(cn[~ev]).all() and not op[~ev].any()
    o = H.oracle(name)
    assert (op[ev] == np.array([o[i]["open"] for i in np.nonzero(ev)[0]], bool)).all()
    closed = np.nonzero(ev & ~op)[0]
    assert np.abs(cn[closed] - np.array([o[i]["cn"] for i in closed])).max(initial=0.0) < H.ATOL
    if name == "111_3x3x4_vacancy" and bulk:
        under = (tags == 1) & (layer == 1)
        assert int(under.sum()) == 3 and np.abs(cn[under] - 9.6).max() < 1e-3


def test_tags_with_a_batch_of_bulks_equal_tags_with_the_table():
    sb = H.batch_of([H.case("111_3x3x4_vacancy"), H.case("110_2x2x6")], DEV)
    bulks = H.batch_of([H.case("fcc_primitive")] * 2, DEV)
    a = ST.tag_surface_atoms(sb, bulk=bulks, masses=masses())
    b = ST.tag_surface_atoms(sb, bulk=fcc_row()[None].expand(2, 119).numpy(), masses=masses())
    assert torch.equal(a.tags, b.tags) and int(a.tags.sum()) == 11 + 8
    assert all(torch.equal(x, y) for x, y in zip(bits(a.surface_cn), bits(b.surface_cn)))


# 3
def test_a_system_gets_the_same_bits_alone_in_a_batch_reversed_and_twice():
    names = ["fcc_primitive", "111_3x3x4", "111_3x3x4_vacancy"]     # a 1-atom bulk, a slab of which nothing is selected, 35 atoms
    select = np.concatenate([H.select_mask(n) if n != "111_3x3x4" else np.zeros(36, bool) for n in names])
    cases = [H.case(n) for n in names]
    both = ST.voronoi_coordination(H.batch_of(cases, DEV), select=torch.from_numpy(select))
    again = ST.voronoi_coordination(H.batch_of(cases, DEV), select=torch.from_numpy(select))
    rsel = np.concatenate([select[37:], select[1:37], select[:1]])
    rev = ST.voronoi_coordination(H.batch_of(cases[::-1], DEV), select=torch.from_numpy(rsel))
    nothing = rows_of(both, names, "111_3x3x4")
    assert torch.isnan(nothing[0]).all() and (nothing[2] == 0).all() and not nothing[3].any()
    rtag_in = H.batch_of(cases[::-1], DEV)
    table = fcc_row()[None].expand(3, 119).contiguous()
    tag_both = ST.tag_surface_atoms(H.batch_of(cases, DEV), bulk=table, masses=masses())
    tag_rev = ST.tag_surface_atoms(rtag_in, bulk=table, masses=masses())
    for name in ("fcc_primitive", "111_3x3x4_vacancy"):
        c = H.case(name)
        alone = ST.voronoi_coordination(H.batch_of([c], DEV))
        want = bits(*rows_of(both, names, name))
        for other, onames in ((again, names), (rev, names[::-1]), (alone, [name])):
            assert all(torch.equal(x, y) for x, y in zip(want, bits(*rows_of(other, onames, name)))), name
        assert torch.equal(rows_of(all_cases_run(), NAMES, name)[0].view(torch.int64), want[0])   # and in the batch of all cases
        tag_alone = ST.tag_surface_atoms(H.batch_of([c], DEV), bulk=fcc_row()[None], masses=masses())
        start, rstart = sum(len(H.case(n)["Z"]) for n in names[:names.index(name)]), 0 if name == names[-1] else 35 + 36
        n = len(c["Z"])
        for t, s in ((tag_both, start), (tag_rev, rstart)):
            assert torch.equal(t.tags[s:s + n], tag_alone.tags)
            assert torch.equal(t.surface_cn[s:s + n].view(torch.int64), tag_alone.surface_cn.view(torch.int64))
    assert int(tag_both.tags[:1].sum()) == 1                          # one atom: the highest of its system


# 4
def test_bulk_coordination_is_the_least_per_element():
    table = ST.bulk_coordination(H.batch_of([H.case(n) for n in BULK_NAMES], DEV))
    want = H.bulk_table(BULK_NAMES)
    assert table.dtype == torch.float64 and tuple(table.shape) == (4, 119)
    got = table.cpu().numpy()
    assert (np.isinf(got) == np.isinf(want)).all() and (got[np.isinf(got)] > 0).all()
    finite = np.isfinite(want)
    assert np.abs(got[finite] - want[finite]).max() < H.ATOL
    assert int(np.isfinite(got).sum()) == 1 + 1 + 2 + 2
    cn = H.oracle_arrays("fcc4_rattled")[0]
    assert len(np.unique(np.round(cn, 6))) == 4                       # four distinct values, two per element
    b = BULK_NAMES.index("fcc4_rattled")
    assert abs(got[b, 78] - cn[:2].min()) < H.ATOL and abs(got[b, 29] - cn[2:].min()) < H.ATOL


# 5
GUARD, SENTINEL = 4, -77


def raw_voronoi(cases, cutoff=H.CUTOFF, offsets=None):
    sb = H.batch_of(cases, DEV)
    B, N = len(cases), int(sb.pos.shape[0])
    off = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    off[1:] = torch.cumsum(sb.natoms.reshape(-1), 0).to(torch.int32)
    if offsets is not None:
        off = torch.tensor(offsets, dtype=torch.int32, device=DEV)
    pos, cell = sb.pos.float().contiguous(), sb.cell.float().reshape(B, 9).contiguous()
    pbc = torch.ones(B, 3, dtype=torch.int32, device=DEV)
    cn = torch.full((N + GUARD,), float(SENTINEL), dtype=torch.float64, device=DEV)
    om = torch.full((N + GUARD,), float(SENTINEL), dtype=torch.float64, device=DEV)
    nn = torch.full((N + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    fl = torch.full((N + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    status = L.load().adf_voronoi_coordination(pos.data_ptr(), cell.data_ptr(), pbc.data_ptr(), off.data_ptr(), N, B, None,
                                               C.c_double(cutoff), C.c_double(H.WEIGHT_TOL), C.c_double(H.FAR), cn.data_ptr(),
                                               om.data_ptr(), nn.data_ptr(), fl.data_ptr(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, N, [t.cpu() for t in (cn, om, nn, fl)]


def raw_tags(cases, table, height=H.HEIGHT, mass_table=None):
    sb = H.batch_of(cases, DEV)
    B, N = len(cases), int(sb.pos.shape[0])
    off = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    off[1:] = torch.cumsum(sb.natoms.reshape(-1), 0).to(torch.int32)
    pos, cell = sb.pos.float().contiguous(), sb.cell.float().reshape(B, 9).contiguous()
    pbc = torch.ones(B, 3, dtype=torch.int32, device=DEV)
    Z = sb.atomic_numbers.to(torch.int32).contiguous()
    m = torch.from_numpy(masses() if mass_table is None else mass_table).to(DEV)
    table = torch.as_tensor(table).to(DEV, torch.float64).contiguous()
    tags = torch.full((N + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    cn = torch.full((N + GUARD,), float(SENTINEL), dtype=torch.float64, device=DEV)
    fl = torch.full((N + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    status = L.load().adf_tag_surface_atoms(pos.data_ptr(), cell.data_ptr(), pbc.data_ptr(), Z.data_ptr(), off.data_ptr(), N, B,
                                            m.data_ptr(), table.data_ptr(), C.c_double(height), C.c_double(H.CUTOFF),
                                            C.c_double(H.WEIGHT_TOL), C.c_double(H.FAR), C.c_double(H.CN_TOL), tags.data_ptr(),
                                            cn.data_ptr(), fl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, N, [t.cpu() for t in (tags, cn, fl)]


def test_refused_arguments_leave_the_outputs_alone():
    good = [H.case("fcc4_rattled"), H.case("fcc_primitive")]
    status, N, outs = raw_voronoi(good)                               # fine, and nothing past the rows
    assert status == L.ADF_OK and all((t[N:] == SENTINEL).all() for t in outs) and (outs[3][:N] == 0).all()
    assert (outs[2][:N] == 12).all()
    for kw, code, what in ((dict(cutoff=30.0), L.ADF_EOVERFLOW, b"more than 1024 candidates"),
                           (dict(offsets=[0, 5, 4]), L.ADF_EINVAL, b"offsets"),
                           (dict(offsets=[0, 4, 6]), L.ADF_EINVAL, b"offsets"),
                           (dict(cutoff=float("nan")), L.ADF_EINVAL, b"cutoff"),
                           (dict(cutoff=float("inf")), L.ADF_EINVAL, b"cutoff")):
        status, N, outs = raw_voronoi(good, **kw)
        assert status == code and what in L.load().adf_last_error(), (kw, L.load().adf_last_error())
        assert all((t == SENTINEL).all() for t in outs), kw          # nothing is written, the guard rows least of all
    status, _, _ = raw_voronoi(good, cutoff=30.0)
    assert b"atom 0" in L.load().adf_last_error()                     # the message names the first such atom
    slabs = [H.case("111_3x3x4_vacancy"), H.case("110_2x2x6")]
    table = np.stack([H.fcc_bulk_row()] * 2)
    status, N, outs = raw_tags(slabs, table)
    assert status == L.ADF_OK and all((t[N:] == SENTINEL).all() for t in outs) and int(outs[0][:N].sum()) == 11 + 8
    missing = table.copy()
    missing[1, 78] = np.inf                                           # the second slab's element is absent from its row
    status, N, outs = raw_tags(slabs, missing)
    assert status == L.ADF_EINVAL and b"absent" in L.load().adf_last_error()
    assert all((t == SENTINEL).all() for t in outs)
    with pytest.raises(ValueError, match="capacity exceeded.*1024 candidates"):
        ST.voronoi_coordination(H.batch_of(good, DEV), cutoff=30.0)
    with pytest.raises(ValueError, match="absent"):
        ST.tag_surface_atoms(H.batch_of(slabs, DEV), bulk=missing, masses=masses())
    with pytest.raises(ValueError, match="open cell"):
        ST.bulk_coordination(H.batch_of([H.case("fcc_primitive"), H.case("alone")], DEV))


def test_the_remaining_error_bits_name_their_atom():
    """The bits of the Voronoi error word that the test above does not raise, each from a system of one or four atoms and
    through the raw entries.  In every case the kernels refuse the value before anything is indexed with it: a refused
    cell or pair count clears the system's reps[3], which vo_cell_kernel tests first; an atomic number outside the tables
    ends vo_tag_prepare_kernel before its masses[Z] load; the commits return on a set error word."""
    good, one = H.case("fcc4_rattled"), H.case("fcc_primitive")
    flat = dict(one, cell=np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [2.0, 2.0, 0.0]], np.float32))
    status, N, outs = raw_voronoi([good, flat])
    assert status == L.ADF_EINVAL, L.load().adf_last_error()
    assert b"voronoi_coordination: the cell of the system of atom 4 is singular or not finite" in L.load().adf_last_error()
    assert all((t == SENTINEL).all() for t in outs)
    tiny = dict(one, pos=np.asarray(one["pos"], np.float32) * 1e-3, cell=np.asarray(one["cell"], np.float32) * 1e-3)
    status, N, outs = raw_voronoi([good, tiny])
    assert status == L.ADF_EOVERFLOW, L.load().adf_last_error()
    assert b"the system of atom 4 has more than 16777216 (atom, image) pairs within the cutoff's repeats" in L.load().adf_last_error()
    assert all((t == SENTINEL).all() for t in outs)
    table = np.full((1, 119), 12.0)
    Z = np.asarray(good["Z"]).copy()
    Z[2] = 119
    status, N, outs = raw_tags([dict(good, Z=Z)], table)
    assert status == L.ADF_EINVAL, L.load().adf_last_error()
    assert b"tag_surface_atoms: atom 2 has an atomic number outside [0, 118]" in L.load().adf_last_error()
    assert all((t == SENTINEL).all() for t in outs)
    status, N, outs = raw_tags([good], table, mass_table=np.zeros_like(masses()))
    assert status == L.ADF_EINVAL, L.load().adf_last_error()
    assert b"tag_surface_atoms: the masses of the system of atom 0 do not sum to a positive number" in L.load().adf_last_error()
    assert all((t == SENTINEL).all() for t in outs)


# 6
def test_untagged_slab_to_heuristic_sites():
    sb = HH.slab_batch(["111_3x3x4"], DEV)
    sb.tags = torch.zeros_like(sb.tags)
    sb.fixed = torch.zeros_like(sb.fixed)
    tagged = ST.tag_surface_atoms(sb, bulk=fcc_row()[None], masses=masses())
    assert int(tagged.tags.sum()) == 9 and torch.equal(tagged.fixed, (tagged.tags == 0).long())
    st = PL.heuristic_sites(tagged, triangles="device")
    kinds = st.kind.cpu().numpy()
    assert tuple(int((kinds == k).sum()) for k in range(3)) == HH.TABLE["111_3x3x4"][1] == (1, 1, 2)
    assert st.multiplicity.tolist() == [9, 27, 9, 9]
