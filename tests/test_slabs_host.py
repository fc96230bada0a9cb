"""CPU tests of slab cutting (adsorbdiff_amd/slabs.py): the float64 oracle of tests/helpers_slabs.py must give
the crystallographic facts of the case table and satisfy the invariants (a)-(g) before the device is held to it
(tests/test_gpu_slabs.py); then the host-side argument checks, the C ABI of the header's section "Slab cutting" and the per-slab keys
through ``Batch`` splitting.  Parity with pymatgen unpinned."""
import functools

import numpy as np
import pytest
import torch

from adsorbdiff_amd import build as BUILD
from adsorbdiff_amd import lib as L
from adsorbdiff_amd import slabs as SL
from adsorbdiff_amd.data import Batch
from tests import helpers_slabs as H

CRYSTALS = H.crystals()


@functools.lru_cache(maxsize=None)
def cut(name, h):
    return H.cut_slabs(CRYSTALS[name], h)


@pytest.mark.parametrize("case", H.CASE_TABLE, ids=lambda c: f"{c[0]}-{''.join(map(str, c[1]))}")
def test_oracle_reproduces_the_case_table(case):
    name, h, d, n_slab, cuts, n_out, n_atoms, layers = case
    slabs, facts = cut(name, h)
    if d is not None:
        assert round(facts["d"], 4) == d
    assert (facts["n_slab"], facts["kept"], len(slabs)) == (n_slab, cuts, n_out)
    assert all(len(s["pos"]) == n_atoms and H.count_layers(s) == layers for s in slabs)
    assert [s["top"] for s in slabs] == sorted((s["top"] for s in slabs), reverse=True)
    tops = [s for s in slabs if s["top"]]
    assert [s["shift"] for s in tops] == sorted(s["shift"] for s in tops) and all(0.0 <= s["shift"] < facts["d"] for s in slabs)


@pytest.mark.parametrize("pair", H.all_pairs()[1], ids=lambda p: f"{p[0]}-{''.join(map(str, p[1]))}")
def test_oracle_slabs_satisfy_the_invariants(pair):
    name, h = pair
    slabs, facts = cut(name, h)
    tops = {s["shift"]: s for s in slabs if s["top"]}
    for s in slabs:
        H.check_invariants(CRYSTALS[name], s, facts, partner=None if s["top"] else tops[s["shift"]])


def test_oracle_named_facts():
    # two cuts of fcc (100) merge under an in-plane translation, the two of hcp (001) under the two-fold rotation
    assert cut("fcc_cu", (1, 0, 0))[1]["cuts"] == 2 and cut("fcc_cu", (1, 0, 0))[1]["kept"] == 1
    assert cut("hcp_mg", (0, 0, 1))[1]["cuts"] == 2 and cut("hcp_mg", (0, 0, 1))[1]["kept"] == 1
    # hcp (100): the short and the long termination
    a, b = cut("hcp_mg", (1, 0, 0))[0]
    gap = lambda s: np.sort(s["pos"][:, 2])[-1] - np.sort(s["pos"][:, 2])[-2]
    assert abs(gap(a) - gap(b)) > 0.5
    # the triclinic (1 -1 2): two layers closer than tol share a termination
    assert cut("triclinic", (1, -1, 2))[1]["cuts"] == 1
    # CsCl (100): the four slabs show Cs, Cl, then the other species on top
    top_species = [int(s["Z"][np.argmax(s["pos"][:, 2])]) for s in cut("cscl", (1, 0, 0))[0]]
    assert sorted(top_species[:2]) == [17, 55] and top_species[2:] == top_species[1::-1]
    # an unreduced or negated index is the reduced one, or its other face
    assert cut("fcc_cu", (2, 2, 2))[0][0]["millers"] == (1, 1, 1)
    assert np.array_equal(cut("fcc_cu", (2, 2, 2))[0][0]["pos"], cut("fcc_cu", (1, 1, 1))[0][0]["pos"])


@pytest.mark.parametrize("name", list(H.MILLER_TABLE))
def test_oracle_distinct_millers(name):
    order, n1, n2 = H.MILLER_TABLE[name]
    m1, o1 = H.distinct_millers(CRYSTALS[name], 1)
    m2, o2 = H.distinct_millers(CRYSTALS[name], 2)
    assert (o1, o2, len(m1), len(m2)) == (order, order, n1, n2)
    assert m2 == sorted(m2, reverse=True) and m1 == sorted(m1, reverse=True)   # (a class's representative depends on the box)
    if order == 48:
        assert m2 == [(2, 2, 1), (2, 1, 1), (2, 1, 0), (1, 1, 1), (1, 1, 0), (1, 0, 0)]


def test_oracle_refuses():
    with pytest.raises(ValueError):
        H.cut_slabs(CRYSTALS["fcc_cu"], (0, 0, 0))
    left = dict(CRYSTALS["fcc_cu"], cell=CRYSTALS["fcc_cu"]["cell"][[1, 0, 2]])
    with pytest.raises(ValueError):
        H.cut_slabs(left, (1, 0, 0))
    with pytest.raises(ValueError):
        H.distinct_millers(CRYSTALS["fcc_cu"], 5)
    with pytest.raises(ValueError):
        H.cut_slabs(CRYSTALS["fcc_cu"], (1, 0, 0), tol=float("nan"))


# ---- host logic of adsorbdiff_amd/slabs.py
def cpu_batch(names=("fcc_cu", "cscl")):
    b = Batch()
    b.pos = torch.cat([torch.from_numpy(CRYSTALS[n]["pos"]) for n in names])
    b.cell = torch.stack([torch.from_numpy(CRYSTALS[n]["cell"]) for n in names])
    b.atomic_numbers = torch.cat([torch.from_numpy(CRYSTALS[n]["Z"]) for n in names])
    b.natoms = torch.tensor([len(CRYSTALS[n]["Z"]) for n in names])
    return b


@pytest.mark.parametrize("kw", [dict(min_slab_size=0.0), dict(min_slab_size=float("nan")), dict(min_vacuum_size=-1.0),
                                dict(min_vacuum_size=float("inf")), dict(tol=0.0), dict(symprec=float("nan")), dict(max_miller=0),
                                dict(max_miller=5), dict(max_miller=1.5)])
def test_argument_checks(kw):
    with pytest.raises(ValueError):
        SL.compute_slabs(cpu_batch(), **kw)
    if "max_miller" in kw or "symprec" in kw:
        with pytest.raises(ValueError):
            SL.distinct_millers(cpu_batch(), **kw)


def test_no_cpu_fallback_and_pbc():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SL.compute_slabs(cpu_batch())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SL.distinct_millers(cpu_batch())


def test_specific_millers_forms():
    bulk, hkl = SL._pairs([(1, 1, 1), (1, 0, 0)], 2, "cpu")
    assert bulk.tolist() == [0, 0, 1, 1] and hkl.tolist() == [[1, 1, 1], [1, 0, 0]] * 2 and hkl.dtype == torch.int32
    bulk, hkl = SL._pairs([[(1, 1, 1)], [(1, 0, 0), (2, 1, 0), (1, 1, 0)]], 2, "cpu")
    assert bulk.tolist() == [0, 1, 1, 1] and hkl.tolist() == [[1, 1, 1], [1, 0, 0], [2, 1, 0], [1, 1, 0]]
    for bad in ([], [[(1, 1, 1)]], [(1.5, 0, 0)], [(1, 1)], [[(1, 1, 1)], []]):
        with pytest.raises(ValueError):
            SL._pairs(bad, 2, "cpu")


def test_c_abi_of_the_slab_header():
    names = ["adf_distinct_millers_scratch", "adf_distinct_millers_count", "adf_distinct_millers_fill",
             "adf_slab_cut_scratch", "adf_slab_cut_count", "adf_slab_cut_fill"]
    at = L.EXPORTS.index(names[0])
    assert list(L.EXPORTS[at:at + len(names)]) == names and "slabcut.hip" in BUILD.SOURCES
    lib = L.load()
    for name in names:
        restype, argtypes = L.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    small, large = lib.adf_slab_cut_scratch(8, 2), lib.adf_slab_cut_scratch(800, 2)
    assert small % 256 == 0 and large >= 800 * (5 * 8 + 3 * 4) + 2 * (80 * 8 + 32 * 4) and small < large and lib.adf_slab_cut_scratch(-1, 2) == 0
    assert lib.adf_distinct_millers_scratch(4, 1) >= 48 * 9 * 4 + 4 * 3 * 8


def test_per_slab_keys_survive_splitting():
    b = Batch()
    b.pos = torch.zeros(5, 3)
    b.atomic_numbers = torch.arange(5)
    b.natoms = torch.tensor([2, 3])
    b.cell = torch.eye(3).repeat(2, 1, 1)
    b.millers = torch.tensor([[1, 1, 1], [2, 1, 0]], dtype=torch.int32)
    b.shift = torch.tensor([0.25, 1.5], dtype=torch.float64)
    b.top = torch.tensor([True, False])
    b.bulk_index = torch.tensor([0, 3])
    parts = b.to_data_list()
    assert parts[1].millers.tolist() == [[2, 1, 0]] and parts[1].shift.tolist() == [1.5] and parts[1].top.tolist() == [False]
    back = Batch.from_data_list(parts[::-1])
    assert back.millers.tolist() == [[2, 1, 0], [1, 1, 1]] and back.bulk_index.tolist() == [3, 0]
    assert back.shift.dtype == torch.float64 and back.top.tolist() == [False, True] and back.natoms.tolist() == [3, 2]


def test_bulk_and_slab_classes_on_the_host():
    c = CRYSTALS["cscl"]
    bulk = SL.Bulk(c["pos"], c["cell"], c["Z"], src_id="mp-cscl", device="cpu")
    assert len(bulk) == 2 and bulk.batch().natoms.tolist() == [2] and bulk.batch().cell.shape == (1, 3, 3)
    with pytest.raises(ValueError):
        SL.Bulk(c["pos"], c["cell"], c["Z"][:1])
    one = Batch()
    one.pos = torch.zeros(2, 3)
    one.atomic_numbers = torch.tensor([55, 17])
    one.tags = torch.tensor([0, 1])
    one.cell = torch.eye(3).reshape(1, 3, 3) * 9.0
    slab = SL.Slab(bulk, one, (1, 0, 0), 0.75, True)
    assert slab.get_metadata_dict()["slab_metadata"] == {"bulk_id": "mp-cscl", "millers": (1, 0, 0), "shift": 0.75, "top": True}
    assert len(slab) == 2 and slab.has_surface_tagged()
    one.tags = torch.tensor([0, 0])
    with pytest.raises(ValueError, match="not tagged"):
        SL.Slab(bulk, one, (1, 0, 0), 0.75, True)
    with pytest.raises(ValueError, match="tuple"):
        SL.Slab.from_bulk_get_specific_millers([1, 0, 0], bulk)
