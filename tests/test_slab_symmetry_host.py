"""CPU tests of the slab symmetry stage: the float64 oracle of tests/helpers_slab_symmetry.py against crystallography (the
operation counts of fcc slabs are known), against a wider enumeration and against the group axioms; the symmetric distance
by hand; the C entries; the host side of ``slab_symmetry`` and of the ``symmetry=`` keywords."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import ml_relaxation as MR
from adsorbdiff_amd import site_select as SS
from adsorbdiff_amd import slab_symmetry as SY
from tests import helpers_slab_symmetry as H
from tests import helpers_unique_sites as U

ROOT = Path(__file__).resolve().parent.parent
HOST_SLABS = [n for n in H.SLABS if n != "111_7x7x4"]


@pytest.mark.parametrize("name", HOST_SLABS)
def test_oracle_counts_are_crystallographic(name):
    ops, _, _ = H.oracle(name)                                          # asserts the margins
    assert len(ops) == H.SLABS[name][1]
    o = ops[0]
    assert (o["R"] == np.eye(3)).all() and (o["t"] == 0).all() and o["perm"].tolist() == list(range(len(o["perm"])))
    keys = [tuple(p["W"].reshape(-1).tolist()) + (p["j"],) for p in ops[1:]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    proper, _, _ = H.oracle(name, True)
    assert len(proper) == (len(ops) // 2 if name in H.MIRRORS else len(ops))
    assert all(round(np.linalg.det(p["R"])) == 1 for p in proper)


def test_oracle_counts_of_the_issue_table():
    assert len(H.oracle("111_1x1x3", True)[0]) == 3
    assert [len(H.oracle(n)[0]) for n in ("111_1x1x3", "111_2x2x3", "111_3x3x4", "100_1x1x2", "100_2x2x3", "110_1x1x2",
                                          "substituted", "non_reduced", "left_handed", "rattled", "one_atom")] == \
        [6, 24, 54, 8, 32, 4, 6, 24, 24, 1, 12]


@pytest.mark.parametrize("kind", ["111", "100", "110"])
def test_wider_enumeration_finds_no_further_point_operation(kind):
    """A cell written as (a + 3b, b): entries in [-3, 3] in the reduced basis give the point operations {-1, 0, 1} gave."""
    _, _, c = H.fcc(kind, 2, 3, 2)
    c = c.copy()
    c[0] = c[0] + 3 * c[1]
    narrow, _ = H.point_ops(c, H.SYMPREC, span=1)
    wide, _ = H.point_ops(c, H.SYMPREC, span=3)
    assert [w.tolist() for w in narrow] == [w.tolist() for w in wide] and len(narrow) >= 2
    # the reduction did work: the given basis is not reduced
    assert np.abs(H.lagrange(c[:2].T.astype(np.float64))).max() > 1


@pytest.mark.parametrize("name", [n for n in HOST_SLABS if n != "111_5x5x3"])
def test_operations_form_a_group(name):
    p, Z, c = H.slab(name)
    ops = H.oracle(name)[0]
    H.assert_group(ops, Z, c)
    H.assert_maps_slab(ops, p, c)


def test_symmetric_distance_sees_an_image_as_the_same_site():
    rng = np.random.default_rng(3)
    for name, n_ads in (("111_2x2x3", 5), ("100_2x2x3", 2), ("substituted", 1)):
        ops = H.oracle(name)[0]
        a = H.base_site(name, n_ads, 0, rng)
        for k in (1, len(ops) // 2, len(ops) - 1):
            b = H.apply_op(a, ops[k], cast=False)
            b = dict(b, pos=b["pos"].astype(np.float32))
            assert H.pair_distance(a, b) > 10 * H.TOL                   # the plain distance: another site
            D, best = H.sym_group_distances([a, b], ops)
            assert D[0, 1] < 1e-5 and D[1, 0] == D[0, 1] and best[0, 1] == best[1, 0]
            moved = H.apply_op(a, ops[int(best[0, 1])])
            assert H.pair_distance(moved, b) == D[0, 1]
    # the identity alone is section 4h's distance
    D, best = H.sym_group_distances([a, b], ops[:1])
    assert D[0, 1] == H.pair_distance(a, b) and best[0, 1] == 0


def test_generated_distance_case_meets_its_margins():
    sites, names = H.distance_case()
    group = [s["group"] for s in sites]
    _, members = U.regroup_numpy(group)
    # the oracle's row function is section 4h's oracle, row by row
    for m in members[:4]:
        g = [sites[i] for i in m]
        for inc, pi in ((True, True), (True, False), (False, True), (False, False)):
            D = U.group_distances(g, inc, pi)[0]
            assert all(np.array_equal(H.row_distances(g[i], g[i + 1:], inc, pi), D[i, i + 1:]) for i in range(len(g) - 1))
    assert [len(m) for m in members] == [1, 2, 3, 6, 65] and group != sorted(group)
    assert {int((s["tags"] == 2).sum()) for s in sites} == {0, 1, 2, 5}
    D, best = H.distance_oracle()                                       # asserts the margins
    assert any(np.isinf(d).any() for d in D) and max(int(b.max()) for b in best) > 0
    plain, _ = U.case_distances(sites)
    rep_sym, n_sym = U.unique_sites(D, group, H.TOL)
    rep_plain, n_plain = U.unique_sites(plain, group, H.TOL)
    assert n_sym.sum() < n_plain.sum()
    assert n_sym.tolist()[4] == 12                                      # the 65-site group: its 12 base sites


def test_c_entries_are_declared_and_exported():
    lib = L.load()
    header = (ROOT / "include" / "adsorbdiff_hip.h").read_text()
    for name in ("adf_slab_symmetry_scratch", "adf_slab_symmetry_search", "adf_slab_symmetry_emit", "adf_site_pair_distances_sym"):
        assert name in L.EXPORTS and hasattr(lib, name) and f" {name}(" in header, name
    assert "symmetry.hip" in __import__("adsorbdiff_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.adf_slab_symmetry_scratch(200, 2) > 200 * (16 + 2 * 48)
    assert lib.adf_slab_symmetry_search(None, None, None, None, 0, 0, C.c_double(0.01), 0, None, None, None, None) == L.ADF_EINVAL
    assert b"slab_symmetry_search" in lib.adf_last_error()
    assert lib.adf_slab_symmetry_emit(None, 0, 0, C.c_double(0.01), None, None, None, 0, 0, None, None, None, None, None) == L.ADF_EINVAL
    assert b"slab_symmetry_emit" in lib.adf_last_error()
    assert lib.adf_site_pair_distances_sym(None, None, None, None, None, None, None, 0, 0, 0, 0, 1, 1, None, None, None, None,
                                           None, 0, 0, None, None, None) == L.ADF_EINVAL
    assert b"site_pair_distances_sym" in lib.adf_last_error()


def test_identity_symmetry_and_group_layout():
    sym = SY.SlabSymmetry.identity([3, 5, 2], "cpu")
    assert sym.counts == [1, 1, 1] and sym.perm.tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 0, 1]
    assert sym.perm_offset.tolist() == [0, 3, 8, 10] and sym.op_offset.tolist() == [0, 1, 2, 3]
    assert sym.ops(1)[3].tolist() == [[0, 1, 2, 3, 4]]
    assert sym.for_groups([0, 1, 2])[0] is sym.op_offset
    op_off, rot, trans, perm, perm_off, K, P = sym.for_groups([0, 2])
    assert op_off.tolist() == [0, 1, 2] and perm.tolist() == [0, 1, 2, 0, 1] and perm_off.tolist() == [0, 3, 5] and (K, P) == (2, 5)
    with pytest.raises(ValueError, match="group id is its slab's index"):
        sym.for_groups([0, 3])


def _as_symmetry(ops_per_slab, sizes):
    """An oracle's operations as a SlabSymmetry on the CPU."""
    counts = [len(o) for o in ops_per_slab]
    flat = [o for ops in ops_per_slab for o in ops]
    off = np.concatenate([[0], np.cumsum(counts)])
    poff = np.concatenate([[0], np.cumsum([c * n for c, n in zip(counts, sizes)])])
    return SY.SlabSymmetry(n_ops=torch.tensor(counts), op_offset=torch.tensor(off, dtype=torch.int32),
                           rot=torch.tensor(np.stack([o["R"] for o in flat])), trans=torch.tensor(np.stack([o["t"] for o in flat])),
                           W=torch.tensor(np.stack([o["W"].reshape(-1) for o in flat]), dtype=torch.int32),
                           perm=torch.tensor(np.concatenate([o["perm"] for o in flat]), dtype=torch.int32),
                           perm_offset=torch.tensor(poff), natoms=torch.tensor(sizes), counts=counts, sizes=list(sizes))


def test_carry_follows_the_oracle_in_both_directions():
    """``carry`` (torch, any device) against ``apply_op``: forward it is g . site, inverse it undoes it; op 0 returns the bits."""
    rng = np.random.default_rng(8)
    names = ["111_2x2x3", "substituted"]
    sym = _as_symmetry([H.oracle(n)[0] for n in names], [len(H.slab(n)[1]) for n in names])
    sites = [H.base_site("111_2x2x3", 5, 0, rng), H.base_site("substituted", 1, 1, rng), H.base_site("111_2x2x3", 2, 0, rng)]
    slab, op = torch.tensor([0, 1, 0]), torch.tensor([7, 4, 0])
    b = U.to_batch(sites)
    force = torch.from_numpy(rng.normal(size=tuple(b.pos.shape))).float()
    fwd, f_fwd = SY.carry(sym, slab, op, torch.tensor([False, False, False]), b.tags, b.natoms, b.pos, force)
    want = [H.apply_op(sites[0], H.oracle(names[0])[0][7]), H.apply_op(sites[1], H.oracle(names[1])[0][4]), sites[2]]
    at = 0
    for s, w in zip(sites, want):
        n = len(s["Z"])
        assert np.abs(fwd[at:at + n].numpy() - w["pos"]).max() < 1e-5
        at += n
    n2 = len(sites[2]["Z"])
    assert torch.equal(fwd[-n2:], b.pos[-n2:]) and torch.equal(f_fwd[-n2:], force[-n2:])
    back, f_back = SY.carry(sym, slab, op, torch.tensor([True, True, False]), b.tags, b.natoms, fwd, f_fwd)
    assert float((back - b.pos).abs().max()) < 2e-5 and float((f_back - force).abs().max()) < 1e-5
    # forces turn with R and ignore tau
    R = H.oracle(names[0])[0][7]["R"]
    n0, ns = len(sites[0]["Z"]), len(H.slab(names[0])[1])
    assert np.abs(f_fwd[ns:n0].numpy() - force[ns:n0].numpy() @ R.T).max() < 1e-5


def test_argument_errors_need_no_device():
    b = U.to_batch(U.chain_case())
    sym = SY.SlabSymmetry.identity([8], "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SY.find_symmetry(H.slab_batch(["111_1x1x3"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SS.site_distances(b, symmetry=sym)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SS.unique_sites(b, symmetry=sym, return_op=True)
    with pytest.raises(ValueError, match="return_op needs symmetry"):
        SS.unique_sites(b, return_op=True)


def test_ml_relax_unique_carries_the_representative_through_the_operation(monkeypatch):
    """The plumbing alone (clustering and optimizer are stand-ins): a duplicate merged under an operation gets its
    representative's result through ``carry`` in the recorded direction, a plain copy the bits."""
    class StubLBFGS:
        def __init__(self, batch, calc, **kw):
            self.batch = batch

        def run(self, fmax, steps):
            self.batch.pos += 0.25
            self.batch.y = torch.tensor([float(s) for s in self.batch.sid])
            self.batch.force = -self.batch.pos
            return self.batch

    name = "111_2x2x3"
    ops = H.oracle(name)[0]
    sym = _as_symmetry([ops], [len(H.slab(name)[1])])
    rng = np.random.default_rng(4)
    a = H.base_site(name, 2, 0, rng)
    sites = [a, H.apply_op(a, ops[5]), dict(a), H.apply_op(a, ops[9])]
    sites = [dict(s, pos=np.asarray(s["pos"], np.float32)) for s in sites]
    rep = torch.tensor([2, 2, 2, 2])
    site_op, inverse = torch.tensor([0, 5, 0, 9]), torch.tensor([False, True, False, False])

    def fake_unique(batch, group=None, tol=0.05, **kw):
        assert kw == {"symmetry": sym, "return_op": True}
        return rep, rep == torch.arange(4), torch.tensor([1]), site_op, inverse

    monkeypatch.setattr(MR, "LBFGS", StubLBFGS)
    monkeypatch.setattr(SS, "unique_sites", fake_unique)
    b = U.to_batch(sites)
    out = MR.ml_relax_unique(b, None, 5, 0.05, {"memory": 7}, False, symmetry=sym, device="cpu")
    n = len(a["Z"])
    relaxed = b.pos[2 * n:3 * n] + 0.25
    assert torch.equal(out.pos[:n], relaxed) and torch.equal(out.pos[2 * n:3 * n], relaxed) and out.y.tolist() == [2.0] * 4
    assert torch.equal(out.site_op, site_op) and torch.equal(out.site_op_inverse, inverse)
    r = dict(a, pos=relaxed.numpy())
    later = H.apply_op(r, ops[9])                                       # site 3 comes after its representative: g . r
    assert np.abs(out.pos[3 * n:].numpy() - later["pos"]).max() < 1e-5
    earlier = out.pos[n:2 * n].numpy()                                   # site 1 comes before it: g . s = r
    assert np.abs(H.apply_op(dict(a, pos=earlier), ops[5])["pos"] - relaxed.numpy()).max() < 2e-5
    assert np.abs(out.force[3 * n:].numpy()[-2:] - (-relaxed.numpy()[-2:]) @ ops[9]["R"].T).max() < 1e-5


# adf_slab_symmetry_scratch sizes caller-owned memory, so its numbers are a contract: recorded from the build that laid the
# scratch out by hand (five regions, each rounded up to 256 bytes), before the layout moved to the shared carver
SCRATCH_BYTES = {(0, 0): 0, (1, 1): 2048, (7, 3): 5120, (64, 1): 8448, (1000, 16): 132864, (200000, 1000): 23680000}


@pytest.mark.parametrize("num_atoms,num_slabs", sorted(SCRATCH_BYTES))
def test_scratch_size_is_unchanged(num_atoms, num_slabs):
    assert L.load().adf_slab_symmetry_scratch(num_atoms, num_slabs) == SCRATCH_BYTES[(num_atoms, num_slabs)]
