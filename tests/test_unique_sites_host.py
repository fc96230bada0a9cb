"""CPU tests of the duplicate-site stage: the float64 oracle against a brute-force search over lattice images and on hand-built
cases, the generators' margins, the C entries, and the host side of ``site_select`` (index maps, argument errors)."""
import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import ml_relaxation as MR
from adsorbdiff_amd import site_select as SS
from adsorbdiff_amd.flag_anomaly import regroup
from tests import helpers_unique_sites as H

ROOT = Path(__file__).resolve().parent.parent


def test_oracle_displacement_is_the_minimum_image_in_an_orthorhombic_cell():
    """Displacements shorter than half of every cell length, each moved by a random lattice vector: the convention gives the
    true shortest image, found by trying all 27 neighbours."""
    rng = np.random.default_rng(0)
    cell = H.ORTHO
    lengths = np.diag(cell)
    short = rng.uniform(-0.49, 0.49, (200, 3)) * lengths
    moved = short + rng.integers(-2, 3, (200, 3)) @ cell
    vec, frac = H.min_diff(moved, cell)
    images = np.asarray(list(itertools.product((-1, 0, 1), repeat=3))) @ cell
    brute = np.linalg.norm(vec[:, None, :] + images[None], axis=-1).min(1)
    assert np.abs(np.linalg.norm(vec, axis=-1) - brute).max() < 1e-12
    assert np.abs(vec - short).max() < 1e-9 and np.abs(frac).max() <= 0.5
    # the whole distance: a site against a copy whose atoms each sit on another lattice image
    rng = np.random.default_rng(1)
    a, = H._family(rng, 1, 12, [6, 8, 1], cell, 0)
    shift = np.array([0.011, -0.007, 0.004])
    b = dict(a, pos=(a["pos"].astype(np.float64) + shift + rng.integers(-1, 2, (15, 3)) @ cell).astype(np.float32))
    D, seam = H.group_distances([a, b])
    assert seam > 0.4 and abs(D[0, 1] - np.linalg.norm(shift)) < 1e-5 and D[1, 0] == D[0, 1] and D[0, 0] == 0


def test_oracle_adsorbate_distances_by_hand():
    rng = np.random.default_rng(2)
    a, = H._family(rng, 1, 8, [7, 7], H.ORTHO, 0)
    a["pos"][-1] = a["pos"][-2] + np.float32([1.1, 0, 0])
    flipped = H.duplicate(a, np.random.default_rng(3), flip=True)
    shift = np.linalg.norm(flipped["pos"][0].astype(np.float64) - a["pos"][0])
    assert 0.2 * H.TOL - 1e-6 <= shift <= 0.4 * H.TOL + 1e-6
    D, _ = H.group_distances([a, flipped], permutation_invariant=True)
    assert abs(D[0, 1] - shift) < 1e-5                                     # upside down is the same site
    D, _ = H.group_distances([a, flipped], permutation_invariant=False)
    assert abs(D[0, 1] - 1.1) < 0.03                                       # atom by atom it is a bond length away
    D, _ = H.group_distances([a, flipped], include_slab=False, permutation_invariant=False)
    assert abs(D[0, 1] - 1.1) < 0.03
    # below half the shortest same-element separation the two adsorbate distances agree
    moved = H.duplicate(a, np.random.default_rng(4))
    assert H.group_distances([a, moved], permutation_invariant=True)[0][0, 1] == pytest.approx(
        H.group_distances([a, moved], permutation_invariant=False)[0][0, 1], abs=1e-12)
    # different elements never pair up; different layouts cannot be compared; no adsorbate: the slab alone
    other = dict(a, Z=np.concatenate([a["Z"][:-1], [8]]))
    assert np.isinf(H.group_distances([a, other])[0][0, 1])
    assert np.isinf(H.group_distances([a, dict(a, pos=a["pos"][:-1], tags=a["tags"][:-1], Z=a["Z"][:-1])])[0][0, 1])
    bare, = H._family(rng, 1, 8, [], H.ORTHO, 0)
    assert H.group_distances([bare, bare], include_slab=False)[0][0, 1] == 0


def test_oracle_clustering_by_hand():
    chain = H.chain_case()
    M, seam = H.case_distances(chain)
    H.assert_margins(M, seam, [0, 0, 0], H.TOL)
    assert M[0][0, 1] < H.TOL and M[0][1, 2] < H.TOL and M[0][0, 2] > H.TOL
    rep, n = H.unique_sites(M, [0, 0, 0], H.TOL)
    assert rep.tolist() == [0, 0, 2] and n.tolist() == [2]                  # a takes b; c is not close to a
    rep, n = H.unique_sites(M, [0, 0, 0], H.TOL, energy=np.float32([1, 0, 2]))
    assert rep.tolist() == [1, 1, 1] and n.tolist() == [1]                  # b first: it takes both
    # an energy tie goes to the earlier site, in the clustering and in the ranking
    rep, _ = H.unique_sites(M, [0, 0, 0], H.TOL, energy=np.float32([1, 1, 1]))
    assert rep.tolist() == [0, 0, 2]
    top, top_e = H.top_sites(np.float32([1, 1, 0.5, 1]), None, [0, 0, 0, 0], 3)
    assert top.tolist() == [[2, 0, 1]] and top_e.tolist() == [[0.5, 1, 1]]
    # an invalid site is no representative and is never merged; the energy tolerance splits a cluster
    flags = np.zeros((3, 4), int)
    flags[0, 2] = 1
    rep, n = H.unique_sites(M, [0, 0, 0], H.TOL, flags=flags)
    assert rep.tolist() == [-1, 1, 1] and n.tolist() == [1]
    rep, n = H.unique_sites(M, [0, 0, 0], H.TOL, energy=np.float32([np.nan, 0.0, 0.2]), energy_tol=0.1)
    assert rep.tolist() == [-1, 1, 2] and n.tolist() == [2]
    top, top_e = H.top_sites(np.float32([0.3, np.nan, 0.1, 0.2]), np.array([[0] * 4, [0] * 4, [0, 1, 0, 0], [0] * 4]), [5, 5, 5, 5], 3,
                             rep=np.array([0, -1, 2, 0]))
    assert top.tolist() == [[0, -1, -1]] and top_e[0, 0] == np.float32(0.3) and np.isinf(top_e[0, 1:]).all()


def test_generated_cases_meet_their_margins():
    sites, energy = H.main_case()
    group = H.groups_of(sites)
    ids, members = H.regroup_numpy(group)
    assert sorted(len(m) for m in members) == [1, 2, 2, 3, 3, 4, 65]
    assert group.tolist() != sorted(group.tolist())                          # interleaved in the caller's order
    n_ads = {int((s["tags"] == 2).sum()) for s in sites}
    n_slab = [int((s["tags"] != 2).sum()) for s in sites]
    assert n_ads == {0, 1, 2, 5, 70} and min(n_slab) == 8 and max(n_slab) == 40
    assert any((s["cell"] != 0).all() for s in sites)                        # the fully skewed cell
    assert max(np.abs(s["pos"]).max() for s in sites) < 64
    # atoms that sit across a cell face from their counterpart
    assert any(np.abs((s["pos"].astype(np.float64) @ np.linalg.inv(s["cell"].astype(np.float64)))).max() > 0.99 for s in sites)
    for inc, pi in itertools.product((True, False), repeat=2):
        M, seam = H.case_distances(sites, inc, pi)
        H.assert_margins(M, seam, group, H.TOL, energy, 0.01)
        assert any(np.isinf(m).any() for m in M)
    M, _ = H.case_distances(sites)
    plain, _ = H.unique_sites(M, group, H.TOL)
    split, n_split = H.unique_sites(M, group, H.TOL, energy, 0.01)
    assert (plain == np.arange(len(sites))).sum() < n_split.sum() < len(sites)   # duplicates exist; the energy splits some


def test_c_entries_are_declared_and_exported():
    lib = L.load()
    header = (ROOT / "include" / "adsorbdiff_hip.h").read_text()
    for name in ("adf_site_pair_distances", "adf_unique_sites", "adf_select_top_sites"):
        assert name in L.EXPORTS and hasattr(lib, name) and f" {name}(" in header, name
    assert "unique.hip" in __import__("adsorbdiff_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "eval.py:765-777" in header
    assert lib.adf_site_pair_distances(None, None, None, None, None, None, None, 0, 0, 0, 0, 1, 1, None, None) == L.ADF_EINVAL
    assert b"site_pair_distances" in lib.adf_last_error()
    assert lib.adf_unique_sites(None, None, None, 0, 0, 0, None, None, C.c_float(0.05), C.c_float(-1), None, None, None) == L.ADF_EINVAL
    assert b"unique_sites" in lib.adf_last_error()
    assert lib.adf_select_top_sites(None, None, None, None, 1, 1, None, None, None) == L.ADF_EINVAL
    assert b"select_top_sites" in lib.adf_last_error()


def test_index_maps_between_the_callers_order_and_the_groups():
    rng = np.random.default_rng(6)
    group = torch.tensor(rng.choice([7, -3, 12], size=23))
    perm, offsets, ids = regroup(group)
    # representatives in the caller's indexing: every site points at the first site of its group, two are invalid
    first = {int(g): int((group == g).nonzero()[0]) for g in ids}
    rep = torch.tensor([first[int(g)] for g in group])
    rep[5] = rep[11] = -1
    moved = SS.to_group_order(rep, perm)
    assert moved.tolist() == [-1 if rep[p] < 0 else int(offsets[ids.tolist().index(int(group[p]))]) for p in perm.tolist()]
    assert torch.equal(SS.to_caller_order(moved, perm), rep[perm])
    back = torch.empty_like(rep)
    back[perm] = SS.to_caller_order(moved, perm)
    assert torch.equal(back, rep)
    top = torch.tensor([[0, 3, -1], [int(offsets[1]), -1, -1]], dtype=torch.int32)
    assert SS.to_caller_order(top, perm).tolist() == [[int(perm[0]), int(perm[3]), -1], [int(perm[int(offsets[1])]), -1, -1]]


def test_argument_errors_need_no_device():
    e, g = torch.zeros(4), torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError, match="4 energies, 3 group ids"):
        SS.top_sites(e, None, g[:3], 2)
    with pytest.raises(ValueError, match=r"expected \(4, 4\)"):
        SS.top_sites(e, torch.zeros(4, 3), g, 2)
    with pytest.raises(ValueError, match="representatives"):
        SS.top_sites(e, None, g, 2, rep=torch.zeros(5, dtype=torch.long))
    with pytest.raises(ValueError, match="at least one"):
        SS.top_sites(e, None, g, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SS.top_sites(e, None, g, 2)
    b = H.to_batch(H.chain_case())
    assert b.site_group.tolist() == [0, 0, 0] and b.natoms.tolist() == [9, 9, 9]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SS.site_distances(b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SS.unique_sites(b)
    with pytest.raises(ValueError, match="3 sites, 2 group ids"):
        SS.site_distances(b, group=[0, 1])
    with pytest.raises(ValueError, match="3 sites, 2 energies"):
        SS.unique_sites(b, energy=torch.zeros(2))
    with pytest.raises(ValueError, match=r"expected \(3, 4\)"):
        SS.unique_sites(b, flags=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="finite"):
        SS.unique_sites(b, tol=float("inf"))
    del b.site_group
    with pytest.raises(ValueError, match="site_group"):
        SS.unique_sites(b)
    with pytest.raises(ValueError, match="rank and world"):
        MR.ml_relax_unique(H.to_batch(H.chain_case()), None, 1, 0.05, {"memory": 5}, False, rank=0)


def test_ml_relax_unique_relaxes_representatives_and_copies_them(monkeypatch):
    """The plumbing alone (the clustering and the optimizer are stand-ins): one relaxation per representative, the whole batch
    back in input order through the out-of-memory split's reordering, duplicates carrying their representative's values."""
    sizes = []

    class StubLBFGS:
        def __init__(self, batch, calc, **kw):
            self.batch = batch

        def run(self, fmax, steps):
            n = len(self.batch.sid)
            if n > 2:
                raise RuntimeError("HIP out of memory")
            sizes.append(n)
            self.batch.pos += 1.0
            self.batch.y = torch.tensor([float(s) for s in self.batch.sid])
            self.batch.force = -self.batch.pos
            return self.batch

    rep = torch.tensor([0, 1, 0, 3, 3, 5])

    def fake_unique(batch, group=None, tol=0.05, **kw):
        assert tol == 0.07 and kw == {"include_slab": False}
        return rep, rep == torch.arange(6), torch.tensor([2, 2])

    from adsorbdiff_amd.synthetic import make_batch

    monkeypatch.setattr(MR, "LBFGS", StubLBFGS)
    monkeypatch.setattr(SS, "unique_sites", fake_unique)
    b = make_batch(6, n_slab=4, n_ads=1, seed=3)
    given = b.pos.clone()
    out = MR.ml_relax_unique(b, None, 5, 0.05, {"memory": 7}, False, tol=0.07, include_slab=False, device="cpu")
    assert sorted(sizes) == [2, 2]                                           # four systems relaxed, in two halves
    assert torch.equal(b.pos, given) and out.sid == b.sid and torch.equal(out.site_rep, rep)
    want = given.view(6, 5, 3)[rep].reshape(-1, 3) + 1.0
    assert torch.equal(out.pos, want) and torch.equal(out.force, -want)
    assert out.y.tolist() == [0.0, 1.0, 0.0, 3.0, 3.0, 5.0]
