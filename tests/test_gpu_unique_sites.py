"""GPU tests of the duplicate-site stage (csrc/unique.hip, adsorbdiff_amd/site_select.py, ml_relax_unique) against the float64
oracle of tests/helpers_unique_sites.py: distances within 5e-5 A, and - the generated cases keep clear of the 0.5 seam, of
``tol`` and of ``energy_tol``, which is asserted first - representatives, counts and rankings exactly."""
import functools
import itertools

import numpy as np
import pytest
import torch

from adsorbdiff_amd import flag_anomaly as FA
from adsorbdiff_amd import site_select as SS
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.ml_relaxation import ml_relax, ml_relax_unique
from adsorbdiff_amd.painn import PaiNN
from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_unique_sites as H
from tests.helpers import batch_from_fixture, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_TOL = 0.01
MODES = list(itertools.product((True, False), repeat=2))          # (include_slab, permutation_invariant)


@functools.lru_cache(maxsize=None)
def _main():
    sites, energy = H.main_case()
    return sites, energy, H.groups_of(sites), H.to_batch(sites, DEV)


@functools.lru_cache(maxsize=None)
def _oracle(include_slab, permutation_invariant):
    sites, energy, group, _ = _main()
    M, seam = H.case_distances(sites, include_slab, permutation_invariant)
    H.assert_margins(M, seam, group, H.TOL, energy, E_TOL)
    return M


def _t(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def _check_matrices(got, want):
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        g = g.cpu()
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32
        assert torch.equal(g, g.T) and bool((g.diagonal() == 0).all())
        inf = np.isinf(w)
        assert np.array_equal(np.isinf(g.numpy()), inf)
        if (~inf).any():
            worst = max(worst, float(np.abs(g.numpy().astype(np.float64)[~inf] - w[~inf]).max()))
    print("largest distance error", worst)
    assert worst <= H.DIST_ATOL, worst


@pytest.mark.parametrize("include_slab,permutation_invariant", MODES)
def test_distances_vs_oracle(include_slab, permutation_invariant):
    """Groups of 1, 2, 3 and 65 sites (and 2, 3, 4), adsorbates of 0, 1, 2 (flipped), 5 and 70 atoms, a fully skewed cell,
    duplicates across cell faces, members that cannot be compared, ids interleaved."""
    sites, _, group, batch = _main()
    want = _oracle(include_slab, permutation_invariant)
    got = SS.site_distances(batch, include_slab=include_slab, permutation_invariant=permutation_invariant)
    assert [m.shape[0] for m in got] == [2, 2, 1, 3, 65, 3, 4]
    _check_matrices(got, want)
    assert any(np.isinf(w).any() for w in want)
    # the group argument overrides batch.site_group: everything in one group is one 80 x 80 matrix
    if include_slab and permutation_invariant:
        one = SS.site_distances(batch, group=torch.zeros(len(sites), dtype=torch.long))
        assert len(one) == 1 and tuple(one[0].shape) == (80, 80) and torch.equal(one[0], one[0].T)
        members = H.regroup_numpy(group)[1][4]                    # the 65-site group is a block of it
        sub = one[0][_t(members)][:, _t(members)].cpu().numpy()
        assert np.abs(sub - want[4]).max() <= H.DIST_ATOL


def test_flipped_homonuclear_adsorbate_is_the_same_site():
    sites, _, group, batch = _main()
    k = H.regroup_numpy(group)[0].index(-3)
    assert float(SS.site_distances(batch)[k][0, 1]) < 0.4 * H.TOL + H.DIST_ATOL
    assert float(SS.site_distances(batch, permutation_invariant=False)[k][0, 1]) > 1.0


def _flags_and_nan(S, seed):
    rng = np.random.default_rng(seed)
    flags = np.zeros((S, 4), np.int64)
    bad = rng.choice(S, S // 8, replace=False)
    flags[bad, rng.integers(0, 4, len(bad))] = 1
    nan = rng.choice(S, S // 10, replace=False)
    return flags, nan


def _assert_unique(got, want):
    rep, is_rep, n_unique = got
    assert rep.dtype == torch.long and is_rep.dtype == torch.bool and n_unique.dtype == torch.long
    assert rep.cpu().tolist() == want[0].tolist()
    assert n_unique.cpu().tolist() == want[1].tolist()
    assert torch.equal(is_rep.cpu(), torch.from_numpy(want[0] == np.arange(len(want[0]))))


@pytest.mark.parametrize("include_slab,permutation_invariant", MODES)
def test_clustering_vs_oracle(include_slab, permutation_invariant):
    sites, energy, group, batch = _main()
    M = _oracle(include_slab, permutation_invariant)
    kw = dict(include_slab=include_slab, permutation_invariant=permutation_invariant)
    _assert_unique(SS.unique_sites(batch, tol=H.TOL, **kw), H.unique_sites(M, group, H.TOL))
    _assert_unique(SS.unique_sites(batch, tol=H.TOL, energy=_t(energy), **kw), H.unique_sites(M, group, H.TOL, energy))
    # the energy tolerance splits geometric clusters
    plain = H.unique_sites(M, group, H.TOL, energy)
    split = H.unique_sites(M, group, H.TOL, energy, E_TOL)
    assert split[1].sum() > plain[1].sum()
    _assert_unique(SS.unique_sites(batch, tol=H.TOL, energy=_t(energy), energy_tol=E_TOL, **kw), split)
    # flagged and NaN sites: never representatives, never merged
    flags, nan = _flags_and_nan(len(sites), 3)
    e = energy.copy()
    e[nan] = np.nan
    want = H.unique_sites(M, group, H.TOL, e, E_TOL, flags)
    assert (want[0] == -1).sum() >= len(nan) and (want[0][flags.any(1)] == -1).all()
    _assert_unique(SS.unique_sites(batch, tol=H.TOL, energy=_t(e), energy_tol=E_TOL, flags=_t(flags), **kw), want)
    _assert_unique(SS.unique_sites(batch, tol=H.TOL, flags=_t(flags) != 0, **kw), H.unique_sites(M, group, H.TOL, flags=flags))


def test_chain_is_cut_by_the_visiting_order():
    chain = H.chain_case()
    M, seam = H.case_distances(chain)
    H.assert_margins(M, seam, [0, 0, 0], H.TOL)
    b = H.to_batch(chain, DEV)
    rep, _, n = SS.unique_sites(b, tol=H.TOL)
    assert rep.tolist() == [0, 0, 2] and n.tolist() == [2]
    rep, _, n = SS.unique_sites(b, tol=H.TOL, energy=_t(np.float32([1, 0, 2])))
    assert rep.tolist() == [1, 1, 1] and n.tolist() == [1]
    rep, _, n = SS.unique_sites(b, tol=H.TOL, energy=_t(np.float32([1, 1, 1])))       # a tie: the caller's order
    assert rep.tolist() == [0, 0, 2]


def test_group_of_1100_sites():
    """More sites than a workgroup has threads, and more than 1024: the rank sort runs over several tiles."""
    sites, energy = H.large_case()
    group = H.groups_of(sites)
    M, seam = H.case_distances(sites)
    H.assert_margins(M, seam, group, H.TOL, energy, E_TOL)
    b = H.to_batch(sites, DEV)
    _check_matrices(SS.site_distances(b), M)
    want = H.unique_sites(M, group, H.TOL, energy, E_TOL)
    assert 400 < want[1][0] < 1100
    _assert_unique(SS.unique_sites(b, tol=H.TOL, energy=_t(energy), energy_tol=E_TOL), want)
    _assert_unique(SS.unique_sites(b, tol=H.TOL), H.unique_sites(M, group, H.TOL))
    top, top_e = SS.top_sites(_t(energy), None, _t(group), 5, rep=_t(want[0]))
    wt, we = H.top_sites(energy, None, group, 5, rep=want[0])
    assert top.cpu().tolist() == wt.tolist() and np.array_equal(top_e.cpu().numpy(), we.astype(np.float32))


def test_invariances_and_reproducibility():
    sites, energy, group, batch = _main()
    assert len(set(energy.tolist())) == len(energy)              # distinct energies: the visiting order is the energies'
    M = _oracle(True, True)
    whole = SS.unique_sites(batch, tol=H.TOL, energy=_t(energy), energy_tol=E_TOL)
    _assert_unique(whole, H.unique_sites(M, group, H.TOL, energy, E_TOL))
    # two identical calls: identical bits
    d1 = torch.cat([m.reshape(-1) for m in SS.site_distances(batch)])
    d2 = torch.cat([m.reshape(-1) for m in SS.site_distances(batch)])
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    again = SS.unique_sites(batch, tol=H.TOL, energy=_t(energy), energy_tol=E_TOL)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    # the sites permuted (inside their groups too): the same clusters after mapping the indices back
    P = np.random.default_rng(9).permutation(len(sites))
    moved = [sites[i] for i in P]
    Mp, seam = H.case_distances(moved)
    H.assert_margins(Mp, seam, group[P], H.TOL, energy[P], E_TOL)
    rep_p, _, n_p = SS.unique_sites(H.to_batch(moved, DEV), tol=H.TOL, energy=_t(energy[P]), energy_tol=E_TOL)
    back = np.empty(len(sites), np.int64)
    back[P] = P[rep_p.cpu().numpy()]
    assert back.tolist() == whole[0].cpu().tolist() and torch.equal(n_p, whole[2])
    # every group in a call of its own
    ids, members = H.regroup_numpy(group)
    for k, m in enumerate(members):
        rep_g, _, n_g = SS.unique_sites(H.to_batch([sites[i] for i in m], DEV), tol=H.TOL, energy=_t(energy[m]), energy_tol=E_TOL)
        assert m[rep_g.cpu().numpy()].tolist() == whole[0][_t(m)].cpu().tolist(), ids[k]
        assert int(n_g[0]) == int(whole[2][k])


@pytest.mark.parametrize("k", [1, 3, 70])
def test_top_sites_vs_oracle(k):
    sites, energy, group, batch = _main()
    S = len(sites)
    flags, nan = _flags_and_nan(S, 4)
    e = energy.copy()
    e[nan] = np.nan
    members = H.regroup_numpy(group)[1][4]
    e[members[10:16]] = e[members[3]]                            # exact ties inside the 65-site group
    rep = H.unique_sites(_oracle(True, True), group, H.TOL, e, None, flags)[0]
    assert k != 70 or k > max(len(m) for m in H.regroup_numpy(group)[1])
    for f, r in ((flags, None), (None, None), (flags, rep), (None, rep)):
        top, top_e = SS.top_sites(_t(e), None if f is None else _t(f), _t(group), k, rep=None if r is None else _t(r))
        wt, we = H.top_sites(e, f, group, k, rep=r)
        assert top.dtype == torch.long and tuple(top.shape) == (7, k)
        assert top.cpu().tolist() == wt.tolist()
        assert np.array_equal(top_e.cpu().numpy(), we.astype(np.float32))
        if r is None:
            best, best_e, _ = FA.best_sites(_t(e), None if f is None else _t(f), _t(group))
            assert torch.equal(top[:, 0], best) and torch.equal(top_e[:, 0], best_e)
    assert (wt == -1).any() if k > 1 else True


# ------------------------------------------------------------------------------------------------------ ml_relax_unique
HP_SMALL = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES_SMALL = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}


class _Counting:
    """A trainer that records the size of every batch it is shown and does not fit more than ``most`` systems."""

    def __init__(self, tr, most=None):
        self.tr, self._unwrapped_model, self.most, self.sizes, self.refused = tr, tr._unwrapped_model, most, [], 0

    def predict(self, batch, per_image=False, disable_tqdm=True):
        n = int(batch.natoms.shape[0])
        if self.most is not None and n > self.most:
            self.refused += 1
            raise RuntimeError("HIP out of memory (stand-in)")
        self.sizes.append(n)
        return self.tr.predict(batch, per_image=per_image, disable_tqdm=disable_tqdm)


@pytest.fixture(scope="module")
def relax_setup():
    """The small S2EF PaiNN of the per-system relaxation tests; 2 groups x 3 sites out of the four relax_run.npz systems: group
    0 = (system 0, a shifted copy of it, system 1), group 1 = (system 2, system 3, a shifted copy of system 3)."""
    fx = load_npz("relax_run.npz")
    torch.manual_seed(int(fx["seed"]))
    model = PaiNN(None, 50, 1, scale_file=dict(SCALES_SMALL), **HP_SMALL).to(DEV).eval()
    tr = ForcesTrainer(model, device=DEV)
    base = batch_from_fixture(fx, pos_key="pos_in").to_data_list()
    shift = torch.tensor([0.012, -0.009, 0.006])                # 0.016 A: a third of tol
    systems = []
    for i in (0, 0, 1, 2, 3, 3):
        d = base[i].clone()
        if len(systems) in (1, 5):
            d.pos = d.pos + shift
        d.sid = str(len(systems))
        systems.append(d)
    group = [0, 0, 0, 1, 1, 1]
    sites = [{"pos": d.pos.numpy().astype(np.float32), "tags": d.tags.numpy(), "Z": d.atomic_numbers.long().numpy(),
              "cell": d.cell.reshape(3, 3).numpy().astype(np.float32), "group": g} for d, g in zip(systems, group)]
    M, seam = H.case_distances(sites)
    H.assert_margins(M, seam, group, H.TOL)
    want_rep, want_n = H.unique_sites(M, group, H.TOL)
    assert want_rep.tolist() == [0, 0, 2, 3, 4, 4] and want_n.tolist() == [2, 2]
    opt = {"memory": int(fx["memory"]), "per_system": True}
    args = dict(steps=int(fx["steps"]), fmax=float(fx["fmax"]), relax_opt=opt, save_full_traj=False, device=DEV)
    reps = [0, 2, 3, 4]
    alone = ml_relax(Batch.from_data_list([systems[i].clone() for i in reps]).to(DEV), tr, **args)
    assert alone.sid == ["0", "2", "3", "4"]
    return systems, group, want_rep, tr, args, alone


def _check_relaxed(out, systems, want_rep, alone):
    assert out.sid == [str(i) for i in range(6)] and out.natoms.tolist() == [24] * 6          # input order
    assert out.site_rep.cpu().tolist() == want_rep.tolist()
    slot = {0: 0, 2: 1, 3: 2, 4: 3}
    pos, force, ref_pos, ref_force = (t.view(-1, 24, 3) for t in (out.pos, out.force, alone.pos, alone.force))
    for s in range(6):
        r = slot[int(want_rep[s])]                               # representatives: bit-equal to their own relaxation alone;
        assert torch.equal(pos[s], ref_pos[r]), s                # duplicates: their representative's values
        assert torch.equal(force[s], ref_force[r]) and torch.equal(out.y[s], alone.y[r]), s
    given = torch.cat([d.pos for d in systems]).view(6, 24, 3).to(DEV)
    assert not torch.equal(pos[0], given[0])                     # something was relaxed


def test_ml_relax_unique_relaxes_one_site_per_cluster(relax_setup):
    systems, group, want_rep, tr, args, alone = relax_setup
    batch = Batch.from_data_list([d.clone() for d in systems]).to(DEV)
    given = batch.pos.clone()
    counting = _Counting(tr)
    out = ml_relax_unique(batch, counting, group=torch.tensor(group), tol=H.TOL, **args)
    assert counting.sizes and set(counting.sizes) == {4}         # four systems in every forward, not six
    assert torch.equal(batch.pos, given)                         # the caller's batch is left alone
    _check_relaxed(out, systems, want_rep, alone)
    # batch.site_group is the default grouping
    batch.site_group = torch.tensor(group)
    again = ml_relax_unique(batch, tr, tol=H.TOL, **args)
    assert torch.equal(again.pos, out.pos) and torch.equal(again.site_rep, out.site_rep)


def test_ml_relax_unique_through_the_out_of_memory_split(relax_setup):
    systems, group, want_rep, tr, args, alone = relax_setup
    batch = Batch.from_data_list([d.clone() for d in systems]).to(DEV)
    small = _Counting(tr, most=2)
    out = ml_relax_unique(batch, small, group=torch.tensor(group), tol=H.TOL, **args)
    assert small.refused == 1 and set(small.sizes) == {2}
    _check_relaxed(out, systems, want_rep, alone)
