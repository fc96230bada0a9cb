"""Host side of the per-system sampling mode: the stop rule's oracle, the numpy mirror of the keyed draws,
the parameter checks of Denoiser and ml_diffuse_sharded, and the keys a system carries through a split.  No GPU needed."""
import logging
from pathlib import Path

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.denoising_torch import Denoiser, per_system_stop_steps
from adsorbdiff_amd.ml_relaxation import ml_diffuse_sharded
from adsorbdiff_amd.synthetic import make_batch
from tests import helpers_sampler_keys as K
from tests.helpers_tr_only import reference_draws

NEW = ("adf_painn_set_per_system_stop", "adf_eqv2_set_per_system_stop", "adf_sampler_draws")


def test_new_symbols_are_declared_exported_and_reject_null():
    header = (Path(__file__).resolve().parent.parent / "include" / "adsorbdiff_hip.h").read_text()
    lib = L.load()
    for name in NEW:
        assert f"int32_t {name}(" in header and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.adf_painn_set_per_system_stop(None, None, 0) == L.ADF_EINVAL
    assert lib.adf_eqv2_set_per_system_stop(None, None, 0) == L.ADF_EINVAL
    assert lib.adf_sampler_draws(0, None, None, 4, 2, None, None, None, None) == L.ADF_EINVAL
    assert lib.adf_last_error()


def _table(T, cols):
    conv = torch.zeros(T, len(cols), dtype=torch.bool)
    for b, steps in enumerate(cols):
        conv[list(steps), b] = True
    return conv


@pytest.mark.parametrize("count", [10, 3, 1, 0])
def test_stop_rule_against_the_reference_loop_per_column(count):
    T = 14
    cols = [
        range(T - count, T) if count else [],      # the count is reached exactly at the last step
        range(0, max(count - 1, 0)),               # never reached: one short
        [0, 2, 3, 5, 8, 9, 10, 11, 12, 13],        # non-consecutive: the count is cumulative, not a run length
        range(T),                                  # converged from the start: stops at step count - 1
        [],                                        # never converged
        [1, 4, 5, 7, 8, 9, 10, 11, 12],            # nine scattered steps
    ]
    conv = _table(T, cols)
    steps, stop = per_system_stop_steps(conv, count)
    assert steps.dtype == torch.int64 and stop.dtype == torch.int64
    for b in range(len(cols)):
        want = K.reference_loop_one_system(conv[:, b].tolist(), count)
        assert (int(steps[b]), int(stop[b])) == want, (count, b)
    if count == 10:
        assert (int(steps[0]), int(stop[0])) == (T - 1, T - 1)     # the last step's update is the one not applied
        assert (int(steps[1]), int(stop[1])) == (T, -1)
        assert (int(steps[2]), int(stop[2])) == (13, 13)
        assert (int(steps[3]), int(stop[3])) == (9, 9)             # what sampler_ode_early.npz records: 9 of 40
    if count == 0:
        assert steps.tolist() == [T] * len(cols) and stop.tolist() == [-1] * len(cols)


def test_stop_rule_rejects_other_shapes():
    with pytest.raises(ValueError):
        per_system_stop_steps(torch.zeros(5, dtype=torch.bool))


def test_mirror_of_the_keyed_draws():
    seed, T = 0x1234_5678_9ABC_DEF0, 5
    keys = np.array([3, -7, 2**40 + 1, 3], dtype=np.int64)
    site = np.array([0, 0, 5, 1])
    place = K.place_draws(seed, keys, site)
    assert place.dtype == np.float32 and place.shape == (4, 3)
    assert float(place.min()) >= 0.0 and float(place.max()) < 1.0
    assert np.array_equal(place.astype(np.float64) * 2.0**24, np.round(place.astype(np.float64) * 2.0**24))  # exact in f32
    # the largest 24-bit word still lies below 1: (2^24 - 1) 2^-24
    assert np.float32((0xFFFFFFFF >> 8) * 2.0**-24) < np.float32(1.0)
    z = K.step_normals(seed, keys, site, T)
    assert z.shape == (T, 4, 6) and np.isfinite(z).all()
    # systems 0 and 3 share a key and differ in the site: other rows
    assert not np.array_equal(place[0], place[3]) and not np.array_equal(z[:, 0], z[:, 3])
    assert np.array_equal(K.place_draws(seed, keys[[3, 0]], site[[3, 0]]), place[[3, 0]])   # a function of (key, site) alone
    # site None = 0
    assert np.array_equal(K.place_draws(seed, keys[:2]), place[:2])
    # and none is a training row of the same (seed, key, step): last counter words 0 / 1 there, >= 4 here
    for t in range(T):
        train = reference_draws(seed, t, keys)[:, 1:7]
        assert not np.isclose(train, z[t]).any()
    # the steps differ, the seeds differ
    assert not np.array_equal(z[0], z[1])
    assert not np.array_equal(K.place_draws(seed + 1, keys, site), place)


class _Unwrapped:
    otf_graph = True


class _Trainer:
    _unwrapped_model = _Unwrapped()


class _Calc:
    model = _Trainer()


PARAMS = dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55)


def test_denoiser_rejects_per_system_with_graph_replay():
    with pytest.raises(ValueError, match="use_graph"):
        Denoiser(object(), _Calc(), dict(PARAMS, per_system=True, use_graph=True), device="cuda:0")
    Denoiser(object(), _Calc(), dict(PARAMS, per_system=True), device="cuda:0")


def test_denoiser_rejects_duplicate_key_and_site(caplog):
    b = make_batch(3, n_slab=8, n_ads=2, seed=1)
    b.noise_key = torch.tensor([5, 9, 5], dtype=torch.int64)
    with pytest.raises(ValueError, match="site_index"):
        Denoiser(b, _Calc(), dict(PARAMS, noise_seed=1), device="cuda:0")
    b.site_index = torch.tensor([0, 0, 1], dtype=torch.int32)       # the same slab twice, two sites: fine
    den = Denoiser(b, _Calc(), dict(PARAMS, noise_seed=1), device="cuda:0")
    assert den._noise_keys.tolist() == [5, 9, 5] and den._noise_site.tolist() == [0, 0, 1]
    b.site_index = torch.tensor([1, 0, 1], dtype=torch.int32)
    with pytest.raises(ValueError, match="site_index"):
        Denoiser(b, _Calc(), dict(PARAMS, noise_seed=1), device="cuda:0")
    # without noise_seed nothing is checked
    Denoiser(b, _Calc(), dict(PARAMS), device="cuda:0")
    # keys that are positions in the batch: one warning
    c = make_batch(2, n_slab=8, n_ads=2, seed=1)
    del c.__dict__["sid"]
    with caplog.at_level(logging.WARNING):
        Denoiser(c, _Calc(), dict(PARAMS, noise_seed=1), device="cuda:0")
    assert sum("batch-invariant" in r.getMessage() for r in caplog.records) == 1


@pytest.mark.parametrize("params,word", [
    (dict(noise_seed=1), "per_system"),                                                # coupled early stop
    (dict(per_system=True), "noise_seed"),                                             # torch.rand placement
    (dict(early_stop=False, placement_noise=torch.zeros(3, 3), ode=False), "noise_seed"),   # SDE normals from a stream
    (dict(early_stop=False, placement_noise=torch.zeros(3, 3), sampler="langevin", n_step_each=1, step_lr=1e-5),
     "noise_seed"),
])
def test_sharded_sampling_names_the_missing_condition(params, word):
    b = make_batch(3, n_slab=8, n_ads=2, seed=1)
    with pytest.raises(ValueError, match=word):
        ml_diffuse_sharded(b, object(), dict(PARAMS, **params), None, False, "cuda:0", 0, 1)


def test_sharded_sampling_checks_the_placement_table():
    b = make_batch(3, n_slab=8, n_ads=2, seed=1)
    with pytest.raises(ValueError, match="placement_noise"):
        ml_diffuse_sharded(b, object(), dict(PARAMS, early_stop=False, placement_noise=torch.zeros(2, 3)), None, False,
                           "cuda:0", 0, 1)


def test_a_rank_assembles_the_gathered_sites_and_marks_foreign_systems():
    """The post-gather assembly of ml_diffuse_sharded on one rank of three: adsorbate rows of EVERY system from the gathered
    sites (global order), sample_steps -1 / sample_stopped False for the systems sampled on other ranks; a rank that was
    dealt nothing gets the sites and no step counts."""
    from adsorbdiff_amd.ml_relaxation import assemble_sharded
    from adsorbdiff_amd.sampler import adsorbate_sites, merge_packed_sites, pack_sites, shard_batch, shard_bounds

    full = Batch.from_data_list(make_batch(3, n_slab=8, n_ads=2, seed=1).to_data_list()
                                + make_batch(2, n_slab=5, n_ads=3, seed=2, sid_offset=3).to_data_list())
    bounds = shard_bounds(full, 3)
    sampled, messages = {}, []
    for r in range(3):
        mine, ids = shard_batch(full, r, 3)
        mine = Batch.from_data_list(mine.to_data_list()[::-1])        # as after an out-of-memory split: another order
        ids = ids[::-1]
        mine.pos = mine.pos + 100.0 * (r + 1) * (mine.tags == 2).float()[:, None]     # "sampling": move the adsorbates
        mine.sample_steps = torch.tensor([10 * r + k for k in range(len(ids))])
        mine.sample_stopped = torch.ones(len(ids), dtype=torch.bool)
        sampled[r] = (mine, ids)
        messages.append(pack_sites(adsorbate_sites(mine), ids, bounds))
    sites = merge_packed_sites(torch.stack(messages), bounds[1])
    assert sites.shape[0] == 5 and bool(torch.isnan(sites).any())          # adsorbates of 2 and 3 atoms: NaN padding
    rank_of = {i: r for r, (_, ids) in sampled.items() for i in ids}
    for r, (mine, ids) in sampled.items():
        out = assemble_sharded(full, sites, mine, ids)
        assert out.sample_steps.tolist() == [mine.sample_steps[ids.index(i)].item() if i in ids else -1 for i in range(5)]
        assert out.sample_stopped.tolist() == [i in ids for i in range(5)]
        shift = torch.tensor([100.0 * (rank_of[int(b)] + 1) for b in full.batch])[:, None] * (full.tags == 2).float()[:, None]
        assert torch.equal(out.pos, full.pos + shift) and out.sid == full.sid
    empty = assemble_sharded(full, sites, None, [])
    assert torch.equal(empty.pos, out.pos) and "sample_steps" not in empty
    assert not torch.equal(full.pos, out.pos)                              # the input batch is not written


def test_a_system_keeps_its_keys_through_the_data_list():
    b = make_batch(3, n_slab=8, n_ads=2, seed=1)
    b.noise_key = torch.tensor([5, -9, 2**40], dtype=torch.int64)
    b.site_index = torch.tensor([0, 2, 1], dtype=torch.int32)
    b.sample_steps = torch.tensor([4, 40, 17], dtype=torch.int64)
    b.sample_stopped = torch.tensor([True, False, True])
    back = Batch.from_data_list(b.to_data_list())
    for k in ("noise_key", "site_index", "sample_steps", "sample_stopped"):
        assert torch.equal(getattr(back, k), getattr(b, k)) and getattr(back, k).dtype == getattr(b, k).dtype, k
    rev = Batch.from_data_list(b.to_data_list()[::-1])
    assert rev.noise_key.tolist() == [2**40, -9, 5] and rev.site_index.tolist() == [1, 2, 0]
    from adsorbdiff_amd.sampler import shard_batch

    mine, ids = shard_batch(b, 1, 2)
    assert torch.equal(mine.noise_key, b.noise_key[torch.tensor(ids)])
