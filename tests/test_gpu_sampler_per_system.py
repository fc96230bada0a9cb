"""GPU tests of the per-system sampling mode: a system's own early stop (csrc/stepper.hip,
adf_*_set_per_system_stop), the keyed draws (csrc/noising.hip, adf_sampler_draws) and what follows from the two: the same
bits for a system alone, in any batch, in any order, after ml_diffuse's split and on any shard.

Model: the stepper fixtures' small PaiNN (stepper_ode8.npz: H = 128, 2 layers, 4 systems x 40 atoms) with a head gain at
which the systems stop at different steps below T (asserted, so that no identity holds vacuously).  The comparisons are
bit tests: the per-system kernel and the coupled kernels share their arithmetic as device functions."""
import numpy as np
import pytest
import torch

import adsorbdiff_amd.ml_relaxation as R
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc, per_system_stop_steps
from adsorbdiff_amd.engine import image_repeats, sampler_draws
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.sampler import adsorbate_sites, merge_packed_sites, pack_sites, shard_batch, shard_bounds
from adsorbdiff_amd.trainer import DenoisingTrainer
from tests import helpers_sampler_keys as K
from tests.helpers import batch_from_fixture, load_npz, state_dict_from_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
T = 40
GAIN = 1.0          # head gain of the early-stop tests: chosen so that the preconditions of test 2 hold (asserted there)
EQV2_GAIN = 1.0     # scale of the EquiformerV2 force blocks' last projection, likewise
PARAMS = dict(num_steps=T, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True)
KEYS = [1101, -2202, 2**41 + 3, 4404]
SEED = 20240607


def _model(gain=GAIN):
    """tests/test_gpu_samplers._model: the small PaiNN of stepper_ode8.npz with its two heads' last layer scaled."""
    sd = state_dict_from_fixture(load_npz("stepper_ode8.npz"))
    for head in ("out_forces", "out_forces2"):
        sd[f"{head}.output_network.1.update_net.2.weight"].mul_(gain)
        sd[f"{head}.output_network.1.update_net.2.bias"].mul_(gain)
    m = PaiNN(None, 50, 1, scale_file=dict(SCALES), so3_denoising=True, **HP)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert set(missing) <= {"atom_radii"} and not unexpected, (missing, unexpected)
    return m.to(DEV).eval()


_CACHE = {}


def _trainer(gain=GAIN):
    if ("trainer", gain) not in _CACHE:
        _CACHE[("trainer", gain)] = DenoisingTrainer(_model(gain), device=DEV)
    return _CACHE[("trainer", gain)]


def _batch():
    b = batch_from_fixture(load_npz("stepper_ode8.npz"), pos_key="pos_in")
    b.sid = [f"s{i}" for i in range(4)]
    b.noise_key = torch.tensor(KEYS, dtype=torch.int64)
    return b


PLACE = torch.rand(4, 3, generator=torch.Generator().manual_seed(11))


def _pick(b, ids):
    systems = b.to_data_list()
    return Batch.from_data_list([systems[i] for i in ids])


def _run(b, params, trainer=None, **kw):
    den = Denoiser(b, DiffTorchCalc(trainer or _trainer()), params, device=DEV, traj_names=b.sid, **kw)
    out = den.run()
    return out, den


def _rows(b, i):
    off = np.concatenate([[0], np.cumsum(b.natoms.cpu().numpy())])
    return slice(int(off[i]), int(off[i + 1]))


def _alone(sampler):
    """Every system of the fixture sampled alone with the DEFAULT (coupled) rule: at B = 1 that is the reference's own
    semantics (pinned by sampler_ode_early.npz and the stepper_* fixtures).  Computed once per sampler."""
    if ("alone", sampler) not in _CACHE:
        runs = []
        for i in range(4):
            out, den = _run(_pick(_batch(), [i]), dict(PARAMS, sampler=sampler, placement_noise=PLACE[i:i + 1]))
            runs.append((out.pos.cpu(), den.steps_applied))
        _CACHE[("alone", sampler)] = runs
    return _CACHE[("alone", sampler)]


# ---------------------------------------------------------------------------------------------------------------- 1. draws
def test_keyed_draws_equal_the_numpy_mirror_and_follow_their_keys():
    keys = torch.tensor([3, -7, 2**40 + 1, 3, 0, 2**63 - 1, -2**63] + list(range(100, 193)), dtype=torch.int64)   # 100: > 1 wave
    site = torch.zeros(100, dtype=torch.int32)
    site[3], site[4] = 1, 2**30 - 1
    Ts = 7
    place, za, zb = (t.cpu().numpy() for t in sampler_draws(SEED, keys, site, Ts, DEV, place=True, z_a=True, z_b=True))
    assert np.array_equal(place, K.place_draws(SEED, keys.numpy(), site.numpy()))     # integer arithmetic: exactly equal
    assert float(place.min()) >= 0.0 and float(place.max()) < 1.0
    want = K.step_normals(SEED, keys.numpy(), site.numpy(), Ts)
    got = np.concatenate([za, zb], axis=-1)
    # double log / cos / sin may differ in their last bits before the cast to float32, nothing more: one float32 ulp
    w32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(w32))
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    print("keyed draws: max error in ulp", float((err / ulp).max()), "rows differing", int((err > 0).sum()))
    assert (err <= ulp).all()
    # permuting, splitting and isolating the key list gives equal bits
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(5))
    p2, a2, b2 = sampler_draws(SEED, keys[perm], site[perm], Ts, DEV, place=True, z_a=True, z_b=True)
    assert np.array_equal(p2.cpu().numpy(), place[perm]) and np.array_equal(a2.cpu().numpy(), za[:, perm])
    assert np.array_equal(b2.cpu().numpy(), zb[:, perm])
    p3, a3, _ = sampler_draws(SEED, keys[37:], site[37:], Ts, DEV, place=True, z_a=True)
    assert np.array_equal(p3.cpu().numpy(), place[37:]) and np.array_equal(a3.cpu().numpy(), za[:, 37:])
    p4, a4, b4 = sampler_draws(SEED, keys[3:4], site[3:4], Ts, DEV, place=True, z_a=True, z_b=True)
    assert np.array_equal(p4.cpu().numpy(), place[3:4]) and np.array_equal(a4.cpu().numpy(), za[:, 3:4])
    assert np.array_equal(b4.cpu().numpy(), zb[:, 3:4])
    # site None = 0; the same key at another site draws other rows
    p5, _, _ = sampler_draws(SEED, keys[:3], None, 0, DEV, place=True)
    assert np.array_equal(p5.cpu().numpy(), place[:3])
    assert not np.array_equal(place[0], place[3]) and not np.array_equal(za[:, 0], za[:, 3])
    # a site outside [0, 2^30) is refused
    with pytest.raises(ValueError):
        sampler_draws(SEED, keys[:2], torch.tensor([0, 2**30], dtype=torch.int32), 2, DEV)
    with pytest.raises(ValueError):
        sampler_draws(SEED, keys[:2], torch.tensor([-1, 0], dtype=torch.int32), 2, DEV)


# ------------------------------------------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("path", ["fused", "per_step"])
@pytest.mark.parametrize("sampler", ["sde_rot", "sde"])
def test_a_system_in_a_batch_equals_the_system_alone(sampler, path):
    alone = _alone(sampler)
    stops = [s for _, s in alone]
    print(sampler, path, "steps applied alone:", stops)
    # preconditions: the systems stop at different steps, one of them before the end ...
    assert len(set(stops)) >= 2 and min(stops) < T, stops
    # ... and the coupled default on the same batch goes on after the earliest of them has stopped
    b0 = _batch()
    _, coupled = _run(_batch(), dict(PARAMS, sampler=sampler, placement_noise=PLACE))
    assert coupled.steps_applied > min(stops), (coupled.steps_applied, stops)
    extra = dict(step_hook=lambda t: None) if path == "per_step" else {}
    out, den = _run(_batch(), dict(PARAMS, sampler=sampler, placement_noise=PLACE, per_system=True, **extra))
    pos = out.pos.cpu()
    assert out.sample_steps.dtype == torch.int64 and out.sample_steps.tolist() == stops
    assert out.sample_stopped.tolist() == [s < T for s in stops]
    assert den.steps_applied == max(stops)
    assert den.stop_step.tolist() == [s if s < T else -1 for s in stops]
    assert den.cvg_count == sum(s < T for s in stops)          # state[0]: the number of stopped systems
    for i in range(4):
        assert torch.equal(pos[_rows(b0, i)], alone[i][0]), (sampler, path, i)
    slab = b0.tags != 2
    assert torch.equal(pos[slab], b0.pos[slab])                 # slab rows never written


# ------------------------------------------------------------------------------------------------- 3. frozen means untouched
def test_a_stopped_system_is_bit_frozen_at_every_later_step():
    b = _batch()
    frames = []
    den = Denoiser(b, DiffTorchCalc(_trainer()), dict(PARAMS, placement_noise=PLACE, per_system=True,
                                                      step_hook=lambda t: frames.append(b.pos.clone())),
                   device=DEV, traj_names=b.sid)
    den.run()
    stop = den.stop_step.tolist()
    assert any(s >= 0 for s in stop)
    checked = 0
    for i, s in enumerate(stop):
        if s < 0:
            continue
        r = _rows(b, i)
        if s > 0:   # the step that stops a system does not move it (the reference's break before the update)
            assert torch.equal(frames[s][r], frames[s - 1][r]), i
        for t in range(s + 1, len(frames)):
            assert torch.equal(frames[t][r], frames[s][r]), (i, t)
            checked += 1
        if s > 1:   # and it did move before
            assert not torch.equal(frames[s - 1][r], frames[0][r]), i
    assert checked > 0
    assert torch.equal(frames[-1], b.pos)


def test_stop_steps_follow_the_host_rule_from_the_recorded_increments():
    """The per-step entry's dcom output rows: the predicate of every step and system, fed to per_system_stop_steps; rows of
    a stopped system are 0 from its stop on."""
    m = _trainer()._unwrapped_model
    eng = m.engine(torch.device(DEV))
    eng.set_moving_atoms(None, None)
    eng.set_incremental(False)
    b = _batch().to(DEV)
    prep = eng.prepare(b)
    pos = b.pos.clone().contiguous()
    from adsorbdiff_amd.denoising_torch import schedule_coefs

    coefs = schedule_coefs(PARAMS)
    coefs_dev = torch.tensor([[c.coef_tr, c.rot_pre, c.rot_dt, c.rot_g2, c.noise_tr, c.noise_rot] for c in coefs],
                             dtype=torch.float32, device=DEV)
    eng.init_placement(prep, pos, PLACE.to(DEV))
    state = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    sys_state = torch.tensor([[0, 0, 0, -1]] * 4, dtype=torch.int32, device=DEV)
    f1, f2 = torch.zeros(160, 3, device=DEV), torch.zeros(160, 3, device=DEV)
    dcom, drot = torch.empty(4, 3, device=DEV), torch.empty(4, 3, device=DEV)
    eng.set_per_system_stop(sys_state)
    try:
        conv, rows = [], []
        for t in range(T):
            eng.forward_prepared(prep, pos, f1, f2)
            eng._sde_step(prep, pos, f1, f2, None, coefs_dev, T, state, None, None, 10, dcom, drot)
            conv.append((dcom.abs() <= 1e-3).all(1).cpu())
            rows.append((dcom.clone().cpu(), drot.clone().cpu()))
        # a batch of another size is refused while the mode is set
        one = _pick(_batch(), [0]).to(DEV)
        p1 = eng.prepare(one)
        with pytest.raises(ValueError, match="per-system"):
            eng._sde_step(p1, one.pos.clone(), f1, f2, None, coefs_dev, T, state, None, None, 10, None, None)
    finally:
        eng.set_per_system_stop(None)
    got = sys_state.cpu()
    conv = torch.stack(conv)
    # a stopped system's later rows are zeros, which read as "converged": the rule only looks at the rows up to the stop
    steps, stop = per_system_stop_steps(conv, 10)
    assert got[:, 2].tolist() == steps.tolist() and got[:, 3].tolist() == stop.tolist()
    assert got[:, 1].tolist() == [int(s >= 0) for s in stop.tolist()]
    st = state.tolist()
    assert st[0] == int((stop >= 0).sum()) and st[1] == int(bool((stop >= 0).all())) and st[3] == int(steps.max()) and st[4] == T
    for t in range(1, T):
        for i in range(4):
            if 0 <= int(stop[i]) < t:
                assert float(rows[t][0][i].abs().max()) == 0.0 and float(rows[t][1][i].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- 4. keyed SDE and Langevin noise
def _keyed(sampler, seed=SEED):
    p = dict(PARAMS, sampler=sampler, ode=False, noise_seed=seed, per_system=True)
    if sampler == "langevin":
        p.update(num_steps=3, n_step_each=2, step_lr=1e-5)
    return p


@pytest.mark.parametrize("path", ["fused", "per_step"])
@pytest.mark.parametrize("sampler", ["sde_rot", "langevin"])
def test_keyed_noise_gives_a_system_the_same_bits_anywhere(sampler, path):
    extra = dict(step_hook=lambda t: None) if path == "per_step" else {}
    params = dict(_keyed(sampler), **extra)
    b0 = _batch()
    whole, den = _run(_batch(), params)
    whole = whole.pos.cpu()
    order = [2, 0, 3, 1]
    permuted, _ = _run(_pick(_batch(), order), params)
    for k, i in enumerate(order):
        assert torch.equal(permuted.pos.cpu()[_rows(b0, k)], whole[_rows(b0, i)]), (sampler, path, "permuted", i)
    for i in range(4):
        alone, d1 = _run(_pick(_batch(), [i]), params)
        assert torch.equal(alone.pos.cpu(), whole[_rows(b0, i)]), (sampler, path, "alone", i)
        assert int(alone.sample_steps[0]) == int(den.batch.sample_steps[i])
    other, _ = _run(_batch(), dict(params, noise_seed=SEED + 1))
    ads = b0.tags == 2
    assert float((other.pos.cpu()[ads] - whole[ads]).abs().max()) > 1e-2
    if sampler == "langevin":   # no stop there: only the attributes appear
        assert den.batch.sample_steps.tolist() == [6] * 4 and not den.batch.sample_stopped.any()


# ------------------------------------------------------------------------------------------------------------------ 5. split
class _TwoAtMost(Denoiser):
    """A sampler that does not fit more than two systems (ml_diffuse then samples the halves)."""
    refused = 0

    def run(self):
        if int(self.batch.natoms.shape[0]) > 2:
            _TwoAtMost.refused += 1
            raise RuntimeError("HIP out of memory (stand-in)")
        return super().run()


def test_the_out_of_memory_split_reproduces_the_unsplit_run(monkeypatch):
    params = dict(PARAMS, ode=False, noise_seed=SEED, per_system=True)     # early stop on
    whole = R.ml_diffuse(_batch(), _trainer(), params, None, False, device=DEV)
    monkeypatch.setattr(R, "Denoiser", _TwoAtMost)
    _TwoAtMost.refused = 0
    split = R.ml_diffuse(_batch(), _trainer(), params, None, False, device=DEV)
    order = [int(s[1:]) for s in split.sid]
    assert _TwoAtMost.refused == 1 and order == [2, 3, 0, 1]    # the reference's order: the upper half first
    b0 = _batch()
    for k, i in enumerate(order):
        assert torch.equal(split.pos.cpu()[_rows(b0, k)], whole.pos.cpu()[_rows(b0, i)]), i
    assert split.sample_steps.tolist() == [int(whole.sample_steps[i]) for i in order]
    assert split.sample_stopped.tolist() == [bool(whole.sample_stopped[i]) for i in order]
    assert split.noise_key.tolist() == [KEYS[i] for i in order]


# ----------------------------------------------------------------------------------------------------------------- 6. shards
@pytest.mark.parametrize("noise", ["keyed_sde", "table_ode"])
def test_shards_reproduce_the_single_run(noise):
    params = dict(PARAMS, per_system=True)
    params.update(dict(ode=False, noise_seed=SEED) if noise == "keyed_sde" else dict(placement_noise=PLACE))
    full = _uneven_batch()                                   # uneven shards: system 1 has lost two slab atoms
    assert full.natoms.tolist() == [40, 38, 40, 40] and full.noise_key.tolist() == KEYS
    single = R.ml_diffuse(full.clone(), _trainer(), params, None, False, device=DEV)
    want = adsorbate_sites(single).cpu()
    bounds = shard_bounds(full, 3)
    # The number of periodic images the graph search tries is the largest need over a batch - the one input a system's graph
    # takes from its batch-mates.  Here the shards differ in it (system 3 has the smallest cell), so the shards pin the
    # count of the whole batch, as ml_diffuse_sharded does; ml_diffuse pinned it for the single run.
    reps = image_repeats(full, HP["cutoff"])
    assert reps == [2, 2, 1] and image_repeats(shard_batch(full, 0, 3)[0], HP["cutoff"]) == [1, 1, 1]
    messages, seen = [], []
    for r in range(3):
        mine, ids = shard_batch(full, r, 3)
        seen += ids
        p = dict(params, image_repeats=reps)
        if noise == "table_ode":
            p["placement_noise"] = PLACE[torch.tensor(ids)]
        local = R.ml_diffuse(mine, _trainer(), p, None, False, device=DEV)
        messages.append(pack_sites(adsorbate_sites(local), ids, bounds).cpu())
    assert sorted(seen) == [0, 1, 2, 3]
    merged = merge_packed_sites(torch.stack(messages), bounds[1])
    assert torch.equal(merged, want)
    out = R.ml_diffuse_sharded(full.clone(), _trainer(), params, None, False, DEV, 0, 1)
    assert torch.equal(out.pos.cpu(), single.pos.cpu())
    assert out.sample_steps.tolist() == single.sample_steps.tolist()
    assert torch.equal(out.noise_key.cpu(), full.noise_key)


def _uneven_batch():
    """The fixture's batch with two slab atoms of system 1 removed: system 1 alone, or with systems 0 and 2, needs [1, 1, 1]
    periodic images; any batch that holds system 3 (the smallest cell) needs [2, 2, 1]."""
    systems = _batch().to_data_list()
    keep = torch.ones(40, dtype=torch.bool)
    keep[[3, 7]] = False
    for k in ("pos", "atomic_numbers", "tags", "fixed"):
        setattr(systems[1], k, getattr(systems[1], k)[keep])
    return Batch.from_data_list(systems)


def test_alone_equals_the_batch_where_the_image_counts_differ_once_they_are_pinned():
    """The periodic-image count of the graph search is a maximum over the batch.  In this batch it matters: with keyed SDE
    noise an adsorbate atom of system 1 leaves its cell and gains a neighbour through the extra image.  With the count of the
    whole batch pinned (``image_repeats``), every system alone gives the bits it gives in the batch."""
    full = _uneven_batch()
    reps = image_repeats(full, HP["cutoff"])
    assert reps == [2, 2, 1] and image_repeats(_pick(full, [1]), HP["cutoff"]) == [1, 1, 1]
    params = dict(PARAMS, ode=False, noise_seed=SEED, per_system=True)
    whole, den = _run(full.clone(), params)
    whole = whole.pos.cpu()
    for i in range(4):
        alone, _ = _run(_pick(full, [i]), dict(params, image_repeats=reps))
        assert torch.equal(alone.pos.cpu(), whole[_rows(full, i)]), i
        assert int(alone.sample_steps[0]) == int(den.batch.sample_steps[i])
    unpinned, _ = _run(_pick(full, [1]), params)
    print("system 1 alone without the pin: max |diff| to the batch",
          float((unpinned.pos.cpu() - whole[_rows(full, 1)]).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- 7. n sites
def test_n_sites_per_slab_in_one_batch():
    from adsorbdiff_amd.placement import place_adsorbates
    from adsorbdiff_amd.synthetic import make_batch
    from tests import helpers_placement as H

    src = make_batch(2, n_slab=36, n_ads=4, seed=31)
    slabs, ads, tris = [], [], []
    for d in src.to_data_list():
        s = d.tags != 2
        slabs.append(dict(pos=d.pos[s].numpy(), Z=d.atomic_numbers[s].long().numpy(), tags=d.tags[s].numpy(),
                          fixed=d.fixed[s].numpy(), cell=d.cell[0].numpy()))
        ads.append((d.atomic_numbers[~s].long().numpy(), d.pos[~s].numpy()))
        tris.append(H.lattice_triangles(d.cell[0].numpy(), 2, float(d.pos[s][:, 2].max()), ring=0))
    sb = H.slab_batch(slabs, device=DEV)
    placed = place_adsorbates(sb, ads, 3, radii=H.synthetic_radii(), masses=H.synthetic_masses(), triangles=tris, seed=9)
    assert placed.site_index.dtype == torch.int32 and placed.site_index.tolist() == [0, 1, 2, 0, 1, 2]
    assert placed.site_group.tolist() == [0, 0, 0, 1, 1, 1] and list(placed.sid) == ["slab0"] * 3 + ["slab1"] * 3
    params = dict(PARAMS, num_steps=8, noise_seed=SEED, per_system=True)
    tr = _trainer(20.0)      # strong heads: eight steps move the adsorbates visibly
    out = R.ml_diffuse(placed.clone(), tr, params, None, False, device=DEV)
    sites = adsorbate_sites(out).cpu()
    for g in (0, 3):
        for i in range(g, g + 3):
            for j in range(i + 1, g + 3):
                assert float((sites[i] - sites[j]).abs().max()) > 1e-2, (i, j)      # pairwise different sites within a slab
    rev = R.ml_diffuse(Batch.from_data_list(placed.clone().to_data_list()[::-1]), tr, params, None, False, device=DEV)
    assert rev.site_index.tolist() == [2, 1, 0, 2, 1, 0]
    assert torch.equal(adsorbate_sites(rev).cpu(), sites.flip(0))                    # the same bits per (sid, site_index)
    assert rev.sample_steps.tolist() == out.sample_steps.tolist()[::-1]
    # without the site index the replicas of a slab cannot be told apart
    bad = placed.clone()
    del bad.__dict__["site_index"]
    with pytest.raises(ValueError, match="site_index"):
        R.ml_diffuse(bad, tr, params, None, False, device=DEV)


# ----------------------------------------------------------------------------------------------------------- 8. trajectories
@pytest.mark.parametrize("path", ["fused", "per_step"])
def test_a_systems_trajectory_file_holds_its_own_frames(tmp_path, path):
    extra = dict(step_hook=lambda t: None) if path == "per_step" else {}
    params = dict(PARAMS, placement_noise=PLACE, per_system=True, **extra)
    b = _batch()
    out, den = _run(b, params, traj_dir=tmp_path / "batch")
    steps = out.sample_steps.tolist()
    assert min(steps) < max(steps)
    for i in range(4):
        one = _pick(_batch(), [i])
        _run(one, dict(params, per_system=False, placement_noise=PLACE[i:i + 1]), traj_dir=tmp_path / f"alone{i}")
        got = np.load(tmp_path / "batch" / f"s{i}.npz")
        want = np.load(tmp_path / f"alone{i}" / f"s{i}.npz")
        assert got["positions"].shape[0] == max(steps[i], 1), (i, got["positions"].shape, steps)
        for k in want.files:
            assert np.array_equal(got[k], want[k]), (i, k)
        assert np.array_equal(got["positions"][-1], out.pos.cpu().numpy()[_rows(b, i)])
    if path == "fused":   # the batch file keeps every frame
        assert np.load(tmp_path / "batch" / "batch_s0.frames.npy").shape[0] >= max(steps)


# ----------------------------------------------------------------------------------------------------------- 10. EquiformerV2
def _eqv2_trainer():
    from tests.test_gpu_eqv2 import model_from_fixture

    if "eqv2" not in _CACHE:
        m = model_from_fixture(load_npz("eqv2_l4m2.npz"))
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.startswith(("force_block.proj.", "force_block2.proj.")):
                    p.mul_(EQV2_GAIN)
        _CACHE["eqv2"] = DenoisingTrainer(m, device=DEV)
    return _CACHE["eqv2"]


def _eqv2_batch():
    two = batch_from_fixture(load_npz("eqv2_l4m2.npz")).to_data_list()
    b = Batch.from_data_list([two[0], two[1], two[0].clone()])
    b.sid = ["e0", "e1", "e2"]
    b.noise_key = torch.tensor([7, 8, 9], dtype=torch.int64)
    return b


def test_eqv2_system_in_a_batch_equals_the_system_alone():
    tr = _eqv2_trainer()
    place = torch.rand(3, 3, generator=torch.Generator().manual_seed(12))
    b0 = _eqv2_batch()
    alone = []
    for i in range(3):
        out, den = _run(_pick(_eqv2_batch(), [i]), dict(PARAMS, placement_noise=place[i:i + 1]), trainer=tr)
        alone.append((out.pos.cpu(), den.steps_applied))
    stops = [s for _, s in alone]
    print("eqv2 steps applied alone:", stops)
    assert min(stops) < T, stops
    out, den = _run(_eqv2_batch(), dict(PARAMS, placement_noise=place, per_system=True), trainer=tr)
    assert out.sample_steps.tolist() == stops and den.steps_applied == max(stops)
    for i in range(3):
        assert torch.equal(out.pos.cpu()[_rows(b0, i)], alone[i][0]), i
    slab = b0.tags != 2
    assert torch.equal(out.pos.cpu()[slab], b0.pos[slab])
