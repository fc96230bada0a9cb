"""GPU tests of "two half-batches, two streams" (the header's section of that name; csrc/stepper.hip sample_loop_split):
a sampling run whose two sides of a cut run on two handles and two streams has the bits of the one-stream run.

Two engines are built from one state dict (the stepper fixtures' small PaiNN: H = 128, 2 layers): `split` runs every case
with split_streams=True, `plain` with False, from the same placement uniforms and noise.  Every comparison is torch.equal: nothing
is compared against a tolerance."""
import pytest
import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc, schedule_coefs
from adsorbdiff_amd.engine import cell_repeats
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.synthetic import make_system
from adsorbdiff_amd.trainer import DenoisingTrainer
from tests.helpers import batch_from_fixture, load_npz, state_dict_from_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
PARAMS = dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True)
RAGGED = {2: (31, 33), 3: (31, 65, 290), 5: (33, 64, 65, 97, 31)}
_CACHE = {}


def _model():
    sd = state_dict_from_fixture(load_npz("stepper_ode8.npz"))
    m = PaiNN(None, 50, 1, scale_file=dict(SCALES), so3_denoising=True, **HP)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert set(missing) <= {"atom_radii"} and not unexpected, (missing, unexpected)
    return m.to(DEV).eval()


def _engines():
    """(split, plain): two models from one state dict, each with its own engine."""
    if "models" not in _CACHE:
        _CACHE["models"] = (_model(), _model())
    return tuple(m.engine(DEV) for m in _CACHE["models"])


def _ragged(sizes, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return Batch.from_data_list([make_system(gen, n - 4, 4, sid=str(i)) for i, n in enumerate(sizes)])


def _sample(eng, batch, split, T=3, ode=True, ads_only=False, static=True, incremental=True, per_system=False, early=0,
            poll=0, seed=3):
    """One fused run at the engine's own interface, the way Denoiser._sample drives it -> pos, f1, f2, state, sys_state."""
    b = batch.clone().to(DEV)
    B, N = int(b.natoms.shape[0]), int(b.pos.shape[0])
    gen = torch.Generator().manual_seed(seed)
    prep = eng.prepare(b)
    pos = b.pos.to(torch.float32).contiguous().clone()
    eng.init_placement(prep, pos, torch.rand(B, 3, generator=gen).to(DEV))
    zt = zr = None
    if not ode:
        zt, zr = (torch.randn(T, B, 3, generator=gen).to(DEV) for _ in range(2))
    coefs = schedule_coefs(dict(PARAMS, num_steps=T, ode=ode))
    coefs_dev = torch.tensor([[c.coef_tr, c.rot_pre, c.rot_dt, c.rot_g2, c.noise_tr, c.noise_rot] for c in coefs],
                             dtype=torch.float32, device=DEV)
    f1, f2 = (torch.zeros(N, 3, dtype=torch.float32, device=DEV) for _ in range(2))
    state = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    sys_state = torch.tensor([[0, 0, 0, -1]] * B, dtype=torch.int32, device=DEV) if per_system else None
    out_idx = torch.nonzero(prep.tags == 2).reshape(-1).to(torch.int32).contiguous() if ads_only else None
    try:
        if static:
            eng.set_moving_atoms(prep, prep.tags == 2)
        eng.set_incremental(incremental and static)
        if per_system:
            eng.set_per_system_stop(sys_state)
        eng.sample(prep, pos, f1, f2, coefs_dev, T, state, zt, zr, early_stop_count=early, poll_every=poll, out_idx=out_idx,
                   split_streams=split)
        eng.check_flags()
        torch.cuda.synchronize()
    finally:
        eng.set_moving_atoms(None, None)
        eng.set_per_system_stop(None)
    return pos, f1, f2, state, sys_state, out_idx


def _same(a, b):
    pos_a, f1_a, f2_a, st_a, ss_a, idx = a
    pos_b, f1_b, f2_b, st_b, ss_b, _ = b
    assert torch.equal(pos_a, pos_b)
    rows = slice(None) if idx is None else idx.long()       # adsorbate-only outputs: the other rows are not written
    assert torch.equal(f1_a[rows], f1_b[rows]) and torch.equal(f2_a[rows], f2_b[rows])
    assert torch.equal(st_a, st_b), (st_a.tolist(), st_b.tolist())
    if ss_a is not None:
        assert torch.equal(ss_a, ss_b)


def _plain(key, batch, **kw):
    """The one-stream run of a case, computed once and shared."""
    if key not in _CACHE:
        _CACHE[key] = _sample(_engines()[1], batch, False, **kw)
    return _CACHE[key]


@pytest.mark.parametrize("variant", ["all_atoms", "out_idx", "no_incremental", "no_static_cache"])
@pytest.mark.parametrize("nsys", [2, 3, 5])
def test_split_run_equals_the_one_stream_run_on_ragged_batches(nsys, variant):
    kw = {"all_atoms": {}, "out_idx": dict(ads_only=True), "no_incremental": dict(incremental=False),
          "no_static_cache": dict(static=False)}[variant]
    batch = _ragged(RAGGED[nsys])
    eng = _engines()[0]
    runs = eng.split_stats()[0]
    got = _sample(eng, batch, True, **kw)
    assert eng.split_stats()[0] == runs + 1                   # it did go through the split loop
    _same(got, _plain((nsys, variant), batch, **kw))
    assert int(got[3][3]) == 3 and int(got[3][4]) == 3


def test_both_views_search_the_whole_batchs_lattice_images():
    gen = torch.Generator().manual_seed(21)
    small, large = make_system(gen, 8, 4, sid="small"), make_system(gen, 196, 4, sid="large")
    ra, rb = cell_repeats(small.cell, HP["cutoff"]), cell_repeats(large.cell, HP["cutoff"])
    assert ra != rb and max(ra) > max(rb), (ra, rb)           # built alone, the two sides would search different images
    batch = Batch.from_data_list([small, large])
    _same(_sample(_engines()[0], batch, True), _plain("images", batch))


def test_sde_noise_tables_are_read_with_the_whole_batchs_stride():
    batch = _ragged(RAGGED[5])
    got = _sample(_engines()[0], batch, True, ode=False)
    _same(got, _plain("sde", batch, ode=False))
    assert not torch.equal(got[0], _plain((5, "all_atoms"), batch)[0])   # the noise did move the sites


def test_per_system_early_stop_freezes_systems_on_both_sides():
    batch = batch_from_fixture(load_npz("stepper_ode8.npz"), pos_key="pos_in")      # 4 systems x 40 atoms: cut after 2
    kw = dict(T=40, per_system=True, early=10, poll=5, seed=11)
    eng = _engines()[0]
    runs = eng.split_stats()[0]
    got = _sample(eng, batch, True, **kw)
    assert eng.split_stats()[0] == runs + 1
    _same(got, _plain("per_system", batch, **kw))
    frozen = got[4][:, 1].tolist()
    print("per-system stop: frozen", frozen, "stop steps", got[4][:, 3].tolist())
    assert any(frozen[:2]) and any(frozen[2:]), frozen        # one system froze on each side


def test_consecutive_split_runs_do_not_trust_a_finished_runs_state():
    eng = _engines()[0]
    first, second = _ragged(RAGGED[5], seed=7), _ragged(RAGGED[5], seed=8)          # same shapes, other positions
    a1 = _sample(eng, first, True)
    b1 = _sample(eng, second, True)
    a2 = _sample(eng, first, True)
    _same(a1, a2)                                             # run-to-run identity, with another run in between
    _same(b1, _plain("second", second))
    _same(a1, _plain((5, "all_atoms"), first))


def test_fallbacks_run_the_one_stream_loop(tmp_path):
    eng, plain_eng = _engines()
    batch = _ragged(RAGGED[3])
    runs = eng.split_stats()[0]
    # one system
    one = _ragged((65,))
    _same(_sample(eng, one, True), _plain("one", one))
    # whole-batch (coupled) early stop
    kw = dict(T=12, early=10, poll=5)
    _same(_sample(eng, batch, True, **kw), _plain("coupled", batch, **kw))
    # a trajectory sink: through the Denoiser, which owns the sink
    trainers = [DenoisingTrainer(m, device=DEV) for m in _CACHE["models"]]
    place = torch.rand(3, 3, generator=torch.Generator().manual_seed(5))
    outs = []
    for tr, split, d in ((trainers[0], True, "a"), (trainers[1], False, "b")):
        b = batch.clone()
        b.sid = ["x", "y", "z"]
        den = Denoiser(b, DiffTorchCalc(tr), dict(PARAMS, early_stop=False, placement_noise=place, split_streams=split),
                       device=DEV, traj_dir=str(tmp_path / d), traj_names=b.sid)
        outs.append(den.run().pos.clone())
    assert torch.equal(outs[0], outs[1])
    assert eng.split_stats()[0] == runs                       # none of the three went through the split loop


def test_exact_f32_falls_back_to_the_one_stream_loop():
    a, b = _model().engine(DEV), _model().engine(DEV)         # fresh engines: the switch to exact f32 stays
    batch = _ragged(RAGGED[2])
    assert a.use_exact_f32() and b.use_exact_f32()
    got = _sample(a, batch, True)
    assert a.split_stats() == (0, 1)
    _same(got, _sample(b, batch, False))


def test_set_weights_on_the_parent_reaches_the_twin():
    m = _model()
    eng = m.engine(DEV)
    batch = _ragged(RAGGED[3])
    before = _sample(eng, batch, True)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.03125)
    eng = m.engine(DEV)                                        # re-binds the weights of the same handle
    assert eng.split_stats()[0] == 1
    after = _sample(eng, batch, True)
    assert eng.split_stats()[0] == 2
    fresh = PaiNN(None, 50, 1, scale_file=dict(SCALES), so3_denoising=True, **HP)
    fresh.load_state_dict(m.state_dict(), strict=False)
    _same(after, _sample(fresh.to(DEV).eval().engine(DEV), batch, False))
    assert not torch.equal(before[1], after[1])


def test_profile_and_counters_of_the_pair():
    eng, plain_eng = _engines()
    batch = _ragged(RAGGED[5])
    for e in (eng, plain_eng):
        e.profile_enable(True)
    try:
        _sample(eng, batch, True, incremental=False)     # (every forward then makes the same kernel groups)
        _sample(plain_eng, batch, False, incremental=False)
        cs, cp = eng.counters(), plain_eng.counters()
        ps, pp = eng.profile_read(), plain_eng.profile_read()
    finally:
        for e in (eng, plain_eng):
            e.profile_enable(False)
    assert (cs.num_edges, cs.num_atoms) == (cp.num_edges, cp.num_atoms) and cs.num_atoms == sum(RAGGED[5])
    assert (cs.dense_flops, cs.message_bytes_per_layer) == (cp.dense_flops, cp.message_bytes_per_layer)
    for cat in eng.PROFILE_CATEGORIES:
        assert ps[cat][1] == 2 * pp[cat][1] and pp[cat][1] > 0, (cat, ps[cat], pp[cat])   # groups of both handles
    assert ps["message_ksteps"] == pp["message_ksteps"]
