"""GPU tests of the translation-only samplers Denoiser.reverse_sde_sampling / langevin_dynamics (csrc/stepper.hip
adf_tr_* kernels, adf_tr_sample / adf_eqv2_tr_sample fused loops) against the reference's own runs recorded by
tools/make_golden_samplers.py.  Tolerances are those of test_gpu_parity.py::test_stepper_each_step_vs_reference_fixture."""
import ctypes

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc, langevin_coefs, ode_tr_coefs
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.sampler import adsorbate_sites, shard_batch
from adsorbdiff_amd.synthetic import make_batch
from adsorbdiff_amd.trainer import DenoisingTrainer
from tests.helpers import batch_from_fixture, load_npz, rel_err, row_rel_err, state_dict_from_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 1e-4
HP = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
ALL = ["ode_large", "ode_mild", "ode_early", "lgv_1head", "lgv_2head"]


def _model(gain=1.0, bias=0.0, heads=2):
    """The stepper fixtures' small PaiNN (stepper_ode8.npz) with the head gain of tools/make_golden_samplers.py."""
    sd = state_dict_from_fixture(load_npz("stepper_ode8.npz"))
    for head in ("out_forces", "out_forces2")[:heads]:
        sd[f"{head}.output_network.1.update_net.2.weight"].mul_(gain)
        sd[f"{head}.output_network.1.update_net.2.bias"].mul_(gain).add_(bias)
    if heads == 1:
        sd = {k: v for k, v in sd.items() if not k.startswith("out_forces2.")}
    m = PaiNN(None, 50, 1, scale_file=dict(SCALES), so3_denoising=heads == 2, **HP)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert set(missing) <= {"atom_radii"} and not unexpected, (missing, unexpected)
    return m.to(DEV).eval()


def _fx(name):
    fx = load_npz(f"sampler_{name}.npz")
    fx["langevin"] = fx["sampler"].item() == b"langevin"
    return fx


def _fx_model(fx):
    return _model(float(fx["gain"]), float(fx["bias"]), int(fx["heads"]))


def _params(fx):
    p = dict(num_steps=int(fx["num_steps"]), ads_std_low=0.1, ads_std_high=10)
    if fx["langevin"]:
        p.update(n_step_each=int(fx["n_step_each"]), step_lr=float(fx["step_lr"]))
    return p


def _coefs(fx):
    return langevin_coefs(_params(fx)) if fx["langevin"] else ode_tr_coefs(_params(fx))


@pytest.mark.parametrize("name", ALL)
def test_translation_step_each_step_vs_reference_fixture(name):
    """Teacher forcing on the reference's recorded positions: per model call, forward + adf_tr_step against the
    reference's per-system head-1 score, wrapped dcom and the positions after the step; slab atoms never move."""
    fx = _fx(name)
    m = _fx_model(fx)
    eng = m.engine()
    coefs = _coefs(fx)
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    prep = eng.prepare(b)
    B, N = prep.num_systems, prep.num_atoms
    torch.manual_seed(int(fx["seed"]))
    pos = b.pos.clone().contiguous()
    eng.init_placement(prep, pos, torch.rand(B, 3).to(DEV))
    log = torch.from_numpy(fx["pos_log"])
    np.testing.assert_allclose(pos.cpu().numpy(), log[0].numpy(), rtol=0, atol=2e-6)
    f1 = torch.empty(N, 3, device=DEV)
    f2 = torch.empty(N, 3, device=DEV) if int(fx["heads"]) == 2 else None
    # the fused loops' shared argument check rejects a negative subset size before any launch (here adf_sample)
    desc, state = prep.desc(pos), torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    out_idx, placed = torch.nonzero(b.tags == 2).reshape(-1).to(torch.int32).contiguous(), pos.clone()
    assert eng.lib.adf_sample(eng.handle, ctypes.byref(desc), pos.data_ptr(), prep.tags.data_ptr(), None,
                              torch.zeros(1, 6, device=DEV).data_ptr(), 1, None, None, 0, 0, state.data_ptr(),
                              out_idx.data_ptr(), -1, f1.data_ptr(), f1.data_ptr(), None) == L.ADF_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(pos, placed) and state.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    tags = torch.from_numpy(fx["tags"])
    ads = b.tags == 2
    cnt = torch.zeros(B, device=DEV).index_add_(0, b.batch[ads], torch.ones(int(ads.sum()), device=DEV))[:, None]
    calls, applied = log.shape[0], int(fx["applied"])
    for t in range(calls):
        pos = log[t].to(DEV).contiguous()
        before = pos.clone()
        eng.forward_prepared(prep, pos, f1, f2)
        score = (torch.zeros(B, 3, device=DEV).index_add_(0, b.batch[ads], f1[ads]) / cnt).cpu()
        ref = fx["ref_score"][t]
        assert rel_err(score, ref) < REL_TOL, (name, t, rel_err(score, ref))
        assert row_rel_err(score, ref) < REL_TOL, (name, t, row_rel_err(score, ref))
        z = torch.from_numpy(fx["ref_randn"][t]).to(DEV).contiguous() if fx["langevin"] else None
        state = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
        dcom = torch.empty(B, 3, device=DEV)
        eng.tr_step(prep, pos, f1, state, coef=coefs[t], z=z, early_stop_count=0, dcom=dcom)
        if t >= fx["ref_dcom"].shape[0]:
            continue
        raw = abs(coefs[t].coef) * float(np.abs(ref).max())
        if fx["langevin"]:
            raw += coefs[t].noise * float(np.abs(fx["ref_randn"][t]).max())
        tol_com = 1e-4 * raw + 2e-5
        err = float((dcom.cpu() - torch.from_numpy(fx["ref_dcom"][t])).abs().max())
        assert err < tol_com, (name, t, err, tol_com)
        if t < applied:
            want = log[t + 1] if t + 1 < calls else torch.from_numpy(fx["pos_final"])
            diff = (pos.cpu() - want).abs()
            assert float(diff.max()) < tol_com + 1e-5, (name, t, float(diff.max()))
        assert torch.equal(pos.cpu()[tags != 2], before.cpu()[tags != 2])  # slab rows never written


def _denoiser(fx, m, traj_dir=None, **extra):
    b = batch_from_fixture(fx, pos_key="pos_in")
    params = dict(_params(fx), **extra)
    return Denoiser(b, DiffTorchCalc(DenoisingTrainer(m, device=DEV)), params, device=DEV, traj_dir=traj_dir,
                    traj_names=b.sid)


@pytest.mark.parametrize("name", ["ode_mild", "lgv_1head", "lgv_2head"])
def test_free_running_vs_reference_final_positions(name):
    fx = _fx(name)
    extra = dict(langevin_noise=torch.from_numpy(fx["ref_randn"])) if fx["langevin"] else {}
    den = _denoiser(fx, _fx_model(fx), **extra)
    torch.manual_seed(int(fx["seed"]))   # placement: torch.rand(B, 3) on the CPU generator, as the reference
    den.langevin_dynamics() if fx["langevin"] else den.reverse_sde_sampling()
    assert den.steps_applied == int(fx["applied"])
    np.testing.assert_allclose(den.batch.pos.cpu().numpy(), fx["pos_final"], rtol=0, atol=1e-4)


def test_early_stop_matches_the_reference_step_count(tmp_path):
    fx = _fx("ode_early")
    den = _denoiser(fx, _fx_model(fx), traj_dir=tmp_path)
    torch.manual_seed(int(fx["seed"]))
    den.reverse_sde_sampling()
    assert den.steps_applied == int(fx["applied"]) == 9
    assert den.cvg_count == 10
    np.testing.assert_allclose(den.batch.pos.cpu().numpy(), fx["pos_final"], rtol=0, atol=1e-5)
    # the early-stopped run publishes its file, one frame per applied step
    z = np.load(tmp_path / "0.npz")
    assert z["positions"].shape[0] == 9
    assert np.array_equal(z["positions"][-1], den.batch.pos.cpu().numpy())


def _eqv2_model_and_batch():
    from tests.test_gpu_eqv2 import model_from_fixture

    fx = load_npz("eqv2_l4m2.npz")
    return model_from_fixture(fx), batch_from_fixture(fx)


def _sample(m, b, method, params, **extra):
    den = Denoiser(b.clone().to(DEV), DiffTorchCalc(DenoisingTrainer(m, device=DEV)), dict(params, **extra), device=DEV)
    getattr(den, method)()
    return den.batch.pos.cpu(), den


@pytest.mark.parametrize("model", ["painn", "eqv2"])
@pytest.mark.parametrize("method", ["reverse_sde_sampling", "langevin_dynamics"])
def test_fused_head1_loop_equals_the_per_step_two_head_path(model, method):
    """The fused loop evaluates head 1 only (no out_forces2 / force_block2); the per-step path (step_hook) runs the full
    two-head forward.  Same sites bit for bit, also with incremental layers and the adsorbate-only outputs switched."""
    if model == "painn":
        m, b = _model(gain=20.0), make_batch(3, n_slab=36, n_ads=4, seed=77)
    else:
        m, b = _eqv2_model_and_batch()
    B = int(b.natoms.shape[0])
    params = dict(num_steps=4, ads_std_low=0.1, ads_std_high=10, early_stop=False, n_step_each=2, step_lr=1e-5,
                  placement_noise=torch.rand(B, 3, generator=torch.Generator().manual_seed(3)))
    if method == "langevin_dynamics":
        params["langevin_noise"] = torch.randn(8, B, 3, generator=torch.Generator().manual_seed(4))
    hooked = []
    runs = {
        "fused": _sample(m, b, method, params)[0],
        "per_step": _sample(m, b, method, params, step_hook=hooked.append)[0],
        "no_incremental": _sample(m, b, method, params, incremental_layers=False)[0],
        "all_rows": _sample(m, b, method, params, scores_on_adsorbate_only=False)[0],
        "per_step_ads_only": _sample(m, b, method, params, step_hook=lambda t: None, scores_on_adsorbate_only=True)[0],
    }
    assert hooked == list(range(8 if method == "langevin_dynamics" else 4))
    for k, v in runs.items():
        assert torch.equal(v, runs["fused"]), k
    moved = (runs["fused"] - b.pos).abs()
    assert float(moved[b.tags != 2].max()) == 0.0 and float(moved[b.tags == 2].max()) > 1e-3


@pytest.mark.parametrize("method", ["reverse_sde_sampling", "langevin_dynamics"])
def test_eight_way_shards_reproduce_the_single_run(method):
    m = _model(gain=20.0)
    full = Batch.from_data_list(make_batch(9, n_slab=36, n_ads=3, seed=5).to_data_list()
                                + make_batch(7, n_slab=24, n_ads=4, seed=6).to_data_list())
    B = int(full.natoms.shape[0])
    placement = torch.rand(B, 3, generator=torch.Generator().manual_seed(0))
    z = torch.randn(3 * 2, B, 3, generator=torch.Generator().manual_seed(1))
    params = dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, early_stop=False, n_step_each=2, step_lr=1e-5)

    def run(batch, ids):
        idx = torch.tensor(ids, dtype=torch.long)
        extra = dict(placement_noise=placement[idx])
        if method == "langevin_dynamics":
            extra["langevin_noise"] = z[:, idx]
        pos, _ = _sample(m, batch, method, params, **extra)
        batch = batch.clone()
        batch.pos = pos
        return adsorbate_sites(batch)

    one = run(full, list(range(B)))
    seen = []
    for r in range(8):
        mine, ids = shard_batch(full, r, 8)
        seen += ids
        got = run(mine, ids)
        want = one[torch.tensor(ids)]
        A = max(got.shape[1], want.shape[1])
        pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, A - t.shape[1]), value=float("nan")).nan_to_num(7e7)
        assert torch.equal(pad(got), pad(want)), (method, r)
    assert sorted(seen) == list(range(B))


def test_trajectory_frames_per_inner_step(tmp_path):
    fx = _fx("lgv_1head")
    steps = int(fx["num_steps"]) * int(fx["n_step_each"])
    for sub, extra in (("fused", {}), ("per_step", dict(step_hook=lambda t: None))):
        d = tmp_path / sub
        den = _denoiser(fx, _fx_model(fx), traj_dir=d, langevin_noise=torch.from_numpy(fx["ref_randn"]), **extra)
        torch.manual_seed(int(fx["seed"]))
        den.langevin_dynamics()
        for s in range(int(fx["natoms"].shape[0])):
            z = np.load(d / f"{s}.npz")
            assert z["positions"].shape[0] == steps, (sub, s)
        assert np.array_equal(np.load(d / "0.npz")["positions"][-1], den.batch.pos.cpu().numpy()[: int(fx["natoms"][0])])


@pytest.mark.parametrize("sampler,method", [("sde", "reverse_sde_sampling"), ("langevin", "langevin_dynamics"),
                                            (None, "reverse_sde_sampling_rot")])
def test_run_dispatches_on_the_sampler_key(sampler, method):
    m = _model(gain=20.0)
    b = make_batch(2, n_slab=36, n_ads=4, seed=8)
    params = dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  n_step_each=2, step_lr=1e-5, placement_noise=torch.rand(2, 3, generator=torch.Generator().manual_seed(2)))
    if sampler == "langevin":
        params["langevin_noise"] = torch.randn(6, 2, 3, generator=torch.Generator().manual_seed(9))
    direct, _ = _sample(m, b, method, params)
    via_run = Denoiser(b.clone().to(DEV), DiffTorchCalc(DenoisingTrainer(m, device=DEV)),
                       dict(params, **({"sampler": sampler} if sampler else {})), device=DEV).run().pos.cpu()
    assert torch.equal(direct, via_run)
    if sampler is not None:   # and it is not the rot sampler
        rot, _ = _sample(m, b, "reverse_sde_sampling_rot", params)
        assert not torch.equal(rot, via_run)
