"""GPU tests of ml_relax: the S2EF PaiNN energy head (adf_painn_forward_energy) and the device L-BFGS (csrc/lbfgs.hip)
against the reference's own outputs and runs recorded by tools/make_golden_relax.py."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc
from adsorbdiff_amd.ml_relaxation import ml_relax
from adsorbdiff_amd.painn import PaiNN
from adsorbdiff_amd.trainer import ForcesTrainer
from tests.helpers import batch_from_fixture, load_npz, rel_err, row_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 1e-4
HP = {"small": dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20),
      "full": dict(hidden_channels=512, num_layers=6, num_rbf=128, cutoff=12.0, max_neighbors=50)}
SCALES = {"small": {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9},
          "full": {f"upd_out_scalar_scale_{i}": 1.0 - 0.04 * i for i in range(6)}}


def _sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def _model(tag="small", seed=None):
    fx = load_npz("relax_painn.npz")
    torch.manual_seed(int(fx[f"{tag}_seed"]) if seed is None else seed)
    return PaiNN(None, 50, 1, scale_file=dict(SCALES[tag]), **HP[tag]).to(DEV).eval()


@pytest.mark.parametrize("tag", ["small", "full"])
def test_energy_and_forces_vs_reference_fixture(tag):
    """The small batch holds a pair of atoms 5e-4 A apart: it checks that both graphs drop it (d^2 <= 1e-4), not the
    distance floor, which no edge reaches (test_distance_floor_clamps_edges exercises the floor)."""
    fx = _sub(load_npz("relax_painn.npz"), tag + "_")
    out = _model(tag)(batch_from_fixture(fx, device=DEV))
    assert row_rel_err(out["energy"].cpu().reshape(-1, 1), torch.from_numpy(fx["energy"]).reshape(-1, 1)) < REL_TOL
    assert rel_err(out["forces"].cpu(), fx["forces"]) < REL_TOL
    assert set(out) == {"energy", "forces"}


def test_distance_floor_clamps_edges():
    """adf_painn_set_distance_floor: with a floor above some edge lengths those edges get exactly the floor; back at the
    default the graph is the unclamped one again."""
    import ctypes as C

    from adsorbdiff_amd import lib as L

    fx = _sub(load_npz("relax_painn.npz"), "small_")
    m = _model()
    b = batch_from_fixture(fx, device=DEV)
    eng = m.engine(DEV)
    eng.build_graph(b)
    d_ref = eng.export_graph()[5].clone()
    floor = float(d_ref.median())
    L.check(eng.lib.adf_painn_set_distance_floor(eng.handle, C.c_float(floor)))
    eng.build_graph(b)
    d_fl = eng.export_graph()[5]
    assert d_fl.shape == d_ref.shape
    assert torch.equal(torch.sort(d_fl).values, torch.sort(torch.clamp(d_ref, min=floor)).values)
    assert bool((d_fl >= floor).all()) and bool((d_ref < floor).any())
    L.check(eng.lib.adf_painn_set_distance_floor(eng.handle, C.c_float(m.distance_floor)))
    eng.build_graph(b)
    assert torch.equal(torch.sort(eng.export_graph()[5]).values, torch.sort(d_ref).values)


def test_energy_bit_identical_alone_and_in_batch():
    fx = _sub(load_npz("relax_painn.npz"), "small_")
    m = _model()
    b = batch_from_fixture(fx, device=DEV)
    full = m(b)
    for s, d in enumerate(b.to_data_list()):
        d.batch = torch.zeros(d.pos.shape[0], dtype=torch.long, device=DEV)
        one = m(d)
        assert torch.equal(one["energy"].view(torch.int32), full["energy"][s:s + 1].view(torch.int32))


def test_energy_only_model_matches_energy_of_full_model():
    fx = _sub(load_npz("relax_painn.npz"), "small_")
    m = _model()
    torch.manual_seed(int(load_npz("relax_painn.npz")["small_seed"]))
    e_only = PaiNN(None, 50, 1, scale_file=dict(SCALES["small"]), regress_forces=False, **HP["small"])
    e_only.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("out_forces")})
    e_only = e_only.to(DEV).eval()
    b = batch_from_fixture(fx, device=DEV)
    out = e_only(b)
    assert set(out) == {"energy"}
    assert torch.equal(out["energy"], m(b)["energy"])


class _Fixed:
    """A trainer whose predict returns whatever forces the test put there (teacher forcing)."""

    def __init__(self):
        self._unwrapped_model = type("M", (), {"otf_graph": True})()
        self.forces = None

    def predict(self, batch, per_image=False, disable_tqdm=True):
        return {"energy": torch.zeros(int(batch.natoms.shape[0]), device=DEV), "forces": self.forces.clone()}


def _ulp_close(a, b):
    a, b = a.float().cpu(), torch.as_tensor(b).float()
    up = torch.nextafter(b, torch.full_like(b, float("inf"))) - b
    return bool(((a - b).abs() <= up.abs() + 0.0).all())


@pytest.mark.parametrize("tag", ["ring", "early"])
def test_teacher_forced_steps_vs_reference(tag):
    fx = _sub(load_npz("relax_teacher.npz"), tag + "_")
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    tr = _Fixed()
    opt = LBFGS(b, TorchCalc(tr), maxstep=float(fx["maxstep"]), memory=int(fx["memory"]), damping=float(fx["damping"]),
                alpha=float(fx["alpha"]), device=DEV, early_stop_batch=bool(fx["early"]))
    opt.fmax = float(fx["fmax"])
    opt._setup()
    for k in range(fx["forces"].shape[0]):
        f = torch.from_numpy(fx["forces"][k]).to(DEV)
        tr.forces = f
        _, energy, forces = opt.check_convergence(k)
        assert torch.equal(opt.max_force_log[-1].cpu().ge(opt.fmax), torch.from_numpy(fx["masks"][k])), k
        opt.step(k, forces)
        assert bool(opt.last_step_max() < 1e-7) == bool(fx["skipped"][k]), k
        assert _ulp_close(b.pos, fx["pos_after"][k]), (k, float((b.pos.cpu() - torch.from_numpy(fx["pos_after"][k])).abs().max()))
    # the same iteration again (or any other but the next) is refused: it would append a history entry without its rho
    with pytest.raises(ValueError, match="iteration"):
        opt.step(k, forces)
    # reset: a fresh run from the first positions replays the reference's first steps
    opt.reset()
    assert not bool(opt.update_mask().any())
    b.pos.copy_(torch.from_numpy(fx["pos_in"]).to(DEV))
    for k in range(4):
        tr.forces = torch.from_numpy(fx["forces"][k]).to(DEV)
        _, _, forces = opt.check_convergence(k)
        assert torch.equal(opt.update_mask().cpu().bool(), torch.from_numpy(fx["masks"][k])), k
        opt.step(k, forces)
        assert _ulp_close(b.pos, fx["pos_after"][k]), k
    opt.close()


def test_nan_force_clears_mask_and_does_not_skip():
    """A NaN force propagates through the maxima as in the reference: its system's mask is clear, the step is not
    skipped."""
    fx = _sub(load_npz("relax_teacher.npz"), "ring_")
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    tr = _Fixed()
    opt = LBFGS(b, TorchCalc(tr), maxstep=0.04, memory=5, damping=1.0, alpha=70.0, device=DEV)
    opt.fmax = 1e-3
    opt._setup()
    f = torch.from_numpy(fx["forces"][0]).to(DEV)
    f[int(fx["natoms"][0]) - 1, 1] = float("nan")   # the last atom of system 0 (a free adsorbate atom)
    tr.forces = f
    _, _, forces = opt.check_convergence(0)
    assert torch.isnan(opt.max_force_log[-1][0]) and opt.update_mask().tolist() == [0, 1, 1]
    assert not opt._all_converged()
    opt.step(0, forces)
    assert torch.isnan(opt.last_step_max())
    opt.close()


class _Harmonic:
    def __init__(self, fx):
        self._unwrapped_model = type("M", (), {"otf_graph": True})()
        self.xstar = torch.from_numpy(fx["xstar"]).to(DEV)
        self.k = torch.from_numpy(fx["k"]).to(DEV)
        self.calls = 0

    def predict(self, batch, per_image=False, disable_tqdm=True):
        self.calls += 1
        kk = self.k[batch.batch].reshape(-1, 1)
        d = batch.pos - self.xstar
        e = torch.zeros(int(batch.natoms.shape[0]), device=DEV).index_add_(0, batch.batch, (0.5 * kk * d * d).sum(1))
        return {"energy": e, "forces": -kk * d}


def _harmonic_run(fx, **kw):
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    opt = LBFGS(b, TorchCalc(_Harmonic(fx)), maxstep=0.04, memory=int(fx["memory"]), damping=1.0, alpha=70.0, device=DEV,
                **kw)
    out = opt.run(fmax=float(fx["fmax"]), steps=int(fx["steps"]))
    return opt, out


def test_harmonic_relaxation_vs_reference():
    fx = load_npz("relax_harmonic.npz")
    opt, out = _harmonic_run(fx)
    assert opt.iterations == int(fx["iterations"])
    masks = torch.stack(opt.max_force_log).cpu().ge(float(fx["fmax"]))
    assert torch.equal(masks, torch.from_numpy(fx["masks"]))
    assert float((out.pos.cpu() - torch.from_numpy(fx["pos_final"])).abs().max()) < 1e-5
    assert rel_err(out.force.cpu(), fx["force"]) < REL_TOL


def test_painn_relaxation_vs_reference_and_reproducible():
    fx = load_npz("relax_run.npz")
    m = _model(seed=int(fx["seed"]))
    tr = ForcesTrainer(m, device=DEV)
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    opt = LBFGS(b, TorchCalc(tr), maxstep=0.04, memory=int(fx["memory"]), damping=1.0, alpha=70.0, device=DEV)
    out = opt.run(fmax=float(fx["fmax"]), steps=int(fx["steps"]))
    assert opt.iterations == int(fx["iterations"])
    assert torch.equal(torch.stack(opt.max_force_log).cpu().ge(float(fx["fmax"])), torch.from_numpy(fx["masks"]))
    assert float((out.pos.cpu() - torch.from_numpy(fx["pos_final"])).abs().max()) < 1e-4
    assert row_rel_err(out.y.cpu().reshape(-1, 1), torch.from_numpy(fx["y"]).reshape(-1, 1)) < REL_TOL
    assert rel_err(out.force.cpu(), fx["force"]) < REL_TOL
    # ml_relax on the same batch: the same bits (a second run of the same relaxation)
    b2 = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    out2 = ml_relax(b2, tr, steps=int(fx["steps"]), fmax=float(fx["fmax"]), relax_opt={"memory": int(fx["memory"])},
                    save_full_traj=False, device=DEV)
    assert torch.equal(out2.pos, out.pos) and torch.equal(out2.y, out.y) and torch.equal(out2.force, out.force)


@pytest.mark.parametrize("full", [True, False])
def test_trajectory_frame_rule(tmp_path, full):
    fx = load_npz("relax_harmonic.npz")
    opt, out = _harmonic_run(fx, save_full_traj=full, traj_dir=tmp_path, traj_names=["a", "b", "c"])
    masks = fx["masks"]
    for s, name in enumerate(["a", "b", "c"]):
        assert not (tmp_path / f"{name}.npz_tmp").exists()
        with np.load(tmp_path / f"{name}.npz") as z:
            n = int(fx["natoms"][s])
            want = int(masks[:, s].sum()) if full else 2
            assert z["positions"].shape == (want, n, 3) and z["forces"].shape == (want, n, 3) and z["energy"].shape == (want,)
            a0 = int(fx["natoms"][:s].sum())
            np.testing.assert_array_equal(z["positions"][0], fx["pos_in"][a0:a0 + n])
            assert z["numbers"].shape == (n,) and z["cell"].shape == (3, 3)
            np.testing.assert_array_equal(z["fixed"], fx["fixed"][a0:a0 + n])
            if not full:
                np.testing.assert_array_equal(z["positions"][-1], out.pos.cpu().numpy()[a0:a0 + n])
