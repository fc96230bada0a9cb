"""CPU tests of the gradient-force interface of the S2EF PaiNN (``PaiNN.force_mode``, the C entry
``adf_painn_forward_energy_gradient``, ``ForcesTrainer.predict``'s scaling rule) and of the float64 oracle the GPU tests use
(tests/helpers_grad_forces.py), pinned to the reference's own float64 autograd in tests/golden/grad_forces.npz
(tools/make_golden_grad_forces.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.painn import PaiNN
from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_grad_forces as HG
from tests.helpers import batch_from_fixture, load_npz

HP_SMALL = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES_SMALL = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}


def _sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def test_force_mode_default_validation_and_constructor_still_rejects_direct_forces_false():
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=1)
    assert m.force_mode == "direct"
    m.force_mode = "energy_gradient"
    assert m.force_mode == "energy_gradient"
    with pytest.raises(ValueError, match="force_mode"):
        m.force_mode = "autograd"
    assert m.force_mode == "energy_gradient"
    m.force_mode = "direct"
    assert "force_mode" not in m.state_dict() and "_force_mode" not in m.state_dict()
    # gradient forces do not need a force head
    e_only = PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, regress_forces=False)
    e_only.force_mode = "energy_gradient"
    # the reference's direct_forces=False differentiates sum(x), not the energy: still not offered
    with pytest.raises(ValueError):
        PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, direct_forces=False)


def test_c_entries_exist_with_declared_signature_and_reject_null_arguments():
    lib = L.load()
    assert "adf_painn_forward_energy_gradient" in L.EXPORTS and "adf_painn_energy_gradient_workspace" in L.EXPORTS
    fn = lib.adf_painn_forward_energy_gradient
    assert fn.argtypes == [C.c_void_p, C.POINTER(L.BatchDesc), C.c_void_p, C.c_void_p, C.c_void_p] and fn.restype == C.c_int32
    assert fn(None, None, None, None, None) == L.ADF_EINVAL
    desc = L.BatchDesc()
    assert fn(None, C.byref(desc), None, None, None) == L.ADF_EINVAL
    with pytest.raises(ValueError, match="null argument"):
        L.check(fn(None, C.byref(desc), None, None, None))
    n = C.c_int64(0)
    assert lib.adf_painn_energy_gradient_workspace(None, 100, C.byref(n)) == L.ADF_EINVAL
    header = (L.lib_path().parent.parent / "include" / "adsorbdiff_hip.h").read_text()
    assert "int32_t adf_painn_forward_energy_gradient(adf_painn_t h, const adf_batch* b, float* energy, float* forces, void* stream);" in header
    assert "torch.autograd.grad(out[\"energy\"].sum(), pos)" in header   # the reference expression it replaces


class _Stub(torch.nn.Module):
    """A model that returns fixed outputs and carries a force_mode."""

    def __init__(self, mode):
        super().__init__()
        self.force_mode = mode
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, data):
        return {"energy": torch.tensor([1.0, -2.0]), "forces": torch.tensor([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])}


def test_predict_scales_gradient_forces_by_the_energy_std_only():
    norms = {"target": {"mean": 3.0, "stdev": 2.0}, "grad_target": {"mean": 0.25, "stdev": 5.0}}
    raw = _Stub("direct")(None)
    out = ForcesTrainer(_Stub("direct"), device="cpu", normalizers=norms).predict(None)
    assert torch.equal(out["energy"], raw["energy"] * 2.0 + 3.0)
    assert torch.equal(out["forces"], raw["forces"] * 5.0 + 0.25)
    out = ForcesTrainer(_Stub("energy_gradient"), device="cpu", normalizers=norms).predict(None)
    assert torch.equal(out["energy"], raw["energy"] * 2.0 + 3.0)
    assert torch.equal(out["forces"], raw["forces"] * 2.0)   # the gradient of the energy returned: its std, no mean
    # no energy normaliser: the gradient forces are returned as they are, whatever the forces normaliser says
    out = ForcesTrainer(_Stub("energy_gradient"), device="cpu", normalizers={"grad_target": norms["grad_target"]}).predict(None)
    assert torch.equal(out["forces"], raw["forces"])


def test_fixture_gradient_agrees_with_its_recorded_central_difference():
    fx = load_npz("grad_forces.npz")
    ana = -(fx["small_forces"] * fx["small_fd_v"]).sum()
    assert fx["small_forces"].dtype == np.float64
    assert abs(ana - float(fx["small_fd"])) / abs(float(fx["small_fd"])) < 1e-7
    # (e): the analytic directional derivative and the h = 1e-2 difference agree to the truncation of that step
    assert abs(float(fx["dir_ana64"]) - float(fx["dir_fd64"])) / abs(float(fx["dir_fd64"])) < 1e-3
    for tag in ("small", "full", "nohead", "ragged"):
        f = torch.from_numpy(fx[f"{tag}_forces"])
        net = torch.zeros(len(fx[f"{tag}_natoms"]), 3, dtype=torch.float64).index_add_(0, torch.from_numpy(fx[f"{tag}_batch"]).long(), f)
        assert float(net.abs().max()) < 1e-12 * float(f.abs().max())
        assert 0 < float(fx[f"{tag}_err32"]) < 2e-5 and 0 < float(fx[f"{tag}_net32"]) < 1e-5


def test_seeded_models_draw_the_fixture_weights():
    fx = load_npz("grad_forces.npz")
    for tag, kw in (("small", {}), ("nohead", dict(regress_forces=False))):
        torch.manual_seed(int(fx[f"{tag}_seed"]))
        m = PaiNN(None, 50, 1, scale_file=dict(SCALES_SMALL), **HP_SMALL, **kw)
        sums = np.array([float(v.double().sum()) for v in m.state_dict().values()])
        assert np.array_equal(sums, fx[f"{tag}_sums"])


def test_float64_oracle_matches_reference_autograd_on_the_reference_graph():
    """The oracle of the GPU tests on fixture (a), with the reference's own symmetrised edge list: float64 against float64."""
    fx = _sub(load_npz("grad_forces.npz"), "small_")
    torch.manual_seed(int(fx["seed"]))
    m = PaiNN(None, 50, 1, scale_file=dict(SCALES_SMALL), **HP_SMALL)
    b = batch_from_fixture(fx)
    src, dst = torch.from_numpy(fx["edge_src"]).long(), torch.from_numpy(fx["edge_dst"]).long()
    off = HG.shift_offsets(torch.from_numpy(fx["edge_shift"]), b.cell, b.batch, dst)
    e, f = HG.energy_forces(m.state_dict(), b.pos, b.atomic_numbers, b.batch, len(b.natoms), src, dst, off,
                            scale_factors=m.scale_factors(), **HP_SMALL)
    assert float((e - torch.from_numpy(fx["energy"])).abs().max()) < 1e-10 * float(np.abs(fx["energy"]).max())
    assert float((f - torch.from_numpy(fx["forces"])).abs().max()) < 1e-10 * float(np.abs(fx["forces"]).max())
    # and the offsets recovered from edge vectors (what the GPU tests do with the engine's exported graph) are the same
    vec = b.pos.double()[src] - b.pos.double()[dst] + off
    assert torch.equal(HG.edge_offsets(b.pos, b.cell, b.batch, src, dst, vec.float()), off)
