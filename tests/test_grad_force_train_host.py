"""Training on energy-gradient forces, on the CPU: the float64 oracle of tests/helpers_grad_force_train.py pinned to the
reference's own second-order autograd (tests/golden/grad_force_train.npz), the identity the device step rests on, what
``setup_training`` and the steps refuse, and the new C entries."""
import ctypes as C
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.painn import PaiNN
from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_grad_force_train as HG
from tests import helpers_s2ef_train as HS
from tests.helpers import rel_err

ROOT = Path(__file__).resolve().parent.parent

NEW_ENTRIES = ("adf_op_edge_tangent", "adf_op_rbf_dual", "adf_op_dual_bias", "adf_op_ssilu_dual_fwd", "adf_op_ssilu_dual_bwd",
               "adf_op_layernorm_dual_fwd", "adf_op_layernorm_dual_bwd", "adf_op_vdot_dual_fwd", "adf_op_vdot_dual_bwd",
               "adf_op_update_out_dual_fwd", "adf_op_update_out_dual_bwd", "adf_op_message_dual_fwd", "adf_op_message_dual_bwd")


def test_float64_oracle_reproduces_the_reference_second_order_autograd():
    """Both are float64 evaluations of the same graph (the reference's edge list with integer shifts is stored): loss, terms,
    energy and forces agree to 1e-10 relative, every parameter's gradient to 1e-9."""
    fx, m, b, kw, edges = HG.fixture_case()
    ref = HG.oracle_loss_and_grads(m, b, edges, **kw)
    e_loss = abs(float(ref["loss"]) - float(fx["loss"])) / abs(float(fx["loss"]))
    e_terms = float(((ref["terms"] - torch.as_tensor(fx["loss_terms"])).abs() / torch.as_tensor(fx["loss_terms"]).abs()).max())
    e_e, e_f = rel_err(ref["energy"], fx["energy_pred"]), rel_err(ref["forces"], fx["forces_pred"])
    errs = HG.fixture_gradient_errors(fx, ref["grads"])
    worst, worst_name = max((e, k) for k, e in errs.items())
    print(f"float64 oracle vs the reference: loss {e_loss:.1e} terms {e_terms:.1e} energy {e_e:.1e} forces {e_f:.1e}, "
          f"worst of {len(errs)} gradients {worst:.1e} ({worst_name})")
    assert len(errs) == len(HG.objective_names(m)) == sum(p.requires_grad for p in m.parameters())
    assert e_loss < 1e-10 and e_terms < 1e-10 and e_e < 1e-10 and e_f < 1e-10
    assert all(e < 1e-9 for e in errs.values()), {k: e for k, e in errs.items() if not e < 1e-9}
    assert (ROOT / "tests" / "golden" / "grad_force_train.npz").stat().st_size < 2**20


def test_force_term_gradient_is_minus_the_directional_derivative_of_the_energy_gradient():
    """The identity the device step rests on, on the smallest configuration ("single"): with v = dL/dF held constant, the
    parameter gradient of the force term equals  -d/d eps grad_theta sum_b E_b(pos + eps v)  at eps = 0.  The right side by
    central differences in float64 at eps |v|_max = 1e-5 A.  Measured on the CPU: 2.54e-8 relative over all parameters
    concatenated (the truncation error of the difference: 2.5e-6 at 1e-4 A, a hundred times less at a tenth of the step);
    the bound is ten times that."""
    name = "single"
    m, b = HG.make_config_model(name), HG.make_config_batch(name)
    graph = HS.oracle_graph(m, b)
    src, dst = graph[0]
    from tests import helpers_grad_forces as GF

    edges = (src, dst, GF.edge_offsets(b.pos, b.cell, b.batch.long(), src, dst, graph[2] * graph[1][:, None]))
    kw = dict(normalizers=HG.NORMALIZERS, **HG.COEFFICIENTS)
    ref = HG.oracle_loss_and_grads(m, b, edges, split=True, **kw)
    # v = dL/dF at the oracle's forces
    f = ref["forces"].clone().requires_grad_(True)
    ne = (kw["normalizers"]["energy"]["mean"], kw["normalizers"]["energy"]["stdev"])
    _, _, lf = HS.s2ef_loss(ref["energy"], f, b.energy.double(), b.forces.double(), b.fixed, ne, (0.0, ne[1]),
                            kw["energy_coefficient"], kw["force_coefficient"], True, None)
    (v,) = torch.autograd.grad(lf, f)
    names = HG.objective_names(m)
    hp = HS.hyper(m)

    def energy_gradient_wrt_parameters(pos):
        sd = {k: t.detach().double() if t.is_floating_point() else t.detach() for k, t in m.state_dict().items()}
        leaves = {k: sd[k].clone().requires_grad_(True) for k in names}
        sd.update(leaves)
        e, _, _ = HG.energy_and_forces(sd, pos, b.atomic_numbers, b.batch, int(b.natoms.shape[0]), src.long(), dst.long(),
                                       edges[2], create_graph=True, **hp)
        gs = torch.autograd.grad(e.sum(), [leaves[k] for k in names], allow_unused=True)
        return torch.cat([(g if g is not None else torch.zeros_like(leaves[k])).reshape(-1) for k, g in zip(names, gs)])

    eps = 1e-5 / float(v.abs().max())
    p0 = b.pos.double()
    fd = -(energy_gradient_wrt_parameters(p0 + eps * v) - energy_gradient_wrt_parameters(p0 - eps * v)) / (2 * eps)
    ana = torch.cat([ref["grads_force"][k].reshape(-1) for k in names])
    err = float((fd - ana).norm() / ana.norm())
    print(f"identity on {name}: |grad of the force term| {float(ana.norm()):.4g}, central difference deviates {err:.2e}")
    assert float(ana.norm()) > 0 and err < 2.6e-7


def test_setup_training_refusals_and_the_value_error():
    from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20
    from adsorbdiff_amd.train_step import PaiNNGradForceTrainStep, PaiNNS2EFTrainStep, _PaiNNStepBase

    assert issubclass(PaiNNGradForceTrainStep, _PaiNNStepBase) and PaiNNGradForceTrainStep.UNUSED_PREFIXES == ("out_forces.",)
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, cutoff=6.0, max_neighbors=20)
    tr = ForcesTrainer(m, device="cpu")
    # the model's mode and the objective must agree: the error names both switches
    with pytest.raises(ValueError, match="force_objective.*force_mode"):
        tr.setup_training(1e-3, force_objective="energy_gradient")
    with pytest.raises(ValueError, match="force_objective.*force_mode"):
        PaiNNGradForceTrainStep(m, "cuda:0")
    with pytest.raises(ValueError, match="force_objective"):
        tr.setup_training(1e-3, force_objective="both")
    m.force_mode = "energy_gradient"
    # the existing refusal stays with the keyword at its default, and now says what to pass
    with pytest.raises(NotImplementedError, match="second-order"):
        tr.setup_training(1e-3)
    with pytest.raises(NotImplementedError, match="force_objective='energy_gradient'"):
        PaiNNS2EFTrainStep(m, "cuda:0")
    # both switches set: only the device is missing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.setup_training(1e-3, force_objective="energy_gradient")
    eq = object.__new__(EquiformerV2_OC20)
    torch.nn.Module.__init__(eq)
    with pytest.raises(NotImplementedError, match="not offered for EquiformerV2"):
        ForcesTrainer(eq, device="cpu").setup_training(1e-3, force_objective="energy_gradient")


def test_new_c_entries_are_declared_exported_and_reject_null_arguments():
    lib = L.load()
    # declared beside their translation units (csrc/dual_ops.h), bound by lib.py's parser from that text
    assert L.DUAL_HEADER == ROOT / "adsorbdiff_amd" / "csrc" / "dual_ops.h"
    header = L.DUAL_HEADER.read_text()
    from adsorbdiff_amd import build as B

    assert "dual_ops.hip" in B.SOURCES and "message_dual.hip" in B.SOURCES
    assert tuple(L.DUAL_SIGNATURES) == NEW_ENTRIES
    units = "".join((ROOT / "adsorbdiff_amd" / "csrc" / u).read_text() for u in ("dual_ops.hip", "message_dual.hip"))
    for name in NEW_ENTRIES:
        assert hasattr(lib, name) and f" {name}(" in header and f'extern "C" int32_t {name}(' in units, name
        assert getattr(lib, name).restype is C.c_int32 and list(getattr(lib, name).argtypes) == L.DUAL_SIGNATURES[name][1]
    assert "DESIGN.md 6j" in header and "create_graph=True" in header
    f = C.c_float
    E = L.ADF_EINVAL
    assert lib.adf_op_edge_tangent(None, None, None, 4, None) == E
    assert lib.adf_op_rbf_dual(None, None, None, 4, None) == E
    assert lib.adf_op_dual_bias(None, 8, None, 4, 8, None) == E
    assert lib.adf_op_ssilu_dual_fwd(None, None, 8, None) == E
    assert lib.adf_op_ssilu_dual_bwd(None, None, None, 8, None) == E
    assert lib.adf_op_layernorm_dual_fwd(None, None, None, None, None, 4, 128, None) == E
    assert lib.adf_op_layernorm_dual_bwd(None, None, None, None, None, None, None, 4, 128, None, None) == E
    assert lib.adf_op_vdot_dual_fwd(None, None, None, 128, 4, 128, f(1e-8), None) == E
    assert lib.adf_op_vdot_dual_bwd(None, None, 128, None, None, 128, None, None, 4, 128, None) == E
    assert lib.adf_op_update_out_dual_fwd(None, None, None, None, None, f(1), None, None, 4, 128, None) == E
    assert lib.adf_op_update_out_dual_bwd(None, None, None, f(1), None, None, None, None, None, None, None, 4, 128, None) == E
    assert lib.adf_op_message_dual_fwd(None, None, None, None, None, None, None, None, 0, 4, None) == E
    assert lib.adf_op_message_dual_bwd(None, None, None, None, None, None, None, None, None, None, None, 0, 4, None) == E
    assert b"message_dual_bwd" in lib.adf_last_error()
