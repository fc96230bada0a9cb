"""CPU side of the EquiformerV2 S2EF training step: the float32 statement of the training oracle reproduces the reference
model's own recordings (so the GPU tests compare against the reference's forward, not against a restatement of the code
under test); the None / identically-zero pattern of the float64 autograd; csrc/eqv2_s2ef_train.h, its translation unit and
lib.py's table name the same entries; ``ForcesTrainer.setup_training`` dispatches and refuses as documented."""
import re
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd import lib as L
from tests import helpers_eqv2_s2ef_train as S
from tests.helpers import rel_err, row_rel_err

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["adf_op_eq_edge_dist", "adf_op_eq_radial_gauss_fwd", "adf_op_eq_radial_gauss_bwd"]


def test_float32_oracle_reproduces_the_reference_recordings():
    """energy, energy with the linear reference, per-atom energies and forces of the fixture's small case on its recorded
    edge list, within REL_TOL."""
    b, ei, vec, cx = S.fixture_case()
    m = S.small_train_model(perturb=False)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        e, ea, f = S.forward_s2ef(sd, S.hp_of(m), b.atomic_numbers, (ei, vec), torch.float32, b.batch.long(), 2)
        e_ref, _, _ = S.forward_s2ef(sd, dict(S.hp_of(m), use_energy_lin_ref=True, regress_forces=False), b.atomic_numbers,
                                     (ei, vec), torch.float32, b.batch.long(), 2)
    figs = dict(energy=row_rel_err(e.reshape(-1, 1), torch.from_numpy(cx["energy"]).reshape(-1, 1)),
                energy_lin_ref=row_rel_err(e_ref.reshape(-1, 1), torch.from_numpy(cx["energy_lin_ref"]).reshape(-1, 1)),
                atom_energy=rel_err(ea, cx["atom_energy"]), forces=rel_err(f, cx["forces"]))
    print("float32 training oracle against the reference's recordings:", {k: f"{v:.2e}" for k, v in figs.items()})
    assert all(v < S.REL_TOL for v in figs.values()), figs
    assert not torch.equal(e, e_ref)


def test_none_and_zero_pattern_of_the_float64_autograd():
    """No parameter is left at None; the parts of energy_block the l = 0 output does not depend on, the rows l >= 1 of
    so3_linear_2.weight and section 6g's two force-block gradients are zero tensors; everything else is live.  Without
    the force block, the same without its parameters."""
    b, ei, vec, _ = S.fixture_case()
    for kw in (dict(), dict(regress_forces=False)):
        m = S.small_train_model(**kw)
        ref = S.reference_step(m, b, (ei, vec), normalizers=S.NORMALIZERS, **S.COEFFICIENTS)
        pattern = S.expected_zero_pattern(m)
        assert any(k.startswith(S.DEAD) for k in pattern) and "energy_block.so3_linear_2.weight" in pattern
        assert ("force_block.proj.bias" in pattern) == (not kw)
        assert "energy_lin_ref" not in ref["grads"]
        for k, g in ref["grads"].items():
            assert g is not None, k
            if pattern.get(k) == "zero":
                assert float(g.abs().max()) == 0.0, k
            elif pattern.get(k) == "rows":
                assert float(g[1:].abs().max()) == 0.0 and float(g[0].abs().max()) > 0.0, k
            elif not kw and k != "energy_block.so3_linear_2.bias":
                # (energy alone: the l >= 1 rows of the last block never reach it, more gradients are zero tensors)
                # (the bias' gradient is sum_b sign(residual_b) n_b / B / avg_num_nodes: two systems of one size whose
                # residuals differ in sign cancel exactly)
                assert float(g.abs().max()) > 0.0, k
        assert (ref["forces"] is None) == bool(kw)
        if kw:
            assert float(ref["loss"][2]) == 0.0 and float(ref["loss"][0]) == float(ref["loss"][1])


def test_header_unit_and_binding_name_the_same_entries():
    header = L.S2EF_TRAIN_HEADER.read_text()
    assert L.S2EF_TRAIN_HEADER == ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_s2ef_train.h"
    declared = re.findall(r"\b(adf_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert declared == ENTRIES == list(L.S2EF_TRAIN_SIGNATURES)
    assert not set(ENTRIES) & (set(L.EXPORTS) | set(L.TRAIN_SIGNATURES))      # the two older tables are as they were
    src = (ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_s2ef_train.hip").read_text()
    assert sorted(re.findall(r'extern "C" int32_t (adf_[a-z_0-9]+)\(', src)) == sorted(ENTRIES)
    assert "atomic" not in src.lower()
    # the basis is defined once, in the header both units include
    gauss = (ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_gauss.h").read_text()
    kernels = (ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_kernels.hip").read_text()
    assert "104.0f" in gauss and "104.0f" not in src and '#include "eqv2_gauss.h"' in src and '#include "eqv2_gauss.h"' in kernels
    assert "eq_gauss_window(" in src and "eq_gauss_value(" in src and "eq_gauss_window(" in kernels and "eq_gauss_value(" in kernels
    from adsorbdiff_amd import build as B
    assert "eqv2_s2ef_train.hip" in B.SOURCES
    lib = L.load()
    i32, i64, vp = L.C.c_int32, L.C.c_int64, L.C.c_void_p
    for name in ENTRIES:
        assert getattr(lib, name).restype is i32 and list(getattr(lib, name).argtypes) == L.S2EF_TRAIN_SIGNATURES[name][1]
    assert lib.adf_op_eq_radial_gauss_fwd.argtypes == [vp, vp, vp, i32, i64, vp, vp, i64, vp]
    assert lib.adf_op_eq_radial_gauss_bwd.argtypes == [vp, vp, vp, vp, i64, vp, i32, vp, i64, vp]
    # null handles and null buffers are refused before anything is launched
    assert lib.adf_op_eq_edge_dist(None, 4, None, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_radial_gauss_fwd(None, None, None, 1, 4, None, None, 0, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_radial_gauss_bwd(None, None, None, None, 4, None, 1, None, 0, None) == L.ADF_EINVAL


def test_forces_trainer_dispatch_and_refusals():
    from adsorbdiff_amd.painn import PaiNN
    from adsorbdiff_amd.trainer import ForcesTrainer
    from tests import helpers_eqv2_train as T

    import inspect
    assert inspect.signature(ForcesTrainer.setup_training).parameters["mask_seed"].default == 0
    eq = S.small_train_model()
    # the loss names are looked at first, whatever the model
    for model in (eq, PaiNN(None, 50, 1, hidden_channels=32, num_layers=1, num_rbf=32)):
        with pytest.raises(NotImplementedError, match="energy loss 'mae' with force loss 'l2mae'"):
            ForcesTrainer(model, device="cpu").setup_training(lr=1e-3, loss_energy="mse")
    with pytest.raises(RuntimeError, match="EqV2S2EFTrainStep needs a ROCm device .*no CPU fallback"):
        ForcesTrainer(eq, device="cpu").setup_training(lr=1e-3)
    with pytest.raises(RuntimeError, match="PaiNNS2EFTrainStep needs a ROCm device .*no CPU fallback"):
        ForcesTrainer(PaiNN(None, 50, 1, hidden_channels=32, num_layers=1, num_rbf=32), device="cpu").setup_training(lr=1e-3)
    den = T.train_model("small")
    with pytest.raises(NotImplementedError, match="the denoiser's step is PaiNNTrainStep"):
        ForcesTrainer(den, device="cpu").setup_training(lr=1e-3)
    # each step names the other model's
    from adsorbdiff_amd.eqv2_train_step import EqV2S2EFTrainStep, EqV2TrainStep
    with pytest.raises(NotImplementedError, match="EqV2S2EFTrainStep"):
        EqV2TrainStep(eq, "cpu")
    with pytest.raises(NotImplementedError, match="trains equiformer_v2_oc20.EquiformerV2_OC20"):
        EqV2S2EFTrainStep(den, "cpu")
    with pytest.raises(ValueError, match="nothing to fit"):
        ForcesTrainer(eq, device="cpu").fit_scale_factors([])
