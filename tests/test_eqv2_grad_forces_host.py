"""CPU side of the EquiformerV2 energy-gradient forces: the float64 yardstick the GPU tests compare against is the derivative
of its own energy (central differences, edges along +y and -y included); ``force_mode`` on the model; the training step
refuses the mode; csrc/eqv2_geo.h, its translation unit and lib.py's table name the same entries."""
import re
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd import lib as L
from tests import helpers_eqv2_grad_forces as G
from tests import helpers_eqv2_s2ef_train as S

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["adf_op_eq_rotate_in_bwd_wig", "adf_op_eq_rotate_out_bwd_wig", "adf_op_eq_radial_gauss_dgrad", "adf_op_eq_wigner_bwd",
           "adf_op_eq_edge_grad_to_atoms"]
# max |F_autograd - F_fd| / max |F| of the yardstick on the 8-atom cluster with a step of 1e-5: measured 8.1e-8 (the
# truncation term (h / sigma)^2 of a basis whose Gaussians are 0.02 wide), times 10
FD_TOL = 1e-6


def test_yardstick_forces_are_the_central_differences_of_its_energy():
    m = S.small_train_model().eval()
    Z, pos, ei = G.pole_cluster()
    along_y = [(pos[s] - pos[d]).tolist() for s, d in ei.t().tolist() if {s, d} == {0, 1}]
    assert sorted(along_y) == [[0.0, -1.5, 0.0], [0.0, 1.5, 0.0]]          # exactly the poles of the device's frame
    off = torch.zeros(ei.shape[1], 3, dtype=torch.float64)
    sysidx = torch.zeros(8, dtype=torch.long)
    _, f = G.energy_and_forces(m, Z, pos, ei, off, sysidx, 1)
    h = 1e-5
    fd = torch.zeros(8, 3, dtype=torch.float64)
    with torch.no_grad():
        for i in range(8):
            for k in range(3):
                up, dn = pos.double().clone(), pos.double().clone()
                up[i, k] += h
                dn[i, k] -= h
                fd[i, k] = -(G.energy_of_pos(m, Z, up, ei, off, sysidx, 1).sum()
                             - G.energy_of_pos(m, Z, dn, ei, off, sysidx, 1).sum()) / (2 * h)
    err = G.rel_force_error(f, fd)
    print(f"yardstick autograd against central differences: {err:.2e} (bound {FD_TOL:.0e}); max|F| {float(f.abs().max()):.3e}")
    assert torch.isfinite(f).all() and float(f.abs().max()) > 0
    assert err < FD_TOL
    assert float(f.sum(0).abs().max()) < 1e-9 * float(f.abs().max())     # a fixed edge set: the forces cancel


def test_force_mode_on_the_model():
    m = S.small_train_model()
    assert type(m).FORCE_MODES == ("direct", "energy_gradient")
    assert m.force_mode == "direct"
    m.force_mode = "energy_gradient"
    assert m.force_mode == "energy_gradient"
    for bad in ("gradient", "", None, "Direct"):
        with pytest.raises(ValueError, match="force_mode must be one of"):
            m.force_mode = bad
    assert m.force_mode == "energy_gradient"
    m.force_mode = "direct"
    assert m.force_mode == "direct"
    assert S.small_train_model(regress_forces=False).force_mode == "direct"


def test_training_step_refuses_the_mode():
    from adsorbdiff_amd.eqv2_train_step import EqV2EnergyGradient, EqV2S2EFTrainStep
    from tests import helpers_eqv2_train as T

    m = S.small_train_model()
    m.force_mode = "energy_gradient"
    with pytest.raises(NotImplementedError, match="needs a second-order backward.*train with force_mode='direct'"):
        EqV2S2EFTrainStep(m, "cpu")
    m.force_mode = "direct"
    with pytest.raises(RuntimeError, match="EqV2S2EFTrainStep needs a ROCm device"):     # as before
        EqV2S2EFTrainStep(m, "cpu")
    with pytest.raises(NotImplementedError, match="differentiates equiformer_v2_oc20.EquiformerV2_OC20"):
        EqV2EnergyGradient(T.train_model("small"), "cpu")
    with pytest.raises(RuntimeError, match="EqV2EnergyGradient needs a ROCm device .*no CPU fallback"):
        EqV2EnergyGradient(m, "cpu")


def test_header_unit_and_binding_name_the_same_entries():
    header = L.GEO_HEADER.read_text()
    assert L.GEO_HEADER == ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_geo.h"
    declared = re.findall(r"\b(adf_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert declared == ENTRIES == list(L.GEO_SIGNATURES)
    assert not set(ENTRIES) & (set(L.EXPORTS) | set(L.TRAIN_SIGNATURES) | set(L.S2EF_TRAIN_SIGNATURES))   # the older tables are as they were
    src = (ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_geo.hip").read_text()
    assert sorted(re.findall(r'extern "C" int32_t (adf_[a-z_0-9]+)\(', src)) == sorted(ENTRIES)
    assert "atomic" not in src.lower()
    # the basis stays defined once: the derivative sits next to the value, the unit restates neither
    gauss = (ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_gauss.h").read_text()
    assert "eq_gauss_dvalue(" in gauss and "eq_gauss_dvalue(" in src and "eq_gauss_window(" in src
    assert "104.0f" not in src and "expf" not in src and '#include "eqv2_gauss.h"' in src
    from adsorbdiff_amd import build as B
    assert "eqv2_geo.hip" in B.SOURCES
    lib = L.load()
    i32, i64, vp = L.C.c_int32, L.C.c_int64, L.C.c_void_p
    for name in ENTRIES:
        assert getattr(lib, name).restype is i32 and list(getattr(lib, name).argtypes) == L.GEO_SIGNATURES[name][1]
    assert lib.adf_op_eq_rotate_out_bwd_wig.argtypes == [vp, vp, vp, i32, i32, vp, vp, i32, i64, vp, vp]
    assert lib.adf_op_eq_radial_gauss_dgrad.argtypes == [vp, vp, vp, i32, vp, i64, vp, vp, i64, vp]
    assert lib.adf_op_eq_edge_grad_to_atoms.argtypes == [vp, vp, vp, vp, i32, i64, vp, vp]
    # null handles and null buffers are refused before anything is launched
    assert lib.adf_op_eq_rotate_in_bwd_wig(None, None, None, None, None, None, 4, None, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_rotate_out_bwd_wig(None, None, None, 1, 1, None, None, -1, 4, None, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_radial_gauss_dgrad(None, None, None, 1, None, 4, None, None, 0, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_wigner_bwd(None, None, None, None, None, 4, None, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_edge_grad_to_atoms(None, None, None, None, 3, 4, None, None) == L.ADF_EINVAL
