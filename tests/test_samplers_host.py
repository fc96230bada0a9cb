"""Host side of the translation-only samplers (Denoiser.reverse_sde_sampling / langevin_dynamics): schedule tables
against the values the reference recorded (tools/make_golden_samplers.py), parameter validation, and the C entries'
argument checks.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.denoising_torch import Denoiser, langevin_coefs, ode_tr_coefs, schedule_coefs
from tests.helpers import load_npz

ODE_CASES = ["ode_large", "ode_mild", "ode_early"]
LGV_CASES = ["lgv_1head", "lgv_2head"]


def _params(fx):
    p = dict(num_steps=int(fx["num_steps"]), ads_std_low=0.1, ads_std_high=10)
    if fx["sampler"].item() == b"langevin":
        p.update(n_step_each=int(fx["n_step_each"]), step_lr=float(fx["step_lr"]))
    return p


@pytest.mark.parametrize("name", LGV_CASES)
def test_langevin_table_is_bit_equal_to_the_reference_recording(name):
    fx = load_npz(f"sampler_{name}.npz")
    coefs = langevin_coefs(_params(fx))
    assert len(coefs) == int(fx["num_steps"]) * int(fx["n_step_each"]) == fx["ref_step_size"].shape[0]
    got = np.array([[c.coef, c.noise] for c in coefs], dtype=np.float32)
    assert np.array_equal(got[:, 0], fx["ref_step_size"])
    assert np.array_equal(got[:, 1], fx["ref_noise_scale"])


@pytest.mark.parametrize("name", ODE_CASES)
def test_ode_table_equals_the_rot_samplers_translation_coefficient(name):
    fx = load_npz(f"sampler_{name}.npz")
    p = _params(fx)
    coefs = ode_tr_coefs(p)
    ref = schedule_coefs(dict(p, rot_std_low=0.01, rot_std_high=1.55, ode=True))
    assert [c.coef for c in coefs] == [c.coef_tr for c in ref]
    assert all(c.noise == 0.0 for c in coefs)


def test_ode_table_reproduces_the_recorded_unwrapped_step():
    """Where the reference's step did not cross the cell boundary, dcom_xy == f32(coef * score) up to the rounding of the
    wrap (com + d -> fractional -> cell.f - com)."""
    fx = load_npz("sampler_ode_mild.npz")
    coefs = ode_tr_coefs(_params(fx))
    for t, c in enumerate(coefs):
        raw = (torch.tensor(c.coef, dtype=torch.float32) * torch.from_numpy(fx["ref_score"][t])).numpy()
        np.testing.assert_allclose(fx["ref_dcom"][t][:, :2], raw[:, :2], rtol=0, atol=2e-5)


class _Unwrapped:
    otf_graph = True


class _Trainer:
    _unwrapped_model = _Unwrapped()


class _Calc:
    model = _Trainer()


@pytest.mark.parametrize("missing", ["n_step_each", "step_lr"])
def test_langevin_requires_its_keys(missing):
    params = dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, n_step_each=2, step_lr=1e-5)
    del params[missing]
    den = Denoiser(object(), _Calc(), params, device="cuda:0")
    with pytest.raises(KeyError):
        den.langevin_dynamics()
    with pytest.raises(KeyError):
        Denoiser(object(), _Calc(), dict(params, sampler="langevin"), device="cuda:0").run()


def test_unknown_sampler_is_rejected():
    den = Denoiser(object(), _Calc(), dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, sampler="ddim"),
                   device="cuda:0")
    with pytest.raises(ValueError, match="sampler"):
        den.run()


@pytest.mark.parametrize("sampler", ["sde", "langevin"])
def test_samplers_are_a_no_op_without_ads_std_low(sampler):
    batch = object()
    den = Denoiser(batch, _Calc(), dict(num_steps=3, sampler=sampler), device="cuda:0")
    assert den.run() is batch
    assert den.steps_applied == 0
    den.reverse_sde_sampling()
    den.langevin_dynamics()


def test_translation_entries_reject_null_and_bad_arguments():
    lib = L.load()
    for name in ("adf_tr_step", "adf_tr_sample", "adf_tr_sample_traj", "adf_eqv2_tr_step", "adf_eqv2_tr_sample",
                 "adf_eqv2_tr_sample_traj"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    desc = L.BatchDesc()
    coef = L.TrCoef()
    # null handle / null descriptor
    assert lib.adf_tr_step(None, ctypes.byref(desc), None, None, None, ctypes.byref(coef), None, 1, None, 0, None, None,
                           None) == L.ADF_EINVAL
    assert lib.adf_tr_step(None, None, None, None, None, None, None, 0, None, 0, None, None, None) == L.ADF_EINVAL
    assert lib.adf_tr_sample(None, ctypes.byref(desc), None, None, None, 4, None, 0, 0, None, None, 0, None,
                             None) == L.ADF_EINVAL
    assert lib.adf_tr_sample_traj(None, ctypes.byref(desc), None, None, None, 4, None, 0, 0, None, None, 0, None, None,
                                  1, None) == L.ADF_EINVAL
    assert lib.adf_eqv2_tr_step(None, ctypes.byref(desc), None, None, None, ctypes.byref(coef), None, 1, None, 0, None,
                                None, None) == L.ADF_EINVAL
    assert lib.adf_eqv2_tr_sample(None, ctypes.byref(desc), None, None, None, 4, None, 0, 0, None, None, 0, None,
                                  None) == L.ADF_EINVAL
    assert lib.adf_eqv2_tr_sample_traj(None, ctypes.byref(desc), None, None, None, 4, None, 0, 0, None, None, 0, None,
                                       None, 1, None) == L.ADF_EINVAL
    assert lib.adf_last_error()
