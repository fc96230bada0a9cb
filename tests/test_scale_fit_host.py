"""Host side of the scale-factor fit (adsorbdiff_amd/scaling.py): the ``ScaleFactor`` protocol and the generic loop of
``fit_scale_factors`` against what the reference's own classes gave on the same plain-torch inputs
(tests/golden/scale_fit.npz, tools/make_golden_scale_fit.py), the scale-file round trip and the C ABI of the two entries."""
import json
import logging

import numpy as np
import pytest
import torch

from adsorbdiff_amd import scaling
from adsorbdiff_amd.scaling import ScaleFactor, ensure_fitted, fit_scale_factors
from tests import helpers_scale_fit as S
from tests.helpers import load_npz

# The stand-in runs float32 Linear layers on the CPU.  The reference's run of it was made with the same torch calls, but a
# matrix product may be summed in another order by another CPU build: 3 stages of 24-wide products, each within a few
# float32 roundings (6e-8), give at most ~1e-6 relative on a variance.  The protocol test, which involves torch.var /
# torch.mean on small tensors only, asks for equality.
STANDIN_TOL = 1e-6


@pytest.fixture(scope="module")
def fx():
    return load_npz("scale_fit.npz")


def test_protocol_equals_the_reference_on_the_same_tensors(fx):
    f = ScaleFactor()
    assert f.stats is None and f.index_fn is None and not f.fitted
    calls = []
    f.initialize_(index_fn=lambda: calls.append(1))
    with f.fit_context_():
        for t in S.standin_batches():
            assert f(t) is t                   # unfitted: the identity
        assert f.stats["variance_out"] == float(fx["proto_acc_variance_out"])
        assert f.stats["n_samples"] == int(fx["proto_acc_n_samples"]) == f.stats["variance_in"]
        stats, ratio, value = f.fit_()
    assert len(calls) == 4
    assert f.stats is None
    assert stats["variance_out"] == float(fx["proto_variance_out"]) and stats["n_samples"] == int(fx["proto_n_samples"])
    assert stats["variance_in"] == 1.0
    assert ratio == float(fx["proto_ratio"]) and value == float(fx["proto_value"])
    assert f.fitted and float(f.scale_factor) == np.float32(value)
    # fitted: multiplies, and observes the product
    f.initialize_(index_fn=None)
    t = S.standin_batches()[0]
    with f.fit_context_():
        y = f(t)
        assert torch.equal(y, t * f.scale_factor)
        assert f.stats["variance_out"] == torch.mean(torch.var(y, dim=0)).item() * t.shape[0]
    # ref= is accepted: variance_in is then the reference tensor's statistic
    with f.fit_context_():
        f(t, ref=2.0 * t)
        assert f.stats["variance_in"] == torch.mean(torch.var(2.0 * t, dim=0)).item() * t.shape[0]


def test_default_forward_is_what_it_was():
    f = ScaleFactor()
    t = torch.randn(5, 3)
    assert f(t) is t
    f.set_(0.5)
    assert torch.equal(f(t), t * 0.5)
    assert torch.equal(f(t[:1]), t[:1] * 0.5)      # one row is fine outside a fit
    assert f.stats is None


def test_fit_without_a_context_raises():
    f = ScaleFactor()
    with pytest.raises((ValueError, AssertionError)):
        f.fit_()
    with f.fit_context_():                          # a context without an observation: every stat is 0
        with pytest.raises((ValueError, AssertionError)):
            f.fit_()


def _check(res, fx, prefix, names):
    assert list(res) == names
    for i, n in enumerate(names):
        r = res[n]
        assert set(r) == {"variance_in", "variance_out", "n_samples", "ratio", "value"}
        assert r["n_samples"] == int(fx[prefix + "_n_samples"][i]) and r["variance_in"] == 1.0
        for k in ("variance_out", "ratio", "value"):
            ref = float(fx[f"{prefix}_{k}"][i])
            assert abs(r[k] / ref - 1) <= STANDIN_TOL, (n, k, r[k], ref)


def test_generic_loop_on_a_torch_module_mode_all(fx):
    net = S.StandIn()
    net.scale_2.set_(3.0)          # mode "all" resets it
    net.train()
    res = fit_scale_factors(net, S.standin_batches())
    _check(res, fx, "standin_all", ["scale_0", "scale_1", "scale_2"])
    assert net.training            # the mode it was in comes back
    for k in range(3):
        m = getattr(net, "scale_%d" % k)
        assert m.index_fn is None and m.stats is None
        assert float(m.scale_factor) == np.float32(res["scale_%d" % k]["value"])
    ensure_fitted(net)
    # sequential is not single-pass: the later factors see the earlier ones
    assert abs(res["scale_1"]["value"] - res["scale_0"]["value"]) > 1e-3
    # num_batches cuts the loader; a one-shot iterator is read once
    two = fit_scale_factors(S.StandIn(), iter(S.standin_batches()), num_batches=2)
    assert [r["n_samples"] for r in two.values()] == [19, 19, 19]


def test_generic_loop_mode_unfitted_keeps_the_preset_factor(fx):
    net = S.StandIn()
    net.scale_1.set_(S.PRESET)
    res = fit_scale_factors(net, S.standin_batches(), mode="unfitted")
    assert list(res) == ["scale_0", "scale_2"]
    assert float(net.scale_1.scale_factor) == np.float32(S.PRESET) == np.float32(fx["standin_unf_value"][1])
    for i, n in ((0, "scale_0"), (2, "scale_2")):
        for k in ("variance_out", "ratio", "value"):
            assert abs(res[n][k] / float(fx[f"standin_unf_{k}"][i]) - 1) <= STANDIN_TOL
    assert fit_scale_factors(net, S.standin_batches(), mode="unfitted") == {}   # nothing left to fit


def test_one_row_batch_and_unknown_mode_raise():
    net = S.StandIn()
    bad = S.standin_batches()[:2] + [torch.randn(1, 24)]
    with pytest.raises(ValueError, match="batch 2"):
        fit_scale_factors(net, bad)
    assert all(getattr(net, "scale_%d" % k).stats is None for k in range(3))
    with pytest.raises(ValueError, match="mode"):
        fit_scale_factors(net, S.standin_batches(), mode="some")
    with pytest.raises(ValueError):
        fit_scale_factors(net, [])


@pytest.mark.parametrize("suffix", [".pt", ".json"])
def test_scale_file_round_trip(tmp_path, suffix, caplog):
    net = S.StandIn()
    with pytest.raises(ValueError, match="Unfitted"):
        scaling.save_scale_file(net, tmp_path / ("early" + suffix))
    res = fit_scale_factors(net, S.standin_batches())
    path = scaling.save_scale_file(net, tmp_path / ("scales" + suffix))
    assert scaling.fitted_scale_dict(net) == {n: float(np.float32(r["value"])) for n, r in res.items()}
    if suffix == ".json":
        assert json.loads(path.read_text()) == scaling.fitted_scale_dict(net)
    other = S.StandIn()
    with caplog.at_level(logging.WARNING):
        ensure_fitted(other, warn=True)
    assert "Unfitted scale factors" in caplog.text
    caplog.clear()
    scaling.load_scales_compat(other, path)
    with caplog.at_level(logging.WARNING):
        ensure_fitted(other, warn=True)
        ensure_fitted(other)
    assert "Unfitted" not in caplog.text
    for k in range(3):
        assert torch.equal(getattr(other, "scale_%d" % k).scale_factor, getattr(net, "scale_%d" % k).scale_factor)
    with pytest.raises(ValueError, match="extension"):
        scaling.save_scale_file(net, tmp_path / "scales.txt")


def test_mirror_models_hold_the_fixture_s_weights(fx):
    for kind in S.MODELS:
        sums = S.weight_sums(S.build_model(kind)).numpy()
        np.testing.assert_array_equal(sums, fx[f"{kind}_sums"])
        # the recorded fit is sequential, and says so: one pass for all factors gives other values
        seq, single = fx[f"{kind}_seq64_value"], fx[f"{kind}_single64_value"]
        assert np.abs(single / seq - 1).max() > 1e-3 and np.abs(seq - 1).min() > 1e-3


def test_c_abi_of_the_two_entries():
    import ctypes as C

    from adsorbdiff_amd import lib as L

    # the section "Scale-factor fit" of include/adsorbdiff_hip.h declares exactly these three, in this order, bound from its text
    names = ["adf_op_column_variance_scratch", "adf_op_column_variance", "adf_painn_forward_observe"]
    at = L.EXPORTS.index(names[0])
    assert list(L.EXPORTS[at:at + len(names)]) == names
    sig = {name: L.SIGNATURES[name] for name in names}
    assert sig["adf_op_column_variance_scratch"] == (C.c_int64, [C.c_int64, C.c_int32])
    assert sig["adf_op_column_variance"] == (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
    rt, at = sig["adf_painn_forward_observe"]
    assert rt is C.c_int32 and len(at) == 7 and at[2] is C.c_int32 and at[1] is C.POINTER(L.BatchDesc)
    lib = L.load()
    for name, (restype, argtypes) in sig.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # host arithmetic only: bytes for R chunk partials + the means, R = ceil(N / 64) capped at 256
    assert lib.adf_op_column_variance_scratch(2, 1) == 8 * 2
    assert lib.adf_op_column_variance_scratch(65, 128) == 8 * 3 * 128
    assert lib.adf_op_column_variance_scratch(10 ** 6, 512) == 8 * 257 * 512
    assert lib.adf_op_column_variance_scratch(0, 128) == 0 and lib.adf_op_column_variance_scratch(5, 0) == 0
    # argument checks come before any device work
    assert lib.adf_op_column_variance(None, 4, 4, None, None, None) == L.ADF_EINVAL
    assert lib.adf_painn_forward_observe(None, None, 0, None, None, None, None) == L.ADF_EINVAL
