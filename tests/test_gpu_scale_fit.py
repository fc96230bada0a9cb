"""The scale-factor fit on the GPU: the column-variance kernel (csrc/scale_fit.hip) against float64 torch,
``adf_painn_forward_observe`` and ``fit_scale_factors`` against the reference's own fit loop (tests/golden/scale_fit.npz:
its float64 run is the reference, its float32 run the yardstick printed next to every deviation), and what the trainers do
with fitted factors.

Bounds.  Kernel: 1e-10 relative - float32 inputs are exact in float64 and a two-pass float64 sum over N <= 4096 rows is off
by at most N * 2^-52 ~ 1e-12 relative; the rest is margin for torch's own summation order.  Per-layer variances, fitted
values and variance_out: 1e-4 relative to the reference's float64 record, the project's parity budget for a forward.
Counts (n_samples, variance_in): equal."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.scaling import ensure_fitted, fit_scale_factors, fitted_scale_dict
from adsorbdiff_amd.trainer import DenoisingTrainer, ForcesTrainer
from tests import helpers_scale_fit as S
from tests.helpers import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL_TOL = 1e-10
PARITY = 1e-4
ROWS = (2, 3, 63, 64, 65, 257, 4096)
WIDTHS = (1, 65, 128, 192, 512, 1024)


@pytest.fixture(scope="module")
def fx():
    return load_npz("scale_fit.npz")


@pytest.fixture(scope="module")
def batches():
    return S.make_batches()


# ------------------------------------------------------------------------------------------------ the kernel
def column_variance(x):
    """adf_op_column_variance of a device float32 [N, H] tensor -> the device double"""
    lib = L.load()
    N, H = x.shape
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=x.device)
    scratch = torch.empty(max(int(lib.adf_op_column_variance_scratch(N, H)), 8) // 8, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        L.check(lib.adf_op_column_variance(x.data_ptr(), N, H, out.data_ptr(), scratch.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
    return out


def table(N, H, constant_column, seed):
    """columns with a mean of 100 sigma, sigma between 0.1 and 10 from column to column; one column constant"""
    g = torch.Generator().manual_seed(seed)
    sigma = 10.0 ** (torch.rand(H, generator=g) * 2.0 - 1.0)
    x = (torch.randn(N, H, generator=g) + 100.0) * sigma
    if constant_column is not None:
        x[:, constant_column] = 37.25
    return x.float().contiguous()


@pytest.mark.parametrize("H", WIDTHS)
def test_column_variance_against_float64_torch(H):
    worst = 0.0
    for N in ROWS:
        x = table(N, H, H - 1 if H > 1 else None, seed=1000 * H + N)
        want = float(torch.mean(torch.var(x.double(), dim=0)))
        xd = x.to(DEV)
        a, b = column_variance(xd), column_variance(xd)
        assert a.view(torch.int64).item() == b.view(torch.int64).item(), (N, H)      # run-to-run bit-identical
        err = abs(float(a) / want - 1.0)
        worst = max(worst, err)
        assert err <= KERNEL_TOL, (N, H, float(a), want, err)
        if H % 4 == 0:   # a table that starts 4 bytes off a 16-byte boundary takes the scalar loads: same sums, same bits
            buf = torch.empty(N * H + 1, dtype=torch.float32, device=DEV)
            buf[1:].copy_(xd.reshape(-1))
            c = column_variance(buf[1:].view(N, H))
            assert c.view(torch.int64).item() == a.view(torch.int64).item(), (N, H)
    print(f"H={H}: worst relative error over N in {ROWS}: {worst:.2e}")


@pytest.mark.parametrize("N", ROWS)
def test_constant_columns_have_variance_exactly_zero(N):
    for H in (1, 65, 128):
        x = torch.full((N, H), 37.25) * torch.arange(1, H + 1, dtype=torch.float32)   # every column constant
        assert float(column_variance(x.to(DEV))) == 0.0, (N, H)


def test_one_row_is_an_invalid_argument():
    with pytest.raises(ValueError, match="at least 2 rows"):
        column_variance(torch.ones(1, 128, device=DEV))
    with pytest.raises(ValueError):
        column_variance(torch.ones(0, 128, device=DEV))


# ------------------------------------------------------------------------------------------------ forward_observe
def scale_dict(fx, kind):
    return {n: float(v) for n, v in zip(S.NAMES, fx[f"{kind}_obs_scales"])}


@pytest.fixture(scope="module")
def observed_models(fx):
    """the two models with the fixture's factors in force, on the device (shared by the tests that only read them)"""
    return {kind: S.build_model(kind, scale_file=scale_dict(fx, kind)).to(DEV) for kind in S.MODELS}


@pytest.mark.parametrize("exact", [False, True], ids=["f16x3", "f32"])
@pytest.mark.parametrize("kind", S.MODELS)
def test_forward_observe_against_the_reference_s_layer_variances(fx, batches, kind, exact):
    m = S.build_model(kind, scale_file=scale_dict(fx, kind)).to(DEV)
    eng = m.engine(DEV)
    if exact:
        assert eng.use_exact_f32()
    for i, b in enumerate(batches):
        bd = b.clone().to(DEV)
        var = eng.forward_observe(bd)
        assert var.dtype == torch.float64 and var.shape == (S.L,)
        want, own = fx[f"{kind}_obs_var64"][i], fx[f"{kind}_obs_var32"][i]
        dev = np.abs(var.cpu().numpy() / want - 1)
        print(f"{kind} {'f32' if exact else 'f16x3'} batch {i}: deviation {dev}, the float32 reference's {np.abs(own / want - 1)}")
        assert dev.max() <= PARITY, (kind, i, dev)
        for l in range(S.L):     # stopping after layer l: the same bits up to l, nothing written after it
            part = eng.forward_observe(bd, upto=l)
            assert torch.equal(part[:l + 1].view(torch.int64), var[:l + 1].view(torch.int64)), (kind, i, l)
            assert bool(torch.isnan(part[l + 1:]).all())
    assert eng.exact_f32 == exact     # no silent switch of arithmetic on the way


@pytest.mark.parametrize("kind", S.MODELS)
def test_forward_is_unchanged_by_an_observing_call(observed_models, batches, kind):
    m = observed_models[kind]
    eng = m.engine(DEV)
    bd = batches[0].clone().to(DEV)

    def forward():
        out = m(bd)
        return [out["energy"], out["forces"]] if kind == "s2ef" else list(out)

    before = [t.clone() for t in forward()]
    var, f1, f2 = eng.forward_observe(bd, with_heads=True)      # heads given: the same outputs as forward's
    assert torch.equal(f1, before[-1] if kind == "s2ef" else before[0])
    assert (f2 is None) if kind == "s2ef" else torch.equal(f2, before[1])
    assert torch.equal(eng.forward_observe(bd).view(torch.int64), var.view(torch.int64))      # NULL heads: accepted
    other = batches[2].clone().to(DEV)
    eng.forward_observe(other, upto=0)
    after = forward()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    # under a static-atom promise with kept layer state: the observing call ends it, the next forward computes every row
    if kind == "denoiser":
        prep = eng.prepare(bd)
        eng.set_moving_atoms(prep, bd.tags == 2)
        f1a, f2a = torch.empty_like(before[0]), torch.empty_like(before[1])
        pos = bd.pos.contiguous()
        eng.forward_prepared(prep, pos, f1a, f2a)
        eng.forward_prepared(prep, pos, f1a, f2a)
        eng.forward_observe(other)
        f1b, f2b = torch.empty_like(f1a), torch.empty_like(f2a)
        eng.forward_prepared(prep, pos, f1b, f2b)
        eng.check_flags()
        assert torch.equal(f1a, before[0]) and torch.equal(f2a, before[1])
        assert torch.equal(f1b, before[0]) and torch.equal(f2b, before[1])


def test_forward_observe_argument_checks(observed_models, batches):
    eng = observed_models["denoiser"].engine(DEV)
    bd = batches[1].clone().to(DEV)
    with pytest.raises(ValueError, match="heads need every layer"):
        eng.forward_observe(bd, upto=0, with_heads=True)
    for upto in (-1, S.L):
        with pytest.raises(ValueError, match="upto"):
            eng.forward_observe(bd, upto=upto)
    one = Batch()
    one.pos = torch.tensor([[1.0, 1.0, 1.0]])
    one.atomic_numbers = torch.tensor([29.0])
    one.tags, one.fixed = torch.tensor([2]), torch.tensor([0])
    one.cell = (torch.eye(3) * 4.0).reshape(1, 3, 3)
    one.natoms, one.batch, one.sid = torch.tensor([1]), torch.tensor([0]), ["lonely"]
    with pytest.raises(ValueError, match="at least 2"):
        eng.forward_observe(one.to(DEV))
    m = S.build_model("denoiser").to(DEV)
    with pytest.raises(ValueError, match=r"batch 1 \(sid=\['lonely'\]\)"):
        fit_scale_factors(m, [batches[1], one])


# ------------------------------------------------------------------------------------------------ the fit
def check_fit(res, fx, kind, prefix, names, label):
    assert list(res) == names
    idx = [S.NAMES.index(n) for n in names]
    worst = 0.0
    for n, i in zip(names, idx):
        r = res[n]
        assert r["n_samples"] == int(fx[f"{kind}_{prefix}_n_samples"][i]) and r["variance_in"] == 1.0
        for k in ("value", "variance_out", "ratio"):
            ref64 = float(fx[f"{kind}_{prefix}_{k}"][i])
            dev = abs(r[k] / ref64 - 1)
            own = abs(float(fx[f"{kind}_seq32_{k}"][i]) / float(fx[f"{kind}_seq64_{k}"][i]) - 1)
            print(f"{label} {n} {k}: {r[k]:.9g} reference64 {ref64:.9g} deviation {dev:.2e} (float32 reference's own {own:.2e})")
            worst = max(worst, dev)
            assert dev <= PARITY, (label, n, k, r[k], ref64)
    return worst


@pytest.mark.parametrize("kind", S.MODELS)
def test_fit_against_the_reference_s_fit(fx, batches, kind):
    m = S.build_model(kind).to(DEV)
    m.train()
    getattr(m, S.NAMES[2]).set_(3.0)      # mode "all" resets it
    res = fit_scale_factors(m, batches)
    assert m.training
    check_fit(res, fx, kind, "seq64", S.NAMES, kind)
    ensure_fitted(m)
    assert fitted_scale_dict(m) == {n: float(np.float32(res[n]["value"])) for n in S.NAMES}
    assert m.scale_factors() == [float(np.float32(res[n]["value"])) for n in S.NAMES]
    # sequential, not single-pass, as recorded: the later factors were measured with the earlier ones in force
    got = np.array([res[n]["value"] for n in S.NAMES])
    assert np.abs(got / fx[f"{kind}_single64_value"] - 1).max() > 1e-3
    # a second fit: the same bits
    again = fit_scale_factors(m, batches)
    assert again == res
    # num_batches cuts the list
    first = fit_scale_factors(m, batches, num_batches=1)
    assert [r["n_samples"] for r in first.values()] == [int(batches[0].pos.shape[0])] * S.L
    # the forward with the fitted factors = the forward of a model built around them
    fit_scale_factors(m, batches)
    twin = S.build_model(kind, scale_file=fitted_scale_dict(m)).to(DEV)
    bd = batches[0].clone().to(DEV)
    a, b = m.eval()(bd), twin(bd)
    if kind == "s2ef":
        assert torch.equal(a["energy"], b["energy"]) and torch.equal(a["forces"], b["forces"])
    else:
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("kind", S.MODELS)
def test_mode_unfitted_keeps_the_preset_factor(fx, batches, kind):
    m = S.build_model(kind, scale_file={S.NAMES[1]: S.PRESET}).to(DEV)
    res = fit_scale_factors(m, batches, mode="unfitted")
    check_fit(res, fx, kind, "unf64", [S.NAMES[0], S.NAMES[2]], kind + " unfitted")
    assert float(getattr(m, S.NAMES[1]).scale_factor) == np.float32(S.PRESET)
    assert fit_scale_factors(m, batches, mode="unfitted") == {}
    with pytest.raises(ValueError, match="mode"):
        fit_scale_factors(m, batches, mode="every")


# ------------------------------------------------------------------------------------------------ the trainers
def test_denoising_trainer_fit_validate_checkpoint_and_train_step(fx, batches, tmp_path, caplog):
    from tests import helpers_train as HT

    m = S.build_model("denoiser").to(DEV)
    tr = DenoisingTrainer(m, device=DEV, config={"cmd": {"checkpoint_dir": str(tmp_path)},
                                                 "model_attributes": {"so3_denoising": True}})
    tr.setup_training(dict(ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55), ema_decay=0.999,
                      tables=HT.igso3_tables()[0])
    noised = []
    for i, b in enumerate(batches):
        nb = b.clone()
        for k, v in HT.make_targets(int(b.natoms.numel()), seed=5 + i).items():
            setattr(nb, k, v)
        noised.append(nb)
    with caplog.at_level(logging.WARNING):
        tr.validate([b.clone() for b in noised], noised=True)
    assert "Unfitted scale factors" in caplog.text
    caplog.clear()

    tr.val_loader = batches                     # the default source of the batches
    res = tr.fit_scale_factors()
    check_fit(res, fx, "denoiser", "seq64", S.NAMES, "trainer")
    with caplog.at_level(logging.WARNING):
        tr.validate([b.clone() for b in noised], noised=True)
        tr.predict_denoising(batches[0].clone(), per_image=False)
    assert "Unfitted" not in caplog.text

    path = tr.save()
    fresh = DenoisingTrainer(S.build_model("denoiser").to(DEV), device=DEV)
    assert not getattr(fresh.model, S.NAMES[0]).fitted
    fresh.load_checkpoint(path)
    for n in S.NAMES:
        assert torch.equal(getattr(fresh.model, n).scale_factor, getattr(m, n).scale_factor)
    ensure_fitted(fresh.model)

    torch.manual_seed(9)
    out = tr.train_step(noised[0].clone(), noised=True)
    assert not out["skipped"] and bool(torch.isfinite(out["loss"]).all())
    for n in S.NAMES:                           # frozen parameters: the optimizer leaves them alone
        assert float(getattr(m, n).scale_factor) == np.float32(res[n]["value"])


def test_forces_trainer_fit_and_validate(fx, batches, tmp_path, caplog):
    m = S.build_model("s2ef").to(DEV)
    tr = ForcesTrainer(m, device=DEV, config={"cmd": {"checkpoint_dir": str(tmp_path)}})
    g = torch.Generator().manual_seed(3)
    labelled = []
    for b in batches:
        lb = b.clone()
        lb.energy = torch.randn(int(b.natoms.numel()), generator=g)
        lb.forces = torch.randn(int(b.pos.shape[0]), 3, generator=g)
        labelled.append(lb)
    res = tr.fit_scale_factors(labelled, mode="all")
    check_fit(res, fx, "s2ef", "seq64", S.NAMES, "forces trainer")
    with caplog.at_level(logging.WARNING):
        tr.validate([b.clone() for b in labelled])
        tr.predict(batches[0].clone())
    assert "Unfitted" not in caplog.text
    path = tr.save()
    fresh = ForcesTrainer(S.build_model("s2ef").to(DEV), device=DEV)
    fresh.load_checkpoint(path)
    assert fitted_scale_dict(fresh.model) == fitted_scale_dict(m)
    with pytest.raises(ValueError, match="val_loader"):
        ForcesTrainer(m, device=DEV).fit_scale_factors()
