"""The translation-only (one-head, so3_denoising=False) training step on the GPU: against the float64 oracle on
COM-noised batches (coincident adsorbate atoms), against the reference's autograd (tests/golden/train_tr_only.npz,
tools/make_golden_tr_only.py), and through DenoisingTrainer with the host and the device noising.  Bounds: loss and output
1e-5, every gradient 1e-4 relative - what tests/helpers_train.py::assert_configuration grants the two-head step."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import noising
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.so3_tables import Igso3Tables
from adsorbdiff_amd.train_step import PaiNNTrainStep
from adsorbdiff_amd.trainer import DenoisingTrainer
from tests import helpers_tr_only as HO
from tests import helpers_train as HT
from tests.helpers import batch_from_fixture, load_npz, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", ["ragged", "single", "big_adsorbate"])
def test_one_head_step_vs_float64_oracle(name):
    m, bd, targets, ref = HO.one_head_case(name, DEV)
    ads = (bd.tags == 2).cpu()
    first_system = ads & (bd.batch.cpu() == 0)
    if int(first_system.sum()) > 1:
        rows = bd.pos.cpu()[first_system]
        assert bool((rows == rows[0]).all()), "the adsorbate atoms do not coincide"
    assert not any(k.startswith("out_forces2.") for k, _ in m.named_parameters())
    step = PaiNNTrainStep(m, DEV)
    assert step.igso3 is None                     # the rotation tables are neither needed nor loaded
    step.zero_grad()
    loss = step.loss_and_grad(bd, targets).double().cpu()
    assert len(step.last_outputs) == 1
    e_loss = abs(float(loss[0]) - float(ref["loss"])) / abs(float(ref["loss"]))
    e_out = rel_err(step.last_outputs[0].cpu(), ref["out1"])
    print(f"{name}: loss {float(loss[0]):.6e} rel err {e_loss:.1e}, output {e_out:.1e}")
    assert e_loss < 1e-5 and e_out < 1e-5, (e_loss, e_out)
    assert float(loss[1]) == float(loss[0]) and float(loss[2]) == 0.0
    first, errs = {}, {}
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        g = ref["grads"][k]
        if g is None:
            assert k.startswith("out_energy.") and p.grad is None, k
            continue
        assert p.grad is not None, k
        first[k] = p.grad.clone()
        errs[k] = rel_err(p.grad.cpu(), g)
    worst = max(errs, key=errs.get)
    print(f"{name}: worst gradient {errs[worst]:.2e} ({worst})")
    bad = {k: e for k, e in errs.items() if not e < 1e-4}
    assert not bad, bad
    assert any(k.startswith("out_energy.") for k, _ in m.named_parameters())
    absent = HT.absent_embedding_rows(m, bd)
    assert int(absent.sum()) > 0 and float(first["atom_emb.embeddings.weight"].cpu()[absent].abs().max()) == 0.0
    # a second call: identical bits of the loss and the output, doubled accumulated gradients
    out_first = step.last_outputs[0].clone()
    loss2 = step.loss_and_grad(bd, targets)
    assert torch.equal(loss2.double().cpu(), loss) and torch.equal(step.last_outputs[0], out_first)
    P = dict(m.named_parameters())
    doubling = max(rel_err(P[k].grad, 2 * g1) for k, g1 in first.items())
    assert doubling < 1e-6, doubling


def _fixture_model(fx):
    hp = {k[3:]: fx[k].item() for k in fx if k.startswith("hp_")}
    torch.manual_seed(int(fx["weight_seed"]))
    m = PaiNN(None, 50, 1, hidden_channels=int(hp["hidden_channels"]), num_layers=int(hp["num_layers"]),
              num_rbf=int(hp["num_rbf"]), cutoff=float(hp["cutoff"]), max_neighbors=int(hp["max_neighbors"]), so3_denoising=False,
              scale_file={"upd_out_scalar_scale_%d" % i: float(s) for i, s in enumerate(fx["scale_factors"])})
    g = torch.Generator().manual_seed(int(fx["bias_seed"]))
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if n_.endswith("bias") or "layernorm" in n_:
                p_.add_(0.1 * torch.randn(p_.shape, generator=g))
    HT.trained_like_rescale_(m)
    return m


def test_one_head_step_vs_reference_autograd():
    fx = load_npz("train_tr_only.npz")
    m = _fixture_model(fx).to(DEV)
    b = batch_from_fixture(fx, pos_key="pos_noised", device=DEV)
    targets = {k: torch.from_numpy(fx[k]) for k in ("tr_sigma", "tr_score")}
    step = PaiNNTrainStep(m, DEV)
    step.zero_grad()
    loss = step.loss_and_grad(b, targets).cpu()
    e_out = rel_err(step.last_outputs[0].cpu(), fx["out1"])
    e_loss = abs(float(loss[0]) - float(fx["loss"])) / abs(float(fx["loss"]))
    print(f"reference fixture: loss rel err {e_loss:.1e}, output {e_out:.1e}")
    assert e_out < 1e-5 and e_loss < 1e-5
    P = dict(m.named_parameters())
    assert list(P) == [n.decode() for n in fx["grad_names"]]
    worst, worst_name = 0.0, ""
    for name, gn in zip(fx["grad_names"], fx["grad_norms"]):
        name = name.decode()
        got = P[name].grad
        if not P[name].requires_grad:
            continue
        if gn == 0.0:
            assert got is None or float(got.norm()) == 0.0, name
            continue
        assert abs(float(got.double().norm()) - gn) < 1e-4 * gn, (name, float(got.norm()), gn)
        idx = torch.from_numpy(fx["gidx::" + name])
        ref = torch.from_numpy(fx["gval::" + name]).double()
        e = float((got.reshape(-1).cpu()[idx].double() - ref).norm() / ref.norm())
        if e > worst:
            worst, worst_name = e, name
        assert e < 1e-4, (name, e)
    print(f"reference fixture: worst sampled gradient error {worst:.2e} ({worst_name})")


# ------------------------------------------------------------------------------------------------ DenoisingTrainer
def test_trainer_trains_and_validates_a_one_head_model():
    m = HO.make_one_head_model("ragged")
    tr = DenoisingTrainer(m, DEV)
    assert tr.config["model_attributes"]["so3_denoising"] is False
    tr.setup_training(HO.PARAMS, lr=1e-4)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    torch.manual_seed(3)
    out = tr.train_step(HT.make_config_batch("ragged"))
    assert set(out) == {"loss", "grad_norm", "skipped", "stop"} and out["skipped"] is False and out["stop"] is False
    assert out["loss"].shape == (3,) and bool(torch.isfinite(out["loss"]).all()) and float(out["loss"][2]) == 0.0
    assert float(out["grad_norm"]) > 0 and tr.step == 1
    changed = [k for k, p in m.named_parameters() if not torch.equal(p.detach(), before[k])]
    assert changed and all(not k.startswith("out_energy.") for k in changed)
    assert any(k.startswith("out_forces.") for k in changed)


def test_trainer_validate_one_head_is_the_mean_of_the_oracle_losses():
    m = HO.make_one_head_model("ragged")
    tr = DenoisingTrainer(m, DEV, config={"optim": {"denoising_pos_params": HO.PARAMS}})   # validate stands alone
    want = []
    batches = []
    for i, name in enumerate(("ragged", "single", "big_adsorbate")):
        torch.manual_seed(60 + i)
        b = noising.ads_COM_gaussian_schedule(HT.make_config_batch(name), HO.PARAMS)
        bd = b.clone().to(DEV)
        eng = tr._unwrapped_model.engine(DEV)
        eng.build_graph(bd)
        targets = {"tr_sigma": b.tr_sigma, "tr_score": b.tr_score}
        want.append(float(HO.oracle_one_head(m, b, targets, HT.graph_from_export(eng))["loss"]))
        batches.append(b)
    res = tr.validate(batches, noised=True)
    assert set(res) == {"loss"} and set(res["loss"]) == {"metric", "total", "numel"}
    assert res["loss"]["numel"] == 3
    mean = sum(want) / 3
    print(f"validate: {res['loss']['metric']:.8e} oracle mean {mean:.8e}")
    assert abs(res["loss"]["metric"] - mean) < 1e-5 * abs(mean)
    # un-noised batches go through the COM schedule of the host
    torch.manual_seed(9)
    res2 = tr.validate([HT.make_config_batch("ragged")])
    assert res2["loss"]["numel"] == 1 and np.isfinite(res2["loss"]["metric"]) and res2["loss"]["metric"] > 0


def _two_head_trainer(noise_on_device, tables):
    m = HT.make_config_model("ragged")
    tr = DenoisingTrainer(m, DEV)
    tr.setup_training(HO.PARAMS, lr=1e-4, tables=tables, noise_on_device=noise_on_device, noise_seed=11)
    return m, tr


def test_trainer_device_noising_equals_the_host_function_of_the_same_rows():
    tables = Igso3Tables.shared()
    b0 = HT.make_config_batch("ragged")
    rows, redrawn = HO.safe_rows(b0, HO.PARAMS, seed=70, kinds=("tr_so3",))
    assert redrawn <= 1
    # device noising inside the step, from the supplied rows
    m_dev, tr_dev = _two_head_trainer(True, tables)
    tr_dev.optimizer.lr = 0.0                      # keep the weights: the gradients are what is compared
    out_dev = tr_dev.train_step(b0.clone(), draws=rows)
    g_dev = {k: p.grad.clone() for k, p in m_dev.named_parameters() if p.grad is not None}
    # host function of the same rows, then the step on the noised batch
    m_host, tr_host = _two_head_trainer(False, tables)
    tr_host.optimizer.lr = 0.0
    nb = noising.tr_so3_schedule_from_draws(b0.clone(), HO.PARAMS, rows, tables)
    out_host = tr_host.train_step(nb, noised=True)
    g_host = {k: p.grad.clone() for k, p in m_host.named_parameters() if p.grad is not None}
    l_dev, l_host = out_dev["loss"].double().cpu(), out_host["loss"].double().cpu()
    print("device-noised loss", l_dev.tolist(), "host-noised loss", l_host.tolist())
    assert float((l_dev - l_host).abs().max()) < 1e-5 * float(l_host[0].abs())
    assert set(g_dev) == set(g_host)
    errs = {k: rel_err(g_dev[k], g_host[k]) for k in g_host}
    worst = max(errs, key=errs.get)
    print(f"worst gradient difference {errs[worst]:.2e} ({worst})")
    assert errs[worst] < 1e-4, (worst, errs[worst])
    # the counter numbers the calls; noise_step overrides it; draws= / noise_step= need the option
    assert tr_dev.noise_step == 0
    tr_dev.train_step(b0.clone())
    assert tr_dev.noise_step == 1
    a = tr_dev.train_step(b0.clone(), noise_step=5)["loss"]
    b = tr_dev.train_step(b0.clone(), noise_step=5)["loss"]
    assert torch.equal(a, b) and tr_dev.noise_step == 1
    with pytest.raises(ValueError, match="noise_on_device"):
        tr_host.train_step(b0.clone(), draws=rows)
    res = tr_dev.validate([b0.clone(), b0.clone()], noise_step=5)
    assert res["loss"]["numel"] == 2 and np.isfinite(res["loss"]["metric"])


def test_trainer_host_noising_leaves_the_generators_where_the_schedule_leaves_them():
    """noise_on_device off (the default): train_step consumes the torch and numpy streams exactly as
    noising.tr_so3_schedule alone does - one number drawn from each afterwards tells."""
    tables = Igso3Tables.shared()
    b0 = HT.make_config_batch("ragged")

    def after(run):
        torch.manual_seed(123)
        np.random.seed(123)
        run()
        return (float(torch.rand(1, device=DEV)), float(torch.rand(1)), float(np.random.rand()))

    want = after(lambda: noising.tr_so3_schedule(b0.clone().to(DEV), HO.PARAMS, tables))
    seen = []
    for _ in range(2):
        _, tr = _two_head_trainer(False, tables)
        seen.append(after(lambda: tr.train_step(b0.clone())))
    assert seen[0] == want and seen[1] == want, (seen, want)
