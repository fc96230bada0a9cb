"""Training the PaiNN force field on its energy-gradient forces on the device (PaiNNGradForceTrainStep,
``ForcesTrainer.setup_training(force_objective="energy_gradient")``): the step against the reference's own second-order
autograd (tests/golden/grad_force_train.npz) and against the float64 oracle of tests/helpers_grad_force_train.py on the engine's
graph at ragged shapes, in both arithmetic modes; the energy-only model; a system without a free atom; bit-reproducibility;
``counts=``; ten optimizer steps against torch; resume; and that a direct-force step is left the same bits."""
import copy
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_grad_force_train as HG
from tests import helpers_s2ef_train as HS
from tests import helpers_train_loop as H
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
KW = dict(normalizers=HG.NORMALIZERS, **HG.COEFFICIENTS)


def _step(m, **kw):
    from adsorbdiff_amd.train_step import PaiNNGradForceTrainStep

    return PaiNNGradForceTrainStep(m, DEV, **kw)


def _grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


# ------------------------------------------------------------------------------------------------ the step
def test_step_vs_reference_second_order_autograd():
    """tests/golden/grad_force_train.npz: loss and both terms to 1e-5; ``last_outputs`` bit-equal to ``model(batch)`` in
    energy_gradient mode; every gradient within the 1e-4 training budget (stored entries and norms)."""
    figs = HG.measure_fixture(DEV)
    print("GRADFORCE " + HG.describe(figs, "fixture [default]"))
    assert figs["loss"] < 1e-5 and figs["terms"] < 1e-5, (figs["loss"], figs["terms"])
    HG.assert_step(figs, "fixture")


@pytest.mark.parametrize("name", HG.CONFIG_NAMES)
def test_step_at_ragged_shapes_vs_float64_oracle(name):
    """Whole gradient within 1e-4 relative; per tensor max(1e-4, 4 x the float32 oracle's own error), the widened bound for at
    most two ``update_layers.*.vec_proj.weight`` tensors."""
    figs = HG.measure_configuration(name, DEV)
    print("GRADFORCE " + HG.describe(figs, f"{name} [default]"))
    HG.assert_step(figs, name)


_EXACT_F32_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, {root!r})
from tests import helpers_grad_force_train as HG
for name in ("ragged", "odd_width"):
    print("FIGS " + json.dumps(HG.measure_configuration(name, "cuda:0")), flush=True)
"""


def test_step_with_the_exact_f32_arithmetic():
    """``ragged`` and ``odd_width`` once more under ADF_GEMM=f32 (the handle's exact arithmetic: phase 1) with the step's own
    products exact as well (ADF_TRAIN_GEMM=f32, ADF_WGRAD=f32); the switches are read once per process, hence the child."""
    env = dict(os.environ, ADF_GEMM="f32", ADF_TRAIN_GEMM="f32", ADF_WGRAD="f32")
    res = subprocess.run([sys.executable, "-c", _EXACT_F32_SCRIPT.format(root=str(ROOT))], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    seen = []
    for line in res.stdout.splitlines():
        if line.startswith("FIGS "):
            figs = json.loads(line[5:])
            print("GRADFORCE " + HG.describe(figs, f"{figs['name']} [exact f32]"))
            HG.assert_step(figs, figs["name"])
            seen.append(figs["name"])
    assert seen == ["ragged", "odd_width"]


def test_energy_only_model():
    """regress_forces=False: no force head is needed; the same bounds."""
    figs = HG.measure_configuration("ragged", DEV, regress_forces=False)
    print("GRADFORCE " + HG.describe(figs, "ragged, energy only"))
    HG.assert_step(figs, "energy only")
    assert not any(k.startswith("out_forces") for k in figs["grads"])


def test_system_without_a_free_atom_takes_no_part_in_the_force_term():
    """train_on_free_atoms: every atom of system 1 fixed.  Its rows of dL/dF are zero, so its share of the parameter gradient
    is the energy term's alone; the whole gradient against the oracle, same bounds."""
    m = HG.make_config_model("ragged").to(DEV)
    b = HG.make_config_batch("ragged")
    b.fixed = b.fixed.clone()
    b.fixed[b.batch == 1] = 1
    bd = b.clone().to(DEV)
    edges = HG.engine_edges(m, bd)
    ref = HG.oracle_loss_and_grads(m, b, edges, **KW)
    ref32 = HG.oracle_loss_and_grads(m, b, edges, dtype=torch.float32, **KW)
    figs = HG.measure_step(m, bd, ref, ref32, KW, DEV)
    print("GRADFORCE " + HG.describe(figs, "ragged, system 1 fixed"))
    HG.assert_step(figs, "all fixed system")


def test_reproducible_step_and_batch_independent_forces():
    """Ordered embedding backward: two calls give the same bits for every gradient.  A system's rows of f_pred are the same
    bits alone and inside a batch."""
    m = HG.make_config_model("ragged").to(DEV)
    b = HG.make_config_batch("ragged")
    bd = b.clone().to(DEV)
    step = _step(m, **KW)
    step.ordered_embedding_backward = True
    runs = []
    for _ in range(2):
        step.zero_grad()
        loss = step.loss_and_grad(bd)
        runs.append((loss.clone(), _grads(m)))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    f_batch = step.last_outputs[1].clone()
    data = b.to_data_list()
    o = 0
    for i, d in enumerate(data):
        one = Batch.from_data_list([d])
        n = int(one.pos.shape[0])
        one.energy, one.forces = b.energy[i:i + 1].clone(), b.forces[o:o + n].clone()
        step.zero_grad()
        step.loss_and_grad(one.to(DEV))
        assert torch.equal(step.last_outputs[1], f_batch[o:o + n]), i
        o += n


def test_counts_two_half_batches_add_up_to_the_full_batch():
    """The gradients of two half batches, each with the global counts (systems, free atoms, W = 2: DDPLoss's divisors), averaged
    as the all-reduce averages them, equal the full batch's within 1e-6.  One process, no second rank."""
    m = HG.make_config_model("ragged").to(DEV)
    b = HG.make_config_batch("ragged")
    step = _step(m, **KW)
    step.zero_grad()
    step.loss_and_grad(b.clone().to(DEV))
    full = _grads(m)
    data = b.to_data_list()
    counts = torch.tensor([len(data), int((b.fixed == 0).sum()), 2], dtype=torch.int64, device=DEV)
    step.zero_grad()
    for lo, hi in ((0, 1), (1, len(data))):
        half = Batch.from_data_list(data[lo:hi])
        a0, a1 = int(b.natoms[:lo].sum()), int(b.natoms[:hi].sum())
        half.energy, half.forces = b.energy[lo:hi].clone(), b.forces[a0:a1].clone()
        step.loss_and_grad(half.to(DEV), counts=counts)        # accumulates: the sum over the two ranks
    worst = max((rel_err(g / 2, full[k]), k) for k, g in _grads(m).items())
    print(f"GRADFORCE counts: worst deviation of the averaged half-batch gradients {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 1e-6, worst


# ------------------------------------------------------------------------------------------------ ForcesTrainer
def _trainer(lr, model=None, **kw):
    fx, m, b, step_kw, _ = HG.fixture_case()
    tr = ForcesTrainer(model if model is not None else m, device=DEV, normalizers=step_kw["normalizers"])
    tr.setup_training(lr, energy_coefficient=step_kw["energy_coefficient"], force_coefficient=step_kw["force_coefficient"],
                      force_objective="energy_gradient", **kw)
    return fx, tr, b.to(DEV), step_kw


def test_ten_training_steps_match_torch_adamw_clip_ema_on_oracle_gradients():
    """Ten steps through ``ForcesTrainer.train_step`` on the fixture batch against torch.optim.AdamW + clip_grad_norm_ + the EMA
    mirror driven by the float64 oracle's gradients (engine graph).  Tolerance and learning rate of
    tests/test_gpu_s2ef_train.py's ten-step test: 2e-6 on the parameters and the EMA shadow, 1e-5 on the gradient norm, lr 1e-6."""
    from adsorbdiff_amd.exponential_moving_average import ExponentialMovingAverage
    from adsorbdiff_amd.train_step import PaiNNGradForceTrainStep

    lr, wd, clip, decay = 1e-6, 0.001, 10.0, 0.999
    fx, tr, bd, kw = _trainer(lr, weight_decay=wd, clip_grad_norm=clip, ema_decay=decay)
    assert isinstance(tr.train_engine, PaiNNGradForceTrainStep)
    m = tr._unwrapped_model
    _, ref, b, _, _ = HG.fixture_case()
    edges = HG.engine_edges(m, bd)
    no_decay = set(ref.no_weight_decay())
    groups = [{"params": [p for n, p in ref.named_parameters() if p.requires_grad and n in no_decay], "weight_decay": 0.0},
              {"params": [p for n, p in ref.named_parameters() if p.requires_grad and n not in no_decay], "weight_decay": wd}]
    topt = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    ema_ref = ExponentialMovingAverage(ref.parameters(), decay)
    for it in range(10):
        out = tr.train_step(bd)
        assert not out["skipped"] and not out["stop"] and out["metrics"].shape == (2,)
        r = HG.oracle_loss_and_grads(ref, b, edges, **kw)
        for n, q in ref.named_parameters():
            q.grad = r["grads"][n].float() if n in r["grads"] else None
        gn_ref = torch.nn.utils.clip_grad_norm_([q for q in ref.parameters() if q.grad is not None], max_norm=clip)
        topt.step()
        ema_ref.update()
        assert abs(float(out["grad_norm"]) - float(gn_ref)) < 1e-5 * float(gn_ref), (it, float(out["grad_norm"]), float(gn_ref))
        assert abs(float(out["loss"][0]) - float(r["loss"])) < 1e-5 * float(r["loss"])
    worst = max((rel_err(p.detach().cpu(), q.detach()), n) for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()))
    worst_ema = max(rel_err(s1.cpu(), s2) for s1, s2 in zip(tr.ema.shadow_params, ema_ref.shadow_params))
    print(f"GRADFORCE ten steps at lr {lr}: gradient norm {float(gn_ref):.4g} (clip {clip}), worst parameter error {worst[0]:.2e} "
          f"({worst[1]}), worst EMA error {worst_ema:.2e}")
    assert float(gn_ref) > clip, "the clip is not active: choose a smaller clip_grad_norm"
    assert worst[0] < 2e-6 and worst_ema < 2e-6, (worst, worst_ema)
    assert tr.step == 10


def test_training_lowers_the_force_mae_of_the_gradient_forces_and_validate_reports_it():
    """Ten steps at lr = 1e-3 on one batch (a model WITH a direct head: its parameters keep ``grad is None`` and both
    optimizers skip them): the force MAE of the gradient forces on that batch falls, and ``validate`` on the batch reports
    the MAE of the trained weights (no EMA, so that it evaluates them)."""
    m = HG.make_config_model("ragged")
    head_before = {k: p.detach().clone() for k, p in m.named_parameters() if k.startswith("out_forces.")}
    b = HG.make_config_batch("ragged")
    tr = ForcesTrainer(m, device=DEV, normalizers=copy.deepcopy(HG.NORMALIZERS))
    tr.setup_training(1e-3, ema_decay=0.0, force_objective="energy_gradient", **HG.COEFFICIENTS)
    bd = b.to(DEV)
    first = tr.train_step(bd)
    mae0, loss0 = float(first["metrics"][1]), float(first["loss"][0])
    for _ in range(9):
        tr.train_step(bd)
    assert all(p.grad is None for k, p in m.named_parameters() if k.startswith("out_forces."))
    assert all(torch.equal(p.detach().cpu(), head_before[k]) for k, p in m.named_parameters() if k.startswith("out_forces."))
    tr.train_engine.zero_grad()
    after = tr.train_engine.loss_and_grad(bd)
    mae1, loss1 = float(tr.train_engine.metrics[1]), float(after[0])
    res = tr.validate([bd])
    print(f"GRADFORCE force MAE {mae0:.4f} -> {mae1:.4f}, loss {loss0:.4f} -> {loss1:.4f}; validate forces_mae "
          f"{float(res['forces_mae']['metric']):.4f}")
    assert mae1 < mae0 and loss1 < loss0
    assert abs(float(res["forces_mae"]["metric"]) - mae1) < 1e-5 * mae1
    assert abs(float(res["loss"]["metric"]) - loss1) < 1e-5 * loss1


def _loop_trainer(directory, **optim):
    cfg = H.loop_config(directory, **optim)
    tr = ForcesTrainer(HG.make_config_model("ragged"), device=DEV, normalizers=copy.deepcopy(HG.NORMALIZERS), config=cfg)
    tr.setup_training(lr=2e-4, weight_decay=0.001, clip_grad_norm=10.0, ema_decay=0.999, reproducible=True,
                      force_objective="energy_gradient", **HG.COEFFICIENTS)
    return tr


def test_resumed_run_retraces_the_uninterrupted_run_bit_for_bit(tmp_path):
    """reproducible=True: a run stopped after 3 of 5 steps, saved and resumed in a new trainer ends with the uninterrupted
    run's bits (parameters, moments, EMA shadow, counters)."""
    def batches():
        train = [x.to(DEV) for x in H.s2ef_batches()]
        return train, [x.to(DEV) for x in H.s2ef_batches()][:1]

    a = _loop_trainer(tmp_path / "a", max_steps=5)
    a.train(*batches())
    want = H.training_state(a)
    assert want["step"] == 5 and want["applied"] == 5
    b = _loop_trainer(tmp_path / "b", max_steps=3)
    b.train(*batches())
    assert b.step == 3
    path = b.save()
    del b
    c = _loop_trainer(tmp_path / "b", max_steps=5)
    c.load_checkpoint(path)
    c.train(*batches())
    H.assert_same_state(H.training_state(c), want)


def test_direct_force_step_gives_the_same_bits_before_and_after_a_gradient_force_step():
    """What this objective adds changes nothing for the default: a direct-force ``train_step`` from the same start gives the
    same parameter bits before and after a gradient-force step has run in the same process (reproducible=True, so that the
    embedding gradient has a fixed order)."""
    def direct_step():
        m = HS.make_config_model("ragged")
        tr = ForcesTrainer(m, device=DEV, normalizers=copy.deepcopy(HS.NORMALIZERS))
        tr.setup_training(1e-3, reproducible=True, **HS.COEFFICIENTS)
        tr.train_step(HS.make_config_batch("ragged").to(DEV))
        return {k: p.detach().cpu().clone() for k, p in m.named_parameters()}

    before = direct_step()
    m = HG.make_config_model("ragged")
    tr = ForcesTrainer(m, device=DEV, normalizers=copy.deepcopy(HG.NORMALIZERS))
    tr.setup_training(1e-3, reproducible=True, force_objective="energy_gradient", **HG.COEFFICIENTS)
    tr.train_step(HG.make_config_batch("ragged").to(DEV))
    after = direct_step()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k], after[k]), k
