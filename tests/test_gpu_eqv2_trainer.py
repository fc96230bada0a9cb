"""``DenoisingTrainer`` on an EquiformerV2 model: ``setup_training`` builds ``EqV2TrainStep``; three ``train_step``s on one
fixed noised batch follow a float64 ``torch.optim.AdamW`` run of the oracle; ``validate`` gives a finite loss; a run stopped
after 2 of 4 steps, saved and resumed in a new trainer ends with the bits of the uninterrupted run (dropout masks included);
``fit_scale_factors`` says that this model has nothing to fit."""
import copy

import pytest
import torch

from tests import helpers_eqv2_train as T
from tests import helpers_train_loop as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=1e-3, weight_decay=0.001, clip_grad_norm=100.0)


def oracle_run(model, batch, targets, graph, dtype, steps=3):
    """``steps`` losses of clip_grad_norm_ + torch.optim.AdamW (weight decay except no_weight_decay()) on a ``dtype`` copy of
    ``model``, the gradients by autograd through the oracle on the fixed edge list."""
    from adsorbdiff_amd.train_step import reference_param_groups

    m = copy.deepcopy(model).cpu().to(dtype)
    opt = torch.optim.AdamW(reference_param_groups(m, HYPER["weight_decay"]), lr=HYPER["lr"])
    losses = []
    for _ in range(steps):
        r = T.reference_step(m, batch, targets, graph, dtype)
        losses.append(float(r["loss"][0]))
        for k, p in m.named_parameters():
            p.grad = None if r["grads"].get(k) is None else r["grads"][k].to(dtype)
        torch.nn.utils.clip_grad_norm_([p for p in m.parameters() if p.grad is not None], HYPER["clip_grad_norm"])
        opt.step()
    return losses


def test_three_train_steps_follow_the_float64_adamw_run_and_validate_is_finite():
    from adsorbdiff_amd.eqv2_train_step import EqV2TrainStep
    from adsorbdiff_amd.train_step import FusedAdamW
    from adsorbdiff_amd.trainer import DenoisingTrainer

    m = T.train_model("small", cutoff=T.SPARSE_CUTOFF)
    cpu_model = copy.deepcopy(m)     # before the trainer binds a device engine to the module
    b, _ = T.sparse_batch()
    b = T.tagged(b)
    targets = T.make_targets(int(b.natoms.numel()))
    for k, v in targets.items():   # a batch that carries its noise and scores: train_step(noised=True)
        setattr(b, k, v)
    tr = DenoisingTrainer(m, device=DEV, config={})
    tr.setup_training(H.NOISE, tables=T.igso3_tables()[0], ema_decay=0.999, **HYPER)
    assert isinstance(tr.train_engine, EqV2TrainStep) and isinstance(tr.optimizer, FusedAdamW)
    bd = b.clone().to(DEV)
    eng = m.engine(DEV)
    _, src, dst, v, _ = eng.export_graph(bd)
    graph = (torch.stack([src.long().cpu(), dst.long().cpu()]), v.cpu())
    r64 = oracle_run(cpu_model, b, targets, graph, torch.float64)
    r32 = oracle_run(cpu_model, b, targets, graph, torch.float32)
    got = []
    for _ in range(3):
        out = tr.train_step(b.clone().to(DEV), noised=True)
        assert not out["skipped"] and not out["stop"]
        got.append(float(out["loss"][0].cpu()))
    assert tr.step == 3
    print("losses  device", got, " float64", r64, " float32 oracle", r32)
    assert abs(got[0] - r64[0]) < 1e-5 * abs(r64[0])
    assert r64[1] != r64[0] and r64[2] != r64[1]
    for i in (1, 2):
        dev32 = abs(r32[i] - r64[i]) / abs(r64[i])
        margin = 10.0 * dev32
        e = abs(got[i] - r64[i]) / abs(r64[i])
        print(f"step {i + 1}: device {e:.2e}  float32 oracle {dev32:.2e}  margin {margin:.2e}")
        assert e < margin, (i, e, margin)
    val = tr.validate([b.clone().to(DEV)], noised=True)
    assert torch.isfinite(torch.tensor(val["loss"]["metric"])) and val["loss"]["metric"] > 0
    with pytest.raises(ValueError, match="nothing to fit"):
        tr.fit_scale_factors([b.clone().to(DEV)])


def _batches():
    out = []
    for b in H.denoising_batches():
        z = b.atomic_numbers.clone()
        z[(z == 36) | (z == 54) | (z >= 85)] = 47.0     # elements without a tabulated radius
        b.atomic_numbers = z
        out.append(b.to(DEV))
    return out


def _trainer(directory, **optim):
    from adsorbdiff_amd.so3_tables import Igso3Tables
    from adsorbdiff_amd.trainer import DenoisingTrainer

    cfg = H.loop_config(directory, max_epochs=1, **optim)
    m = T.train_model("small", alpha_drop=0.1, drop_path_rate=0.1)
    tr = DenoisingTrainer(m, device=DEV, config=cfg)
    tr.setup_training(H.NOISE, lr=2e-4, weight_decay=0.001, clip_grad_norm=100.0, ema_decay=0.999, tables=Igso3Tables.shared(),
                      noise_on_device=True, noise_seed=5, reproducible=True)
    return tr


def test_resumed_run_ends_with_the_bits_of_the_uninterrupted_run(tmp_path):
    from adsorbdiff_amd.train_step import MultiTensorAdamW

    a = _trainer(tmp_path / "a")
    assert isinstance(a.optimizer, MultiTensorAdamW)
    a.train(_batches(), _batches()[:1])
    want = H.training_state(a)
    assert want["step"] == 4 and want["applied"] == 4
    b = _trainer(tmp_path / "b", max_steps=2)
    b.train(_batches(), _batches()[:1])
    assert b.step == 2 and b.train_engine.last_masks is not None and float(b.train_engine.last_masks["alpha"][0].min()) == 0.0
    path = b.save()
    del b
    c = _trainer(tmp_path / "b")
    c.load_checkpoint(path)
    c.train(_batches(), _batches()[:1])
    got = H.training_state(c)
    # the frozen radius table holds NaN for the elements it does not list: compared with the NaNs mapped to a number
    radii = [s.pop("p::atom_radii").nan_to_num(-1.0) for s in (got, want)]
    assert torch.equal(radii[0], radii[1])
    H.assert_same_state(got, want)
