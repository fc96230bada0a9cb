"""``ForcesTrainer`` on the EquiformerV2 S2EF force field: ``setup_training`` builds ``EqV2S2EFTrainStep``; three
``train_step``s on one batch follow a float64 ``torch.optim.AdamW`` run of the oracle; a NaN target skips the update;
``validate`` gives the eight S2EF metrics and the loss; with ``reproducible=True`` and masks on, a run stopped after 2 of 4
steps, saved and resumed in a new trainer ends with the bits of the uninterrupted run."""
import copy

import pytest
import torch

from tests import helpers_eqv2_s2ef_train as S
from tests import helpers_train_loop as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=1e-3, weight_decay=0.001, clip_grad_norm=10.0)
STEP_KW = dict(normalizers=S.NORMALIZERS, **S.COEFFICIENTS)


def _trainer(m, **kw):
    from adsorbdiff_amd.trainer import ForcesTrainer

    tr = ForcesTrainer(m, device=DEV, normalizers=copy.deepcopy(S.NORMALIZERS), config=kw.pop("config", None))
    tr.setup_training(ema_decay=0.999, **S.COEFFICIENTS, **dict(HYPER, **kw))
    return tr


def test_three_train_steps_follow_the_float64_adamw_run_skip_and_validate():
    from adsorbdiff_amd.eqv2_train_step import EqV2S2EFTrainStep
    from adsorbdiff_amd.evaluator import Evaluator
    from adsorbdiff_amd.train_step import FusedAdamW

    m = S.small_train_model()
    cpu_model = copy.deepcopy(m)     # before the trainer binds a device engine to the module
    b, ei, vec, _ = S.fixture_case()
    tr = _trainer(m)
    assert isinstance(tr.train_engine, EqV2S2EFTrainStep) and isinstance(tr.optimizer, FusedAdamW)
    norm = tr._objective()["norm"]
    assert norm["energy"] == pytest.approx((-0.7, 1.9)) and norm["forces"] == pytest.approx((0.15, 2.1))
    m.engine(DEV).set_edges(ei, vec)
    r64 = S.oracle_run(cpu_model, b, (ei, vec), torch.float64, HYPER, STEP_KW)
    r32 = S.oracle_run(cpu_model, b, (ei, vec), torch.float32, HYPER, STEP_KW)
    # a NaN target: the parameters stay, the step is reported as skipped and does not count
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    bad = b.clone()
    bad.energy = bad.energy.clone()
    bad.energy[0] = float("nan")
    out = tr.train_step(bad.to(DEV))
    assert out["skipped"] and not out["stop"] and out["grad_norm"] is None and tr.step == 0
    assert all(torch.equal(p.detach(), before[k]) for k, p in m.named_parameters())
    got = []
    for _ in range(3):
        out = tr.train_step(b.clone().to(DEV))
        assert not out["skipped"] and not out["stop"] and out["metrics"] is not None
        got.append(float(out["loss"][0].cpu()))
    assert tr.step == 3
    print("losses  device", got, " float64", r64, " float32 oracle", r32)
    assert abs(got[0] - r64[0]) < 1e-5 * abs(r64[0])
    assert r64[1] != r64[0] and r64[2] != r64[1]
    for i in (1, 2):
        dev32 = abs(r32[i] - r64[i]) / abs(r64[i])
        margin = S.TIGHT_FACTOR * dev32
        e = abs(got[i] - r64[i]) / abs(r64[i])
        print(f"step {i + 1}: device {e:.2e}  float32 oracle {dev32:.2e}  margin {margin:.2e}  hard {S.REL_TOL:.0e}")
        assert e < S.REL_TOL and e < margin, (i, e, margin)
    val = tr.validate([b.clone().to(DEV)])
    assert set(val) == set(Evaluator(task="s2ef").metric_names()) | {"loss"} and len(val) == 9
    assert all(torch.isfinite(torch.tensor(float(v["metric"]))) for v in val.values()) and val["loss"]["metric"] > 0
    with pytest.raises(ValueError, match="nothing to fit"):
        tr.fit_scale_factors([b.clone().to(DEV)])


def _batches():
    out = []
    for b in H.s2ef_batches():
        z = b.atomic_numbers.clone()
        z[z >= 85] = 47.0     # inside the model's element tables
        b.atomic_numbers = z
        out.append(b.to(DEV))
    return out


def _loop_trainer(directory, **optim):
    cfg = H.loop_config(directory, max_epochs=1, **optim)
    m = S.small_train_model(alpha_drop=0.1, drop_path_rate=0.1)
    return _trainer(m, config=cfg, reproducible=True, mask_seed=5, lr=2e-4)


def test_resumed_run_ends_with_the_bits_of_the_uninterrupted_run(tmp_path):
    from adsorbdiff_amd.train_step import MultiTensorAdamW

    a = _loop_trainer(tmp_path / "a")
    assert isinstance(a.optimizer, MultiTensorAdamW) and a.train_engine.mask_seed == 5
    a.train(_batches(), _batches()[:1])
    want = H.training_state(a)
    assert want["step"] == 4 and want["applied"] == 4
    b = _loop_trainer(tmp_path / "b", max_steps=2)
    b.train(_batches(), _batches()[:1])
    assert b.step == 2 and b.train_engine.last_masks is not None and float(b.train_engine.last_masks["alpha"][0].min()) == 0.0
    path = b.save()
    del b
    c = _loop_trainer(tmp_path / "b")
    c.load_checkpoint(path)
    c.train(_batches(), _batches()[:1])
    H.assert_same_state(H.training_state(c), want)
