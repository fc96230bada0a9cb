"""Host side of train(): the schedules against values recorded from the reference's module
(tests/golden/lr_schedules.npz, tools/make_golden_lr_schedules.py), the mapping between torch.optim.AdamW's state and the
multi-tensor optimizer's flat moments, the checkpoint's key set, the generator round trip and the best-checkpoint rule."""
import copy
import json

import numpy as np
import pytest
import torch

from adsorbdiff_amd import noising
from adsorbdiff_amd import train_loop as TL
from adsorbdiff_amd.lr_scheduler import CosineLRLambda, LRScheduler, MultistepLRLambda, epochs_to_steps
from adsorbdiff_amd.so3_tables import Igso3Tables
from adsorbdiff_amd.train_step import adamw_state_to_flat, flat_to_adamw_state, reference_param_groups
from tests import helpers_tr_only as HO
from tests import helpers_train as HT
from tests import helpers_train_loop as H
from tests.helpers import load_npz


# ------------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("name", ["cosine", "multistep"])
def test_schedule_values_equal_the_reference_module(name):
    fx = load_npz("lr_schedules.npz")
    spe = int(fx["steps_per_epoch"])
    optim = json.loads(str(fx[f"{name}_params_json"]))
    conv = epochs_to_steps(optim, spe)
    # the conversion: every *epochs* key times the steps per epoch, epochs = max_epochs
    assert conv["scheduler_params"] == json.loads(str(fx[f"{name}_converted_json"]))
    assert "epochs" not in optim["scheduler_params"]   # the input is not modified
    sp = conv["scheduler_params"]
    steps = [int(s) for s in fx[f"{name}_steps"]]
    w, mx = sp["warmup_epochs"], sp["epochs"]
    assert {0, 1, w - 1, w, w + 1, mx - 1, mx, mx + 5} <= set(steps)
    fn = (CosineLRLambda if name == "cosine" else MultistepLRLambda)(sp)
    got = np.array([fn(s) for s in steps], dtype=np.float64)
    assert np.array_equal(got, fx[f"{name}_lambda"]), (got - fx[f"{name}_lambda"])   # exact in double
    # the same through LRScheduler and a torch optimizer, stepped once per step
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=conv["lr_initial"])
    sched = LRScheduler(opt, conv)
    lrs = {}
    for s in range(max(steps) + 1):
        if s in steps:
            lrs[s] = sched.get_lr()
        opt.step()
        sched.step()
    assert np.array_equal(np.array([lrs[s] for s in steps]), fx[f"{name}_lr"])


def test_null_scheduler_and_plateau():
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.5)
    null = LRScheduler(opt, {"scheduler": "Null", "scheduler_params": {}})
    null.step()
    assert null.get_lr() == 0.5 and null.scheduler is None
    plateau = LRScheduler(opt, {"scheduler": "ReduceLROnPlateau", "scheduler_params": {"factor": 0.5, "patience": 0, "lr": 1}})
    with pytest.raises(ValueError, match="validation"):
        plateau.step()
    plateau.step(metrics=1.0)
    plateau.step(metrics=2.0)
    assert plateau.get_lr() == 0.25
    with pytest.raises(ValueError, match="lambda_type"):
        LRScheduler(opt, {"scheduler": "LambdaLR", "scheduler_params": {"lambda_type": "linear"}})


# ------------------------------------------------------------------------------------------------ optimizer state mapping
def _two_steps():
    m = H.FiveTensors()
    groups = reference_param_groups(m, 0.01)
    names = dict((id(p), n) for n, p in m.named_parameters())
    assert [[names[id(p)] for p in g["params"]] for g in groups] == [["b", "e"], ["a", "c", "d"]]
    assert [g["weight_decay"] for g in groups] == [0, 0.01]
    assert len(reference_param_groups(m, 0.0)) == 1
    opt = torch.optim.AdamW(groups, lr=1e-2)
    for k in range(2):
        opt.zero_grad(set_to_none=True)
        m.loss(k).backward()
        assert m.d.grad is None
        opt.step()
    return m, opt


def test_adamw_state_maps_to_flat_moments_and_back():
    m, opt = _two_steps()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]   # b, e, a, c: `d` (index 4) never had a gradient
    step, moments, groups = adamw_state_to_flat(sd)
    assert step == 2 and sorted(moments) == [0, 1, 2, 3]
    assert torch.equal(moments[2][0], opt.state[m.a]["exp_avg"]) and torch.equal(moments[2][1], opt.state[m.a]["exp_avg_sq"])
    back = flat_to_adamw_state(step, moments, groups)
    assert back["param_groups"] == sd["param_groups"]
    assert sorted(back["state"]) == sorted(sd["state"])
    for i, e in sd["state"].items():
        assert set(back["state"][i]) == set(e) == {"step", "exp_avg", "exp_avg_sq"}
        for k in e:
            assert back["state"][i][k].dtype == e[k].dtype and torch.equal(back["state"][i][k], e[k]), (i, k)
    # and torch takes it back: the next step of a fresh AdamW from the mapped state equals the original's next step
    m2 = H.FiveTensors()
    m2.load_state_dict(m.state_dict())
    opt2 = torch.optim.AdamW(reference_param_groups(m2, 0.01), lr=1e-2)
    opt2.load_state_dict(copy.deepcopy(back))   # state_dict() hands out the optimizer's own tensors
    for mm, oo in ((m, opt), (m2, opt2)):
        oo.zero_grad(set_to_none=True)
        mm.loss(2).backward()
        oo.step()
    for p, q in zip(m.parameters(), m2.parameters()):
        assert torch.equal(p, q)


def test_unequal_steps_raise():
    _, opt = _two_steps()
    sd = opt.state_dict()
    sd["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="one counter"):
        adamw_state_to_flat(sd)
    assert adamw_state_to_flat({"state": {}, "param_groups": []})[0] == 0


# ------------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_has_the_reference_keys_plus_noise_step_and_rng(tmp_path):
    tr = H.HostTrainer(tmp_path)
    tr.setup_scheduler(4)
    full = tr.checkpoint_dict(metrics={"loss": {"metric": 1.0}})
    assert set(full) == set(TL.REFERENCE_CHECKPOINT_KEYS) | {"noise_step", "rng"}
    assert len(TL.REFERENCE_CHECKPOINT_KEYS) == 12
    assert full["amp"] is None and full["scheduler"] is None and full["noise_step"] == 11 and full["step"] == 3
    assert full["primary_metric"] == "loss" and full["best_val_metric"] == 0.5
    assert set(full["optimizer"]) == {"state", "param_groups"} and set(full["rng"]) == {"torch_cpu", "torch_device", "numpy"}
    assert set(full["ema"]) >= {"decay", "num_updates", "shadow_params"}
    # weights only: the EMA weights, nothing of the training state
    with torch.no_grad():
        for s in tr.ema.shadow_params:
            s.add_(1.0)
    before = {k: v.clone() for k, v in tr.model.state_dict().items()}
    best = tr.checkpoint_dict(training_state=False)
    assert set(best) == {"state_dict", "normalizers", "config", "val_metrics", "amp"} and "optimizer" not in best
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, before[k]) and torch.equal(best["state_dict"][k], before[k] + 1.0), k
    # written under a temporary name and renamed; the reference's loader reads it as a plain dict
    path = tr.save(checkpoint_file="checkpoint.pt")
    assert path == str(tmp_path / "checkpoint.pt") and sorted(p.name for p in tmp_path.iterdir()) == ["checkpoint.pt"]
    assert set(torch.load(path, map_location="cpu", weights_only=False)) == set(full)


def test_checkpoint_carries_a_scheduler_state_and_load_puts_the_rate_back(tmp_path):
    tr = H.HostTrainer(tmp_path)
    tr.config["optim"].update(lr_initial=1e-3, scheduler="LambdaLR",
                              scheduler_params={"lambda_type": "cosine", "warmup_factor": 0.2, "warmup_epochs": 1,
                                                "lr_min_factor": 0.01})
    tr.setup_scheduler(4)
    for _ in range(3):
        tr.optimizer.step()
        tr.scheduler.step()
    lr = tr.scheduler.get_lr()
    path = tr.save()
    new = H.HostTrainer(tmp_path)
    new.config["optim"] = tr.config["optim"]
    new.load_checkpoint(path)           # before the scheduler exists: kept until setup_scheduler
    new.setup_scheduler(4)
    assert new.scheduler.get_lr() == lr and new.scheduler.scheduler.last_epoch == 3
    assert new.step == 3 and new.noise_step == 11 and new.best_val_metric == 0.5 and new.primary_metric == "loss"
    tr.scheduler.step()
    new.scheduler.step()
    assert new.scheduler.get_lr() == tr.scheduler.get_lr()


def test_host_noising_continues_its_streams_after_an_rng_round_trip(tmp_path):
    tables = Igso3Tables.shared()
    b0 = HT.make_config_batch("ragged")
    torch.manual_seed(123)
    np.random.seed(321)
    noising.tr_so3_schedule(b0.clone(), HO.PARAMS, tables)
    state = TL.capture_rng("cpu")
    torch.save({"rng": state}, tmp_path / "rng.pt")
    want = noising.tr_so3_schedule(b0.clone(), HO.PARAMS, tables)
    torch.manual_seed(999)   # the streams move on
    np.random.seed(999)
    torch.rand(7)
    TL.restore_rng(torch.load(tmp_path / "rng.pt", weights_only=False)["rng"], "cpu")
    got = noising.tr_so3_schedule(b0.clone(), HO.PARAMS, tables)
    for key in ("pos", "tr_sigma", "rot_sigma", "tr_score", "rot_score"):
        assert torch.equal(getattr(got, key), getattr(want, key)), key


# ------------------------------------------------------------------------------------------------ best checkpoint
def test_update_best_follows_the_reference_rule_in_both_directions(tmp_path):
    # "mae" in the name: smaller is better
    tr = H.HostTrainer(tmp_path, eval_metrics={"primary_metric": "energy_mae"})
    tr.best_val_metric = TL.initial_best("energy_mae")
    assert tr.best_val_metric == 1e9
    tr.update_best("energy_mae", {"energy_mae": {"metric": 2.0}})
    tr.update_best("energy_mae", {"energy_mae": {"metric": 3.0}})
    assert tr.best_val_metric == 2.0 and (tmp_path / "best_checkpoint.pt").exists()
    assert torch.load(tmp_path / "best_checkpoint.pt", weights_only=False)["val_metrics"] == {"energy_mae": {"metric": 2.0}}
    # no "mae" in the name: larger is better - the reference keeps the checkpoint with the LARGEST loss
    tr = H.HostTrainer(tmp_path / "loss")
    tr.best_val_metric = TL.initial_best("loss")
    assert tr.best_val_metric == -1.0
    tr.update_best("loss", {"loss": {"metric": 2.0}})
    tr.update_best("loss", {"loss": {"metric": 1.0}})
    tr.update_best("loss", {"loss": {"metric": 3.0}})
    assert tr.best_val_metric == 3.0
    assert torch.load(tmp_path / "loss" / "best_checkpoint.pt", weights_only=False)["val_metrics"]["loss"]["metric"] == 3.0


def test_update_best_min_override(tmp_path):
    tr = H.HostTrainer(tmp_path, eval_metrics={"primary_metric": "loss", "primary_metric_mode": "min"})
    tr.best_val_metric = TL.initial_best("loss", "min")
    assert tr.best_val_metric == 1e9
    tr.update_best("loss", {"loss": {"metric": 2.0}})
    tr.update_best("loss", {"loss": {"metric": 3.0}})
    tr.update_best("loss", {"loss": {"metric": 1.0}})
    assert tr.best_val_metric == 1.0
    with pytest.raises(ValueError, match="primary_metric_mode"):
        TL.is_better("loss", 1.0, 2.0, "smallest")
