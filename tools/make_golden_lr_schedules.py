"""Records tests/golden/lr_schedules.npz from the reference's own scheduler module.

    python tools/make_golden_lr_schedules.py

Needs the reference checkout that oracle/refshim finds (like oracle/make_golden.py).  Imports
``adsorbdiff.models.equiformer_v2.trainers.lr_scheduler`` from it and stores, for the parameters of
``configs/denoising/painn_so3.yml`` (cosine) and one multistep set:

  <name>_params_json     the ``optim`` block before the conversion (what the test feeds to ``epochs_to_steps``)
  <name>_converted_json  its ``scheduler_params`` after the reference's epochs-to-steps conversion
                         (``DenoisingTrainer.load_extras``, sde_denoising_trainer.py:238-274)
  <name>_steps           the steps compared: 0, 1, warm-up - 1, warm-up, warm-up + 1, max - 1, max, max + 5 (+ the decay
                         boundaries of the multistep set)
  <name>_lambda          the reference lambda at those steps (float64)
  <name>_lr              the learning rate ``LRScheduler`` + ``torch.optim.SGD`` leave in the optimizer after that many
                         ``step()`` calls (float64)

The conversion is the reference's own method: its source is parsed out of the trainer module (which cannot be imported
without the reference's whole dependency tree) and run on a stand-in object that has the attributes the method reads.
"""
from __future__ import annotations

import argparse
import ast
import copy
import importlib.util
import json
import logging
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import refshim  # noqa: E402

refshim.install()

# loaded by file: the package around it imports the whole EquiformerV2 model
_spec = importlib.util.spec_from_file_location(
    "reference_lr_scheduler",
    Path(refshim.REFERENCE_ROOT) / "adsorbdiff" / "models" / "equiformer_v2" / "trainers" / "lr_scheduler.py")
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

STEPS_PER_EPOCH = 37

CASES = {
    "cosine": {   # configs/denoising/painn_so3.yml:54-66
        "lr_initial": 1.0e-4, "max_epochs": 100, "scheduler": "LambdaLR",
        "scheduler_params": {"lambda_type": "cosine", "warmup_factor": 0.2, "warmup_epochs": 4, "lr_min_factor": 0.01},
    },
    "multistep": {
        "lr_initial": 4.0e-4, "max_epochs": 10, "scheduler": "LambdaLR",
        "scheduler_params": {"lambda_type": "multistep", "warmup_factor": 0.1, "warmup_epochs": 2,
                             "decay_epochs": [3, 5.5, 8], "decay_rate": 0.3},
    },
}


def reference_load_extras():
    """``DenoisingTrainer.load_extras`` compiled from the reference's source."""
    src = (Path(refshim.REFERENCE_ROOT) / "adsorbdiff" / "trainers" / "sde_denoising_trainer.py").read_text()
    for node in ast.parse(src).body:
        if isinstance(node, ast.ClassDef) and node.name == "DenoisingTrainer":
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == "load_extras":
                    ns = {"logging": logging, "LRScheduler": ref.LRScheduler, "ExponentialMovingAverage": lambda *a, **k: None}
                    exec(compile(ast.Module(body=[sub], type_ignores=[]), "<reference load_extras>", "exec"), ns)
                    return ns["load_extras"]
    raise RuntimeError("DenoisingTrainer.load_extras not found in the reference")


def convert(optim: dict, n_iter_per_epoch: int):
    """(converted optim block, the LRScheduler the reference built on an SGD optimizer) by the reference's method."""
    optim = copy.deepcopy(optim)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=optim["lr_initial"])
    fake = types.SimpleNamespace(config={"optim": optim}, train_loader=range(n_iter_per_epoch), optimizer=opt,
                                 model=torch.nn.Linear(1, 1))
    reference_load_extras()(fake)
    return fake.config["optim"], opt, fake.scheduler


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "lr_schedules.npz"))
    a = ap.parse_args()

    out = {"steps_per_epoch": np.int64(STEPS_PER_EPOCH)}
    for name, optim in CASES.items():
        conv, opt, sched = convert(optim, STEPS_PER_EPOCH)
        sp = conv["scheduler_params"]
        w, mx = sp["warmup_epochs"], sp["epochs"]
        steps = [0, 1, w - 1, w, w + 1, mx - 1, mx, mx + 5]
        if name == "multistep":
            for d in sp["decay_epochs"]:
                steps += [d - 1, d, d + 1]
        steps = sorted(set(steps))
        fn = (ref.CosineLRLambda if name == "cosine" else ref.MultistepLRLambda)(sp)
        lam = np.array([fn(s) for s in steps], dtype=np.float64)
        # the learning rate the reference's LRScheduler leaves in an optimizer after s steps
        lrs = {}
        for s in range(max(steps) + 1):
            if s in steps:
                lrs[s] = sched.get_lr()
            opt.step()
            sched.step()
        out[f"{name}_params_json"] = np.array(json.dumps(optim))
        out[f"{name}_converted_json"] = np.array(json.dumps(sp))
        out[f"{name}_steps"] = np.array(steps, dtype=np.int64)
        out[f"{name}_lambda"] = lam
        out[f"{name}_lr"] = np.array([lrs[s] for s in steps], dtype=np.float64)
    np.savez(a.out, **out)
    print(a.out, {k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
