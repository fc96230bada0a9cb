"""Learning-rate schedules of the training loop, on the host.

Same interface and values as the reference's ``models/equiformer_v2/trainers/lr_scheduler.py`` (``CosineLRLambda``,
``MultistepLRLambda``, ``LRScheduler(optimizer, optim_config)`` with the keys ``scheduler`` / ``scheduler_params`` and the
``"Null"`` scheduler) and the epochs-to-steps conversion its denoising trainer applies first
(``sde_denoising_trainer.py:238-274``).  The schedule is stepped once per applied optimizer step; the value it leaves in
``optimizer.param_groups[0]["lr"]`` reaches the HIP kernel as an argument, so nothing here touches the device.
"""
from __future__ import annotations

import bisect
import copy
import inspect
import math
from typing import Optional

import torch


def _warmup(step: int, warmup_steps: int, warmup_factor: float) -> float:
    """Linear ramp from ``warmup_factor`` at step 0 to 1 at ``warmup_steps``."""
    alpha = step / float(warmup_steps)
    return warmup_factor * (1.0 - alpha) + alpha


class CosineLRLambda:
    """Warm-up, then half a cosine from 1 down to ``lr_min_factor`` at ``epochs`` (all in steps), flat afterwards."""

    def __init__(self, scheduler_params: dict) -> None:
        self.warmup_epochs = int(scheduler_params["warmup_epochs"])
        self.lr_warmup_factor = float(scheduler_params["warmup_factor"])
        self.max_epochs = int(scheduler_params["epochs"])
        self.lr_min_factor = float(scheduler_params["lr_min_factor"])

    def __call__(self, current_step: int) -> float:
        if current_step <= self.warmup_epochs:
            return _warmup(current_step, self.warmup_epochs, self.lr_warmup_factor)
        if current_step >= self.max_epochs:
            return self.lr_min_factor
        return self.lr_min_factor + 0.5 * (1 - self.lr_min_factor) * (1 + math.cos(math.pi * (current_step / self.max_epochs)))


class MultistepLRLambda:
    """Warm-up, then ``decay_rate`` to the power of the number of ``decay_epochs`` (in steps) already reached."""

    def __init__(self, scheduler_params: dict) -> None:
        self.warmup_epochs = int(scheduler_params["warmup_epochs"])
        self.lr_warmup_factor = float(scheduler_params["warmup_factor"])
        self.lr_decay_epochs = list(scheduler_params["decay_epochs"])
        self.lr_gamma = float(scheduler_params["decay_rate"])

    def __call__(self, current_step: int) -> float:
        if current_step <= self.warmup_epochs:
            return _warmup(current_step, self.warmup_epochs, self.lr_warmup_factor)
        return pow(self.lr_gamma, bisect.bisect(self.lr_decay_epochs, current_step))


def epochs_to_steps(optim_config: dict, steps_per_epoch: int) -> dict:
    """A copy of the ``optim`` block with its ``scheduler_params`` in steps: ``epochs`` is set to ``max_epochs`` and ``lr``
    to ``lr_initial`` (where those keys exist), then every key with "epochs" in its name is multiplied by the steps per
    epoch and truncated to int (lists element by element)."""
    cfg = copy.deepcopy(optim_config)
    sp = cfg.setdefault("scheduler_params", {})
    if "max_epochs" in cfg:
        sp["epochs"] = cfg["max_epochs"]
    if "lr_initial" in cfg:
        sp["lr"] = cfg["lr_initial"]
    for k in list(sp):
        if "epochs" not in k:
            continue
        v = sp[k]
        if isinstance(v, bool):
            continue
        if isinstance(v, (int, float)):
            sp[k] = int(v * steps_per_epoch)
        elif isinstance(v, list):
            sp[k] = [int(x * steps_per_epoch) for x in v]
    return cfg


class LRScheduler:
    """``optim_config["scheduler"]`` names a class of ``torch.optim.lr_scheduler`` (or ``"Null"``: constant rate);
    ``scheduler_params`` holds its arguments (others are ignored).  ``LambdaLR`` takes ``lambda_type`` "cosine" or
    "multistep" and builds the lambda above from the same block."""

    def __init__(self, optimizer, config: dict) -> None:
        self.optimizer = optimizer
        self.config = dict(config)
        if "scheduler" not in self.config or "scheduler_params" not in self.config:
            raise KeyError("the optim block needs `scheduler` and `scheduler_params`")
        self.scheduler_type = str(self.config["scheduler"])
        self.scheduler_params = dict(self.config["scheduler_params"])
        if self.scheduler_type == "LambdaLR":
            self.lambda_type = self.scheduler_params["lambda_type"]
            if self.lambda_type == "cosine":
                fn = CosineLRLambda(self.scheduler_params)
            elif self.lambda_type == "multistep":
                fn = MultistepLRLambda(self.scheduler_params)
            else:
                raise ValueError(f"lambda_type {self.lambda_type!r}: 'cosine' or 'multistep'")
            self.scheduler_params["lr_lambda"] = fn
        self.scheduler = None
        if self.scheduler_type != "Null":
            cls = getattr(torch.optim.lr_scheduler, self.scheduler_type)
            self.scheduler = cls(optimizer, **self.filter_kwargs(cls, self.scheduler_params))

    @staticmethod
    def filter_kwargs(cls, params: dict) -> dict:
        names = [p.name for p in inspect.signature(cls).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        return {k: v for k, v in params.items() if k in names and k != "optimizer"}

    def step(self, metrics=None, epoch=None) -> None:
        if self.scheduler_type == "Null":
            return
        if self.scheduler_type == "ReduceLROnPlateau":
            if metrics is None:
                raise ValueError("ReduceLROnPlateau needs a validation metric")
            self.scheduler.step(metrics)
        else:
            self.scheduler.step()

    def get_lr(self) -> Optional[float]:
        for group in self.optimizer.param_groups:
            return float(group["lr"])
        return None
