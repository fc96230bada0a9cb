"""The epoch loop, checkpoints and best-checkpoint selection both trainers share.

``TrainLoopMixin`` gives ``DenoisingTrainer`` and ``ForcesTrainer``:

  ``train(train_batches, val_batches)``   the loop of the reference's ``sde_denoising_trainer.py:370-537`` and of
                                          ``ocp_trainer.py``'s twin around ``train_step`` / ``validate``
  ``save(metrics, checkpoint_file, training_state)``   the reference's checkpoint keys (``base_trainer.py:625-684``) plus
                                          ``noise_step`` and ``rng``
  ``load_checkpoint(path)``               weights as before; with training set up also optimizer, scheduler, EMA, counters
  ``update_best(primary_metric, val_metrics)``   ``base_trainer.py:686-704``

Everything here runs on the host and only reads attributes (``model``, ``optimizer``, ``ema``, ``config`` ...), so the
checkpoint layout and the selection rule are testable without a device.

Two places where the loop leaves the reference, both so that a run resumed from ``checkpoint.pt`` retraces the
uninterrupted run bit for bit (with ``setup_training(reproducible=True)`` and ``noise_on_device=True``):

* on resume the first ``step % len(train_batches)`` batches of the epoch are skipped (the reference restarts its iterator
  at batch 0);
* ``checkpoint.pt`` is written at the end of an iteration, after the scheduler step and the validation of that iteration
  (the reference writes it before both, so its file holds the schedule of the step before and misses that validation).
"""
from __future__ import annotations

import logging
import os
from typing import Iterable, Optional

import numpy as np
import torch

from .lr_scheduler import LRScheduler, epochs_to_steps

REFERENCE_CHECKPOINT_KEYS = ("epoch", "step", "state_dict", "optimizer", "scheduler", "normalizers", "config", "val_metrics",
                             "ema", "amp", "best_val_metric", "primary_metric")
EXTRA_CHECKPOINT_KEYS = ("noise_step", "rng")


def capture_rng(device=None) -> dict:
    """The states of the generators host noising draws from: torch CPU, torch device (None without one), numpy global."""
    dev = torch.device(device) if device is not None else None
    on_device = dev is not None and dev.type == "cuda" and torch.cuda.is_available()
    return {"torch_cpu": torch.get_rng_state(), "torch_device": torch.cuda.get_rng_state(dev) if on_device else None,
            "numpy": np.random.get_state()}


def restore_rng(state: dict, device=None) -> None:
    torch.set_rng_state(state["torch_cpu"].cpu())
    dev = torch.device(device) if device is not None else None
    if state.get("torch_device") is not None and dev is not None and dev.type == "cuda" and torch.cuda.is_available():
        torch.cuda.set_rng_state(state["torch_device"].cpu(), dev)
    np.random.set_state(state["numpy"])


def is_better(primary_metric: str, value, best, mode: Optional[str] = None) -> bool:
    """The reference's rule (``base_trainer.py:692-698``): smaller is better iff "mae" is in the metric's name, larger
    otherwise - so with ``primary_metric: loss`` the LARGEST loss is kept.  ``mode`` ("min" / "max",
    ``eval_metrics["primary_metric_mode"]``) overrides the rule."""
    if mode not in (None, "min", "max"):
        raise ValueError(f"primary_metric_mode {mode!r}: 'min' or 'max'")
    smaller = ("mae" in primary_metric) if mode is None else (mode == "min")
    return value < best if smaller else value > best


def initial_best(primary_metric: str, mode: Optional[str] = None) -> float:
    smaller = ("mae" in primary_metric) if mode is None else (mode == "min")
    return 1e9 if smaller else -1.0


def _is_master() -> bool:
    import torch.distributed as dist

    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


class TrainLoopMixin:
    # ---------------------------------------------------------------- configuration
    @property
    def evaluation_metrics(self) -> dict:
        return self.config.get("eval_metrics", {}) or {}

    def _task_name(self) -> str:
        return getattr(self, "name", "ocp")

    def _primary_metric_name(self) -> Optional[str]:
        from .evaluator import Evaluator

        return self.evaluation_metrics.get("primary_metric", Evaluator.task_primary_metric.get(self._task_name()))

    def setup_scheduler(self, steps_per_epoch: int) -> None:
        """``self.scheduler`` from ``config["optim"]`` (``scheduler``, ``scheduler_params``, ``max_epochs``, ``lr_initial``;
        no ``scheduler`` key: "Null"), its epochs turned into steps.  A scheduler state that ``load_checkpoint`` met before
        the scheduler existed is loaded now."""
        optim = dict(self.config.get("optim", {}))
        optim.setdefault("scheduler", "Null")
        optim.setdefault("scheduler_params", {})
        optim = epochs_to_steps(optim, steps_per_epoch)
        if optim["scheduler"] != "Null" and not isinstance(self.optimizer, torch.optim.Optimizer):
            raise NotImplementedError(
                f"scheduler {optim['scheduler']!r} needs setup_training(reproducible=True): FusedAdamW keeps a fixed "
                "learning rate (scheduler 'Null')")
        self.scheduler = LRScheduler(self.optimizer, optim)
        pending = getattr(self, "_pending_scheduler_state", None)
        if pending is not None and self.scheduler.scheduler is not None:
            self._load_scheduler_state(pending)
        self._pending_scheduler_state = None

    def _load_scheduler_state(self, state: dict) -> None:
        sched = self.scheduler.scheduler
        sched.load_state_dict(state)
        # building a torch scheduler sets the groups' rates to its step-0 values: put back the ones that were saved
        last = getattr(sched, "_last_lr", None)
        if last is not None:
            for group, lr in zip(self.optimizer.param_groups, last):
                group["lr"] = lr

    # ---------------------------------------------------------------- scale factors
    def fit_scale_factors(self, batches: Optional[Iterable] = None, num_batches: int = 16, mode: str = "all") -> dict:
        """Fit the model's ``ScaleFactor``s as the reference's ``modules/scaling/fit.py`` does (``scaling.fit_scale_factors``):
        the first ``num_batches`` of ``batches`` (default ``val_loader``) as they are - not noised -, the current weights
        (no EMA swap), one factor after the other on the device.  The factors are parameters, so ``save()`` writes them;
        afterwards ``validate`` / ``predict`` no longer warn about unfitted factors.  -> ``{name: {"variance_in",
        "variance_out", "n_samples", "ratio", "value"}}``."""
        from .scaling import ScaleFactor, fit_scale_factors

        if not any(isinstance(m, ScaleFactor) for m in self._unwrapped_model.modules()):
            raise ValueError(f"fit_scale_factors: {type(self._unwrapped_model).__name__} has no scale factors: "
                             "there is nothing to fit for this model")
        if batches is None:
            batches = getattr(self, "val_loader", None)
            if batches is None:
                raise ValueError("fit_scale_factors: no batches given and the trainer has no val_loader")
        return fit_scale_factors(self._unwrapped_model, batches, num_batches=num_batches, mode=mode, device=self.device)

    # ---------------------------------------------------------------- checkpoints
    def checkpoint_dict(self, metrics=None, training_state: bool = True) -> dict:
        """What ``save`` writes.  ``training_state=True``: the reference's twelve keys plus ``noise_step`` (the counter of
        the device noising) and ``rng`` (``capture_rng``: host noising continues its streams).  ``False``: the EMA weights
        as ``state_dict``, without optimizer, scheduler or counters."""
        normalizers = {k: v.state_dict() for k, v in (getattr(self, "normalizers", None) or {}).items()}
        if not training_state:
            if self.ema is not None:
                self.ema.store()
                self.ema.copy_to()
            try:
                weights = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
            finally:
                if self.ema is not None:
                    self.ema.restore()
            return {"state_dict": weights, "normalizers": normalizers, "config": self.config, "val_metrics": metrics,
                    "amp": None}
        scheduler = getattr(self, "scheduler", None)
        sched_state = None
        if scheduler is not None and scheduler.scheduler_type != "Null":
            sched_state = scheduler.scheduler.state_dict()
        elif getattr(self, "_pending_scheduler_state", None) is not None:
            sched_state = self._pending_scheduler_state
        optimizer = getattr(self, "optimizer", None)
        # the optimizer first: its state_dict() reads the device counter and refreshes ema.num_updates from it
        opt_state = optimizer.state_dict() if hasattr(optimizer, "state_dict") else None
        return {
            "epoch": getattr(self, "epoch", 0), "step": getattr(self, "step", 0), "state_dict": self.model.state_dict(),
            "optimizer": opt_state, "scheduler": sched_state, "normalizers": normalizers, "config": self.config,
            "val_metrics": metrics, "ema": self.ema.state_dict() if self.ema else None, "amp": None,
            "best_val_metric": getattr(self, "best_val_metric", None), "primary_metric": self._primary_metric_name(),
            "noise_step": getattr(self, "noise_step", 0), "rng": capture_rng(getattr(self, "device", None)),
        }

    def save(self, metrics=None, checkpoint_file: str = "checkpoint.pt", training_state: bool = True) -> Optional[str]:
        """Writes ``checkpoint_dict`` to ``config["cmd"]["checkpoint_dir"]`` on rank 0 (a temporary name, then a rename);
        returns the path, None on the other ranks."""
        if not _is_master():
            return None
        ckpt = self.checkpoint_dict(metrics, training_state)
        directory = self.config["cmd"]["checkpoint_dir"]
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, checkpoint_file)
        tmp = path + ".tmp"
        torch.save(ckpt, tmp)
        os.replace(tmp, path)
        return path

    def load_checkpoint(self, checkpoint_path: str) -> None:
        """Reads ``state_dict`` (with 0-2 ``module.`` prefixes) and the normalizers from a checkpoint of the reference's
        layout (base_trainer.py:456-533).  Without ``setup_training`` (sampling, relaxation) the ``ema`` shadow parameters,
        if present, are copied into the weights.  With it, what a training needs to go on is restored as well: EMA
        (``load_state_dict``), optimizer (where it has a ``load_state_dict``: ``reproducible=True``), scheduler, ``step``,
        ``epoch``, ``best_val_metric``, ``primary_metric`` and - from a checkpoint written here - ``noise_step`` and the
        host generators."""
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        sd = ckpt.get("state_dict", ckpt)
        clean = {}
        for k, v in sd.items():
            while k.startswith("module."):
                k = k[len("module."):]
            clean[k] = v
        missing, unexpected = self._unwrapped_model.load_state_dict(clean, strict=False)
        for k in missing:
            logging.warning(f"checkpoint is missing key {k}")
        for k in unexpected:
            logging.warning(f"checkpoint has unexpected key {k}")
        if ckpt.get("normalizers") and hasattr(self, "load_normalizers"):
            self.load_normalizers(ckpt["normalizers"])
        ema = ckpt.get("ema")
        optimizer = getattr(self, "optimizer", None)
        if optimizer is None:
            if ema and "shadow_params" in ema:
                params = [p for p in self._unwrapped_model.parameters() if p.requires_grad]
                with torch.no_grad():
                    for p, s in zip(params, ema["shadow_params"]):
                        p.copy_(s.to(p.device))
            return
        # ---- training state
        if ema and "shadow_params" in ema and self.ema is not None:
            self.ema.load_state_dict(ema)
        if ckpt.get("optimizer") is not None:
            if hasattr(optimizer, "load_state_dict"):
                optimizer.load_state_dict(ckpt["optimizer"])
            else:
                logging.warning("the optimizer state of the checkpoint is not loaded: setup_training(reproducible=True) "
                                "builds the optimizer that takes one")
        if hasattr(optimizer, "resync_ema"):
            optimizer.resync_ema()
        if ckpt.get("scheduler") is not None:
            scheduler = getattr(self, "scheduler", None)
            if scheduler is not None and scheduler.scheduler is not None:
                self._load_scheduler_state(ckpt["scheduler"])
            else:
                self._pending_scheduler_state = ckpt["scheduler"]
        self.epoch = ckpt.get("epoch", 0)
        self.step = ckpt.get("step", 0)
        self.best_val_metric = ckpt.get("best_val_metric", None)
        self.primary_metric = ckpt.get("primary_metric", None)
        if "noise_step" in ckpt:
            self.noise_step = int(ckpt["noise_step"])
        if ckpt.get("rng") is not None:
            restore_rng(ckpt["rng"], self.device)

    def update_best(self, primary_metric: str, val_metrics: dict, disable_eval_tqdm: bool = True) -> None:
        """``base_trainer.py:686-704``: a better validation value becomes ``best_val_metric`` and the EMA weights are
        written to ``best_checkpoint.pt``.  Better: ``is_better`` - the reference's rule, under which a primary metric
        without "mae" in its name (``loss``) keeps the largest value; ``eval_metrics["primary_metric_mode"] = "min"`` opts
        out.  (The reference's prediction pass over a test loader is not part of this trainer.)"""
        value = val_metrics[primary_metric]["metric"]
        if is_better(primary_metric, value, self.best_val_metric, self.evaluation_metrics.get("primary_metric_mode")):
            self.best_val_metric = value
            self.save(metrics=val_metrics, checkpoint_file="best_checkpoint.pt", training_state=False)

    # ---------------------------------------------------------------- the loop
    def train(self, train_batches: Optional[Iterable] = None, val_batches: Optional[Iterable] = None) -> None:
        """Epochs ``step // len(train_batches) .. config["optim"]["max_epochs"]`` of ``train_step`` over ``train_batches``
        (default ``self.train_loader``; anything with ``len`` and ``iter``), as the reference's loops:

        * ``optim.eval_every`` (default: once per epoch) and at the end of every epoch: ``validate(val_batches)`` (default
          ``self.val_loader``; none: no validation) and ``update_best``;
        * ``optim.checkpoint_every`` (default ``eval_every``): ``save()``; -1: at the end of every epoch;
        * a step ``train_step`` reports as skipped (NaN loss) takes no scheduler step; ``stop`` (loss above 1e6) ends
          that epoch;
        * the scheduler steps once per applied iteration, ``ReduceLROnPlateau`` on the primary validation metric every
          ``eval_every`` steps;
        * ``sampler.set_epoch(epoch)`` where ``train_batches`` (or the trainer) has a sampler;
        * ``optim.max_steps`` (not in the reference): return once ``step`` reaches it.

        The two deviations from the reference (resume skips the batches already seen; ``checkpoint.pt`` is written last in
        an iteration) are described in the module docstring."""
        if not hasattr(self, "optimizer"):
            raise RuntimeError("call setup_training() before train()")
        if train_batches is None:
            train_batches = self.train_loader
        if val_batches is None:
            val_batches = getattr(self, "val_loader", None)
        optim = self.config.setdefault("optim", {})
        n = len(train_batches)
        if n < 1:
            raise ValueError("train(): no training batches")
        eval_every = optim.get("eval_every", n)
        checkpoint_every = optim.get("checkpoint_every", eval_every)
        print_every = self.config.get("cmd", {}).get("print_every", 10)
        max_steps = optim.get("max_steps")
        primary_metric = self._primary_metric_name()
        mode = self.evaluation_metrics.get("primary_metric_mode")
        if getattr(self, "primary_metric", None) != primary_metric or getattr(self, "best_val_metric", None) is None:
            self.best_val_metric = initial_best(primary_metric, mode) if primary_metric is not None else None
        self.primary_metric = primary_metric
        if getattr(self, "scheduler", None) is None:
            self.setup_scheduler(n)
        sampler = getattr(train_batches, "sampler", None) or getattr(self, "train_sampler", None)
        self.step = getattr(self, "step", 0)
        start_epoch = self.step // n
        val_metrics = None
        for epoch_int in range(start_epoch, optim["max_epochs"]):
            if sampler is not None and hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch_int)
            skip_steps = self.step % n
            it = iter(train_batches)
            for _ in range(skip_steps):   # deviation: the batches this epoch already trained on
                next(it)
            for i in range(skip_steps, n):
                batch = next(it)
                out = self.train_step(batch)
                self.epoch = epoch_int + (i + 1) / n
                self.step = epoch_int * n + i + 1
                if out["stop"]:   # the reference's `break`: this epoch ends, the next one starts
                    break
                if out["skipped"]:
                    continue
                plateau = self.scheduler.scheduler_type == "ReduceLROnPlateau"
                if not plateau:
                    self.scheduler.step()
                if (self.step % print_every == 0 or i == 0 or i == n - 1) and _is_master():
                    logging.info("loss: %.2e, lr: %.2e, epoch: %.2e, step: %.2e", float(out["loss"].reshape(-1)[0]),
                                 self.scheduler.get_lr(), self.epoch, self.step)
                if self.step % eval_every == 0 or i == n - 1:
                    if val_batches is not None:
                        val_metrics = self.validate(val_batches, split="val")
                        if primary_metric is not None:
                            self.update_best(primary_metric, val_metrics)
                if plateau and self.step % eval_every == 0:
                    if val_metrics is None or primary_metric is None:
                        raise ValueError("ReduceLROnPlateau needs validation batches and a primary metric")
                    self.scheduler.step(metrics=val_metrics[primary_metric]["metric"])
                if checkpoint_every != -1 and self.step % checkpoint_every == 0:
                    self.save(checkpoint_file="checkpoint.pt", training_state=True)
                if max_steps is not None and self.step >= max_steps:
                    return
            if checkpoint_every == -1:
                self.save(checkpoint_file="checkpoint.pt", training_state=True)
