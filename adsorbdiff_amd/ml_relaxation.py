"""``ml_diffuse`` — driver of the diffusion sampler; ``ml_relax`` — driver of the L-BFGS relaxation.

Drop-ins for ``adsorbdiff.relaxation.ml_relaxation.ml_diffuse`` / ``ml_relax`` (reference:
adsorbdiff/relaxation/ml_relaxation.py:98-168 / :23-95).  Written from their contract, not their text:

* same signature and return type (one re-collated ``Batch``);
* a ``RuntimeError`` while sampling a batch of more than one system (the HIP library reports device OOM
  and 32-bit-offset overflow as ``RuntimeError``) makes the batch be sampled as two halves instead;
* a ``RuntimeError`` on a single system propagates to the caller;
* order of the returned systems: the reference pushes both halves on the *left* of its work deque, first
  half first, so the second half is sampled (and collated) before the first one.  ``_sample_or_split``
  reproduces that order by recursing into the upper half first.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Iterator

import torch

from .data import Batch, data_list_collater
from .denoising_torch import Denoiser, DiffTorchCalc
from .lbfgs_torch import LBFGS, TorchCalc


def _sample_or_split(batch, make_denoiser, construct_in_try: bool = True) -> Iterator:
    """Yield sampled (sub-)batches of ``batch``; halve and retry on RuntimeError.  ``construct_in_try=False``: only
    ``run()`` is guarded, an error of the constructor propagates (``ml_relax``, reference ml_relaxation.py:56-79)."""
    runner = None if construct_in_try else make_denoiser(batch)
    try:
        yield (runner if runner is not None else make_denoiser(batch)).run()
        return
    except RuntimeError:
        systems = batch.to_data_list()
        if len(systems) == 1:
            raise
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    logging.info(f"Failed to relax batch with size: {len(systems)}, splitting into two...")
    half = len(systems) // 2
    for part in (systems[half:], systems[:half]):
        yield from _sample_or_split(data_list_collater(part), make_denoiser, construct_in_try)


def ml_diffuse(
    batch,
    model,
    denoising_pos_params: dict,
    traj_dir,
    save_full_traj,
    device: str = "cuda:0",
    transform=None,
    early_stop_batch: bool = False,
    logger=None,
):
    sink = Path(traj_dir) if traj_dir is not None else None

    def make_denoiser(b):
        return Denoiser(b, DiffTorchCalc(model, transform), denoising_pos_params=denoising_pos_params,
                        device=device, save_full_traj=save_full_traj, traj_dir=sink, traj_names=b.sid,
                        early_stop_batch=early_stop_batch, logger=logger)

    return Batch.from_data_list(list(_sample_or_split(batch, make_denoiser)))


def ml_relax(
    batch,
    model,
    steps: int,
    fmax: float,
    relax_opt,
    save_full_traj,
    device: str = "cuda:0",
    transform=None,
    early_stop_batch: bool = False,
):
    """Relax every system of ``batch`` with the device L-BFGS driven by ``model.predict`` (a trainer such as
    ``trainer.ForcesTrainer``).  ``relax_opt``: ``memory`` (required), ``maxstep`` (0.04), ``damping`` (1.0), ``alpha`` (70.0),
    ``traj_dir`` (None).  Same split-on-RuntimeError order as ``ml_diffuse``; returns one re-collated ``Batch``."""
    opts = {"maxstep": 0.04, "damping": 1.0, "alpha": 70.0, "traj_dir": None}
    opts.update(relax_opt)
    sink = None if opts["traj_dir"] is None else Path(opts["traj_dir"])

    class _Relaxer:
        def __init__(self, b):
            self.optimizer = LBFGS(b, TorchCalc(model, transform), maxstep=opts["maxstep"], memory=opts["memory"],
                                   damping=opts["damping"], alpha=opts["alpha"], device=device,
                                   save_full_traj=save_full_traj, traj_dir=sink, traj_names=b.sid,
                                   early_stop_batch=early_stop_batch)

        def run(self):
            return self.optimizer.run(fmax=fmax, steps=steps)

    return Batch.from_data_list(list(_sample_or_split(batch, _Relaxer, construct_in_try=False)))
