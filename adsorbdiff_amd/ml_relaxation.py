"""``ml_diffuse`` — driver of the diffusion sampler; ``ml_relax`` — driver of the L-BFGS relaxation; ``ml_relax_unique`` —
``ml_relax`` of one representative per cluster of duplicate sites (an extension).

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

from . import flag_anomaly as _anomaly
from .data import Batch, data_list_collater
from .denoising_torch import Denoiser, DiffTorchCalc
from .lbfgs_torch import LBFGS, TorchCalc


def _sample_or_split(batch, make_denoiser, construct_in_try: bool = True, order=None, ids=None) -> Iterator:
    """Yield sampled (sub-)batches of ``batch``; halve and retry on RuntimeError.  ``construct_in_try=False``: only
    ``run()`` is guarded, an error of the constructor propagates (``ml_relax``, reference ml_relaxation.py:56-79).
    ``order`` (a list) receives the input index of every yielded system, in the order they are yielded."""
    if order is not None and ids is None:
        ids = list(range(int(batch.natoms.shape[0])))
    runner = None if construct_in_try else make_denoiser(batch)
    try:
        yield (runner if runner is not None else make_denoiser(batch)).run()
        if order is not None:
            order.extend(ids)
        return
    except RuntimeError:
        systems = batch.to_data_list()
        if len(systems) == 1:
            raise
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    logging.info(f"Failed to relax batch with size: {len(systems)}, splitting into two...")
    half = len(systems) // 2
    for part in (slice(half, None), slice(None, half)):
        yield from _sample_or_split(data_list_collater(systems[part]), make_denoiser, construct_in_try, order,
                                    None if order is None else ids[part])


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
    _order=None,
):
    """Relax every system of ``batch`` with the device L-BFGS driven by ``model.predict`` (a trainer such as
    ``trainer.ForcesTrainer``).  ``relax_opt``: ``memory`` (required), ``maxstep`` (0.04), ``damping`` (1.0), ``alpha`` (70.0),
    ``traj_dir`` (None), ``per_system`` (False: the reference's coupled recursion; True: every system keeps its own history
    and decisions, so the split below and a shard reproduce the unsplit run), ``drop_converged`` (False; True: a system whose
    update mask is clear is left out of the model forward from then on and the final forward is skipped,
    ``LBFGS.set_drop_converged`` - the same bits for a force model whose rows do not depend on the batch and whose forward
    is deterministic; not with ``early_stop_batch``), ``flag_anomalies`` (False; True: the returned batch carries ``anomaly``
    [B,4] bool, ``flag_anomaly.flag_anomalies`` of the positions given here against the relaxed ones, computed once on the
    collated result; ``anomaly_radii``: its radius table, default ``ase.data.covalent_radii``).  Same split-on-RuntimeError
    order as ``ml_diffuse``; returns one re-collated ``Batch``."""
    opts = {"maxstep": 0.04, "damping": 1.0, "alpha": 70.0, "traj_dir": None, "per_system": False, "drop_converged": False,
            "flag_anomalies": False, "anomaly_radii": None}
    opts.update(relax_opt)
    sink = None if opts["traj_dir"] is None else Path(opts["traj_dir"])

    # the keyword goes out only when set: LBFGS stand-ins with the reference's signature keep working
    per_system = {"per_system": True} if opts["per_system"] else {}

    class _Relaxer:
        def __init__(self, b):
            self.optimizer = LBFGS(b, TorchCalc(model, transform), maxstep=opts["maxstep"], memory=opts["memory"],
                                   damping=opts["damping"], alpha=opts["alpha"], device=device,
                                   save_full_traj=save_full_traj, traj_dir=sink, traj_names=b.sid,
                                   early_stop_batch=early_stop_batch, **per_system)
            # called only when set, for the same reason
            if opts["drop_converged"]:
                self.optimizer.set_drop_converged(True)

        def run(self):
            return self.optimizer.run(fmax=fmax, steps=steps)

    if not opts["flag_anomalies"]:
        return Batch.from_data_list(list(_sample_or_split(batch, _Relaxer, construct_in_try=False, order=_order)))
    # the optimizer moves batch.pos in place: keep the positions this call was given
    initial = batch.clone()
    order = [] if _order is None else _order
    first = len(order)
    out = Batch.from_data_list(list(_sample_or_split(batch, _Relaxer, construct_in_try=False, order=order)))
    out.anomaly = _flag_relaxed(initial, order[first:], out, opts["anomaly_radii"])
    return out


def _flag_relaxed(initial, order, relaxed, radii):
    """Anomaly flags of ``relaxed`` against ``initial``, whose systems are brought into the returned order first (the
    out-of-memory split reorders them; ``order[k]`` is the input index of returned system ``k``)."""
    if order != list(range(len(order))):
        systems = initial.to_data_list()
        initial = Batch.from_data_list([systems[i] for i in order])
    return _anomaly.flag_anomalies(initial.to(relaxed.pos.device), relaxed.pos, radii=radii)


def ml_relax_sharded(
    batch,
    model,
    steps: int,
    fmax: float,
    relax_opt,
    save_full_traj,
    rank: int,
    world: int,
    via: str = "torch",
    device: str = "cuda:0",
    transform=None,
):
    """``ml_relax`` dealt over ``world`` ranks: this rank relaxes its share of ``batch`` (``sampler.shard_batch``, by atom
    count) and ONE all-gather (``sampler.gather_relaxed``) brings every system's relaxed positions, energy and forces to
    every rank.  Returns the whole batch in global system order with ``pos``, ``y`` and ``force`` filled in.  Needs
    ``relax_opt["per_system"]``: only then does a system relax the same way in a shard as in the whole batch.  ``relax_opt``
    goes to ``ml_relax`` unchanged, so ``drop_converged`` works on every shard as it does there - but for ``flag_anomalies``:
    the flags are computed after the gather, on the whole batch, on every rank."""
    from . import sampler

    if not dict(relax_opt).get("per_system", False):
        raise ValueError("ml_relax_sharded needs relax_opt['per_system'] = True: the default L-BFGS couples the systems of "
                         "a batch through batch-wide dot products, so a shard would not reproduce the single run")
    want_flags = bool(dict(relax_opt).get("flag_anomalies", False))
    initial = batch.clone() if want_flags else None     # a shard may share storage with batch.pos
    shard_opt = dict(relax_opt, flag_anomalies=False) if want_flags else relax_opt
    mine, ids = sampler.shard_batch(batch, rank, world)
    local = None
    if ids:
        order = []
        local = ml_relax(mine, model, steps, fmax, shard_opt, save_full_traj, device=device, transform=transform,
                         _order=order)
        ids = [ids[i] for i in order]   # ml_relax returns its out-of-memory halves in the reference's order
    pos, y, force = sampler.gather_relaxed(local, ids, batch.natoms.tolist(), world, via=via)
    out = batch.clone()
    out.pos = pos.to(batch.pos.device)
    out.y = y.to(batch.pos.device)
    out.force = force.to(batch.pos.device)
    if want_flags:
        out.anomaly = _anomaly.flag_anomalies(initial.to(out.pos.device), out.pos, radii=dict(relax_opt).get("anomaly_radii"))
    return out


def ml_relax_unique(
    batch,
    model,
    steps: int,
    fmax: float,
    relax_opt,
    save_full_traj,
    group=None,
    tol: float = 0.05,
    rank=None,
    world=None,
    **kw,
):
    """``ml_relax`` of one representative per cluster of duplicate sites (``site_select.unique_sites`` on the positions given
    here, no energies yet; ``group`` defaults to ``batch.site_group``; ``include_slab`` / ``permutation_invariant`` go to it,
    every other keyword to ``ml_relax``, or to ``ml_relax_sharded`` when ``rank`` and ``world`` are given).  Returns the whole
    batch in input order - the out-of-memory split's reordering is undone: a duplicate carries its representative's relaxed
    ``pos``, ``y`` and ``force`` (and, with ``relax_opt["flag_anomalies"]``, its ``anomaly`` row); ``site_rep`` [S] holds every
    site's representative.  The sites of a cluster are the same atoms within ``tol``, so a duplicate's own relaxation would
    start from the same basin; how many relaxations that saves is a property of the input."""
    from . import site_select

    select = {k: kw.pop(k) for k in ("include_slab", "permutation_invariant") if k in kw}
    if (rank is None) != (world is None):
        raise ValueError("ml_relax_unique: rank and world go together")
    rep, is_rep, _ = site_select.unique_sites(batch, group=group, tol=tol, **select)
    dev = batch.pos.device
    chosen = is_rep.nonzero().reshape(-1).tolist()
    systems = batch.to_data_list()
    sub = Batch.from_data_list([systems[i] for i in chosen])     # a copy: the optimizer moves positions in place
    if rank is None:
        order = []
        relaxed = ml_relax(sub, model, steps, fmax, relax_opt, save_full_traj, _order=order, **kw)
    else:
        relaxed = ml_relax_sharded(sub, model, steps, fmax, relax_opt, save_full_traj, rank=rank, world=world, **kw)
        order = list(range(len(chosen)))
    # slot[i]: where input site i sits in `relaxed` (representatives only)
    S = int(batch.natoms.shape[0])
    slot = torch.full((S,), -1, dtype=torch.long)
    slot[torch.tensor([chosen[i] for i in order], dtype=torch.long)] = torch.arange(len(order))
    src = slot.to(dev)[rep]
    r_dev = relaxed.pos.device
    r_natoms = relaxed.natoms.to(r_dev).long()
    r_start = torch.cumsum(r_natoms, 0) - r_natoms
    natoms = batch.natoms.to(r_dev).long()
    N = int(batch.pos.shape[0])
    start = torch.cumsum(natoms, 0) - natoms
    src_r = src.to(r_dev)
    rows = torch.arange(N, device=r_dev) + torch.repeat_interleave(r_start[src_r] - start, natoms, output_size=N)
    out = batch.clone()
    out.pos = relaxed.pos[rows].to(dev)
    out.y = relaxed.y.reshape(-1)[src_r].to(dev)
    out.force = relaxed.force[rows].to(dev)
    if hasattr(relaxed, "anomaly"):
        out.anomaly = relaxed.anomaly[src_r.to(relaxed.anomaly.device)].to(dev)
    out.site_rep = rep
    return out
