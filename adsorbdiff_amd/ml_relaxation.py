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


def _pin_image_repeats(batch, model, params: dict, always: bool = False) -> dict:
    """In per-system mode (or ``always``): ``params`` with ``image_repeats`` set to what ``batch`` as a whole needs, unless
    the caller pinned it.  The halves of an out-of-memory split and the shards then search the periodic images the unsplit
    run searches (``engine.image_repeats``: the count is a maximum over the batch)."""
    if not (always or params.get("per_system", False)) or params.get("image_repeats") is not None:
        return params
    from .engine import image_repeats

    return dict(params, image_repeats=image_repeats(batch, model._unwrapped_model.cutoff))


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
    """What a system carries (``noise_key``, ``site_index``; after a per-system run ``sample_steps``, ``sample_stopped``)
    travels with it through the out-of-memory split."""
    return Batch.from_data_list(list(_diffuse_parts(batch, model, denoising_pos_params, traj_dir, save_full_traj, device,
                                                    transform, early_stop_batch, logger, None)))


def _diffuse_parts(batch, model, denoising_pos_params, traj_dir, save_full_traj, device, transform, early_stop_batch, logger,
                   order):
    """The sampled (sub-)batches of ``ml_diffuse``; ``order`` (a list) receives the input index of every yielded system."""
    sink = Path(traj_dir) if traj_dir is not None else None
    denoising_pos_params = _pin_image_repeats(batch, model, denoising_pos_params)

    def make_denoiser(b):
        return Denoiser(b, DiffTorchCalc(model, transform), denoising_pos_params=denoising_pos_params,
                        device=device, save_full_traj=save_full_traj, traj_dir=sink, traj_names=b.sid,
                        early_stop_batch=early_stop_batch, logger=logger)

    return _sample_or_split(batch, make_denoiser, order=order)


def ml_diffuse_sharded(
    batch,
    model,
    denoising_pos_params: dict,
    traj_dir,
    save_full_traj,
    device: str = "cuda:0",
    rank: int = 0,
    world: int = 1,
    via: str = "torch",
    transform=None,
):
    """``ml_diffuse`` dealt over ``world`` ranks, the twin of ``ml_relax_sharded``: this rank samples its share of ``batch``
    (``sampler.shard_batch``) and ONE all-gather (``sampler.gather_sites``) brings every system's sampled adsorbate to every
    rank.  Returns the whole batch in global system order with the adsorbate rows filled in; ``sample_steps`` (per-system
    mode) is -1 for the systems sampled on another rank - it is not gathered.  A shard reproduces the single run only if
    nothing couples a system to its batch-mates, so this needs

    * ``per_system=True`` or ``early_stop=False`` (the default early stop is one decision over the batch), and
    * a shard-invariant noise source: ``noise_seed``, or an ODE run (``ode`` not False, sampler not ``"langevin"``) with a
      global ``[B,3]`` ``placement_noise``, which is sliced by system id here;

    otherwise ``ValueError`` names what is missing."""
    from . import sampler

    params = dict(denoising_pos_params)
    if not params.get("per_system", False) and params.get("early_stop", True) and params.get("sampler", "sde_rot") != "langevin":
        raise ValueError("ml_diffuse_sharded needs denoising_pos_params['per_system'] = True or ['early_stop'] = False: the "
                         "default early stop is one decision over all systems of a batch, so a shard would not reproduce "
                         "the single run")
    B = int(batch.natoms.shape[0])
    table = params.get("placement_noise")
    if params.get("noise_seed") is None:
        stochastic = params.get("sampler", "sde_rot") == "langevin" or (
            params.get("sampler", "sde_rot") == "sde_rot" and not params.get("ode", True))
        if stochastic or table is None:
            raise ValueError("ml_diffuse_sharded needs a shard-invariant noise source: denoising_pos_params['noise_seed'], "
                             "or an ODE sampler with a global [B,3] 'placement_noise' (the default draws are streams over "
                             "the batch)")
    if table is not None:
        table = torch.as_tensor(table, dtype=torch.float32).reshape(-1, 3)
        if table.shape[0] != B:
            raise ValueError(f"placement_noise has {table.shape[0]} rows, the batch has {B} systems")
    params = _pin_image_repeats(batch, model, params, always=True)   # of the GLOBAL batch: every shard searches the same images
    mine, ids = sampler.shard_batch(batch, rank, world)
    local = None
    if ids:
        if table is not None:
            params["placement_noise"] = table[torch.as_tensor(ids, dtype=torch.long)]
        order = []
        if table is not None:   # a table indexed by position cannot follow the out-of-memory split: sample unsplit
            local = Batch.from_data_list([Denoiser(mine, DiffTorchCalc(model, transform), denoising_pos_params=params,
                                                   device=device, save_full_traj=save_full_traj,
                                                   traj_dir=Path(traj_dir) if traj_dir is not None else None,
                                                   traj_names=mine.sid).run()])
            order = list(range(len(ids)))
        else:
            local = Batch.from_data_list(list(_diffuse_parts(mine, model, params, traj_dir, save_full_traj, device, transform,
                                                             False, None, order)))
        ids = [ids[i] for i in order]
    sites = sampler.gather_sites(local, world, via=via, system_ids=ids, bounds=sampler.shard_bounds(batch, world))
    if world <= 1:   # no exchange: the local sites, brought into global order here
        sites = sites[torch.argsort(torch.as_tensor(ids, dtype=torch.long)).to(sites.device)]
    return assemble_sharded(batch, sites, local, ids)


def assemble_sharded(batch, sites, local, ids):
    """The result of ``ml_diffuse_sharded`` on one rank: ``batch`` with every system's adsorbate rows taken from ``sites``
    ([B, A_max, 3] in global system order, what ``gather_sites`` returns) and, if this rank's shard ``local`` (systems
    ``ids``, in its order; None for a rank that was dealt nothing) ran in per-system mode, ``sample_steps`` /
    ``sample_stopped`` filled in for its own systems: -1 / False for the systems sampled elsewhere."""
    B = int(batch.natoms.shape[0])
    out = batch.clone()
    dev = out.pos.device
    m = out.tags == 2
    idx_b = out.batch[m]
    counts = torch.bincount(idx_b, minlength=B)
    within = torch.arange(idx_b.shape[0], device=dev) - (torch.cumsum(counts, 0) - counts)[idx_b]
    out.pos = out.pos.clone()
    out.pos[m] = sites.to(dev, out.pos.dtype)[idx_b, within]
    if local is not None and hasattr(local, "sample_steps"):
        gid = torch.as_tensor(ids, dtype=torch.long, device=dev)
        out.sample_steps = torch.full((B,), -1, dtype=torch.int64, device=dev)
        out.sample_steps[gid] = local.sample_steps.to(dev)
        out.sample_stopped = torch.zeros(B, dtype=torch.bool, device=dev)
        out.sample_stopped[gid] = local.sample_stopped.to(dev)
    return out


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
    symmetry=None,
    **kw,
):
    """``ml_relax`` of one representative per cluster of duplicate sites (``site_select.unique_sites`` on the positions given
    here, no energies yet; ``group`` defaults to ``batch.site_group``; ``include_slab`` / ``permutation_invariant`` go to it,
    every other keyword to ``ml_relax``, or to ``ml_relax_sharded`` when ``rank`` and ``world`` are given).  Returns the whole
    batch in input order - the out-of-memory split's reordering is undone: a duplicate carries its representative's relaxed
    ``pos``, ``y`` and ``force`` (and, with ``relax_opt["flag_anomalies"]``, its ``anomaly`` row); ``site_rep`` [S] holds every
    site's representative.  The sites of a cluster are the same atoms within ``tol``, so a duplicate's own relaxation would
    start from the same basin; how many relaxations that saves is a property of the input.

    ``symmetry`` (``slab_symmetry.find_symmetry`` of the bare slabs; its slab b is group id b): sites that are images of each
    other under an operation of their slab are one cluster too.  A duplicate s merged into r under operation
    g = (R, tau, perm) gets ``y`` and the ``anomaly`` row of r unchanged and r's relaxed ``pos`` and ``force`` carried through g
    (``slab_symmetry.carry``), in the direction the distance recorded: where s comes before r in its group (g takes s onto r)
    slab atom i of s is ``R^-1 (x_r[perm[i]] - tau)`` and adsorbate atom m ``R^-1 (x_r[m] - tau)``; otherwise slab atom
    ``perm[i]`` of s is ``R x_r[i] + tau`` and adsorbate atom m ``R x_r[m] + tau``; forces go through ``R`` / ``R^-1`` without
    ``tau``; positions are not wrapped back into the cell.  Adsorbate rows keep r's atom order: with the permutation-invariant
    (Hausdorff) adsorbate rule the result is r's relaxed site up to a relabelling of same-element adsorbate atoms.
    Operation 0 is the plain copy, bit for bit.  The batch also carries ``site_op`` [S] and ``site_op_inverse`` [S]."""
    from . import site_select

    select = {k: kw.pop(k) for k in ("include_slab", "permutation_invariant") if k in kw}
    if (rank is None) != (world is None):
        raise ValueError("ml_relax_unique: rank and world go together")
    if symmetry is None:
        rep, is_rep, _ = site_select.unique_sites(batch, group=group, tol=tol, **select)
    else:
        rep, is_rep, _, site_op, site_op_inverse = site_select.unique_sites(batch, group=group, tol=tol, symmetry=symmetry,
                                                                            return_op=True, **select)
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
    if symmetry is not None:
        from . import slab_symmetry

        slab = torch.as_tensor(batch.site_group if group is None else group).reshape(-1).to(dev)
        out.pos, out.force = slab_symmetry.carry(symmetry, slab, site_op, site_op_inverse, batch.tags, batch.natoms, out.pos,
                                                 out.force)
        out.site_op, out.site_op_inverse = site_op, site_op_inverse
    return out
