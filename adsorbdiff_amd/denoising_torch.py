"""Reverse-SDE/ODE stepper — host-side mirror of the reference's ``Denoiser`` / ``DiffTorchCalc``.

Drop-in for ``adsorbdiff.relaxation.diffusers.denoising_torch`` (reference:
adsorbdiff/relaxation/diffusers/denoising_torch.py:18-511): same class names, constructor
signatures and ``run() -> batch`` contract (positions updated in place; ``batch.y`` /
``batch.force`` zeroed as the reference's ``write`` does, :470).

What differs is where the work happens: the whole loop is device resident.  The host enqueues
``adf_painn_forward`` + ``adf_sde_step`` per step on the current HIP stream — as one ``adf_sample`` call
when nothing has to be handed to the host between steps; the per-system
Python loop, the ``torch.linalg.solve``/``%``/``einsum`` wrap and the per-step device->host
trajectory dump of the reference (:296-367) are replaced by two tiny kernels.  The cumulative
early-stop counter lives on the device; once it fires, later steps are no-ops on the positions,
which is exactly the reference's ``break``.

Extensions (all optional, defaults reproduce the reference):
  * ``denoising_pos_params["early_stop"]`` (default True): ``False`` disables the allclose
    early stop so that exactly ``num_steps`` steps run (used by bench.py).
  * ``denoising_pos_params["use_graph"]`` (default False): replay one captured hipGraph per step.
  * ``denoising_pos_params["static_atom_cache"]`` (default True): declare the slab static for the loop
    (``adf_graph_set_moving``) so that loop-invariant work — the slab-slab part of the top-K search and the
    layer-0 gather records, which depend on atomic numbers only — is done once.  Bit-identical results.
  * ``denoising_pos_params["incremental_layers"]`` (default True; needs ``static_atom_cache``): the engine keeps the
    node state of every layer across the steps and recomputes a row only if one of its inputs changed since it was
    computed (detected by comparing the new graph with the previous one bit for bit and following the edges; the
    receptive field of the moving adsorbate grows one neighbour shell per layer).  Bit-identical results.
  * ``denoising_pos_params["scores_on_adsorbate_only"]`` (default: on inside the fused loop, off on the per-step
    path): the update only ever reads the model output on tag-2 atoms (reference :263-268, :460-467), so the last
    layer and the heads can be evaluated for those atoms alone (``adf_painn_forward_subset`` /
    ``adf_eqv2_forward_subset``).  Sampled positions are bit-identical.  Inside ``adf_sample`` / ``adf_sample_traj``
    the per-atom outputs never leave the library, so since round 5 the subset form is what runs there unless the
    caller passes ``False``; the per-step path (step hook, host noise, graph replay) and every direct
    ``model.forward(data)`` / ``predict_denoising`` call keep the full per-atom outputs.
  * ``denoising_pos_params["placement_noise"]`` (default None): ``[B,3]`` uniforms for the initial placement instead
    of ``torch.rand(B,3)`` from the CPU generator (:215) — a sharded run that indexes one global table by system id
    samples exactly what the single-process run samples.
  * ``denoising_pos_params["sampler"]`` (default ``"sde_rot"``): what ``run()`` calls - ``"sde_rot"``
    ``reverse_sde_sampling_rot`` (the reference's ``run``), ``"sde"`` ``reverse_sde_sampling``, ``"langevin"``
    ``langevin_dynamics``; any other value raises ``ValueError``.
  * ``denoising_pos_params["langevin_noise"]`` (default None): ``[num_steps * n_step_each, B, 3]`` standard normals for
    ``langevin_dynamics`` instead of the device generator's ``randn_like`` per inner step (a sharded run slices one global
    table by system id, as with ``placement_noise``).
  * ``denoising_pos_params["per_system"]`` (default False): every system follows the reference's loop as if it were sampled
    alone (``adf_*_set_per_system_stop``, csrc/stepper.hip): its own cumulative count of converged steps, its own stop - a
    stopped system is neither read nor written again - instead of ONE ``allclose`` over the whole batch (:312-320), which in
    a large batch almost never fires.  A system then gets the same bits alone, in any batch, in any order, after
    ``ml_diffuse``'s split and on any shard (given noise that is keyed the same way: ``noise_seed``, or ODE with
    ``placement_noise``).  After ``run()``: ``batch.sample_steps`` (int64 [B], steps applied), ``batch.sample_stopped`` (bool
    [B]), ``Denoiser.stop_step`` ([B], the step at which the system stopped, -1 = ran to the end), ``Denoiser.steps_applied``
    = the largest; ``Denoiser.cvg_count`` is the number of stopped systems.  With a ``traj_dir``, ``<sid>.npz`` holds the
    system's own ``max(sample_steps[b], 1)`` frames (the batch file keeps every frame).  Fused and per-step path, all three
    samplers (Langevin has no stop: only the attributes appear); with ``use_graph``: ``ValueError``.  What stays a decision
    of the whole batch is the exact-f32 retry: one system leaving the f16x3 range re-runs all of them in exact f32.
  * ``denoising_pos_params["noise_seed"]`` (default None): the placement uniforms and the step normals (``ode=False``,
    Langevin) come from the counter-based ``adf_sampler_draws`` keyed by ``(noise_seed, noising.noise_keys(batch)[b],
    batch.site_index[b] or 0)`` instead of ``torch.rand`` / ``normal_()`` streams over the batch.  An explicit
    ``placement_noise``, ``langevin_noise`` or ``noise_fn`` still wins for its part.  Two systems of one batch with the same
    ``(key, site_index)`` would be sampled identically: ``ValueError``.  Keys that fell back to the batch index: one
    warning, the run is not batch-invariant.  Independent of ``per_system``.
  * ``denoising_pos_params["split_streams"]`` (default None = ``ADF_SAMPLE_SPLIT`` as the engine's handle read it: on
    unless it is 0): the fused ``sde_rot`` loop of a PaiNN batch of two or more systems runs as two half-batches on two
    streams (``adf_sample_split``, DESIGN.md 4 "Two half-batches, two streams"); bit-identical results.
  * ``denoising_pos_params["image_repeats"]`` (default None): a floor ``[ra, rb, rc]`` for the number of periodic images the
    graph search tries per lattice direction.  That number is the largest need over the batch (reference
    utils/utils.py:634-662), the one input a system's graph takes from its batch-mates: an adsorbate atom outside the cell
    can gain a neighbour when a mate with a smaller cell raises the count.  ``ml_diffuse`` (in per-system mode) and
    ``ml_diffuse_sharded`` pin it to the need of the batch they are given, so their halves and shards build the graphs of
    the unsplit run; pass ``engine.image_repeats(global_batch, cutoff)`` to compare runs of other batches bit for bit.
  * ``traj_dir=None`` is allowed (the reference crashes in ``write``); with a ``traj_dir`` the
    frames are kept on the device during the loop and written once at the end.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Callable, List, Optional

import numpy as np
import torch

from . import lib as _lib


def schedule_coefs(params: dict) -> List[_lib.StepCoef]:
    """Per-step scalars with the reference's own 0-dim tensor arithmetic and dtypes
    (denoising_torch.py:209-213, 237-293)."""
    lo, hi = params["ads_std_low"], params["ads_std_high"]
    rlo, rhi = params["rot_std_low"], params["rot_std_high"]
    T = int(params["num_steps"])
    ode = params.get("ode", True)
    sched = torch.tensor(np.linspace(1, 0, T + 1)[:-1], dtype=torch.float32)
    out = []
    for t_idx in range(T):
        t = sched[t_idx]
        tr_sigma = lo ** (1 - t) * hi**t
        rot_sigma = rlo ** (1 - t) * rhi**t
        tr_g = tr_sigma * (2 * np.log(hi / lo)) ** 0.5
        rot_g = 2 * rot_sigma * torch.sqrt(torch.tensor(np.log(rhi / rlo)))
        dt = sched[t_idx] - sched[t_idx + 1] if t_idx < T - 1 else sched[t_idx]
        c = _lib.StepCoef()
        c.rot_dt = float(dt)
        c.rot_g2 = float((rot_g**2).to(torch.float32))
        if ode:
            c.coef_tr = float(0.5 * tr_g**2 * dt)
            c.rot_pre = 0.5
            c.noise_tr = c.noise_rot = 0.0
        else:
            c.coef_tr = float(tr_g**2 * dt)
            c.rot_pre = 1.0
            sqrt_dt = np.sqrt(np.float32(dt.item()))  # the reference's np.sqrt(dt) on a float32 0-dim tensor
            c.noise_tr = float(tr_g * sqrt_dt)
            c.noise_rot = float((rot_g * sqrt_dt).to(torch.float32))
        out.append(c)
    return out


def ode_tr_coefs(params: dict) -> List[_lib.TrCoef]:
    """Per-step scalars of ``reverse_sde_sampling`` (probability-flow ODE, reference :101-107, 139-150): coef =
    0.5 * g_tr^2 * dt with the reference's 0-dim f32 tensor arithmetic - the ``coef_tr`` of ``schedule_coefs`` with
    ``ode``, without reading the rotation keys."""
    lo, hi = params["ads_std_low"], params["ads_std_high"]
    T = int(params["num_steps"])
    sched = torch.tensor(np.linspace(1, 0, T + 1)[:-1], dtype=torch.float32)
    out = []
    for t_idx in range(T):
        sigma = lo ** (1 - sched[t_idx]) * hi ** sched[t_idx]
        tr_g = sigma * (2 * np.log(hi / lo)) ** 0.5
        dt = sched[t_idx] - sched[t_idx + 1] if t_idx < T - 1 else sched[t_idx]
        c = _lib.TrCoef()
        c.coef = float(0.5 * tr_g**2 * dt)
        c.noise = 0.0
        out.append(c)
    return out


def langevin_coefs(params: dict) -> List[_lib.TrCoef]:
    """Per-inner-step scalars of ``langevin_dynamics`` (reference :376-421): for each noise level sigma of
    f32(exp(linspace(log hi, log lo, num_steps))), ``n_step_each`` rows of (step_size, sqrt(2 * step_size)) with
    step_size = step_lr * (sigma / sigma_min)^2, all f32 as there.  ``n_step_each`` / ``step_lr`` missing: KeyError."""
    lo, hi = params["ads_std_low"], params["ads_std_high"]
    T = int(params["num_steps"])
    n_each = int(params["n_step_each"])
    step_lr = params["step_lr"]
    sigmas = torch.tensor(np.exp(np.linspace(np.log(hi), np.log(lo), T)), dtype=torch.float32)
    out = []
    for sigma in sigmas:
        step_size = step_lr * (sigma / sigmas[-1]) ** 2
        noise = torch.sqrt(step_size * 2)
        for _ in range(n_each):
            c = _lib.TrCoef()
            c.coef, c.noise = float(step_size), float(noise)
            out.append(c)
    return out


def per_system_stop_steps(conv, count: int = 10):
    """The per-system stop rule on the host: ``conv`` [T,B] bool (step t left every wrapped abs(dcom) of system b <= 1e-3) ->
    ``(steps_applied [B], stop_step [B])`` int64.  A system's cumulative count of converged steps reaching ``count`` at step t
    stops it BEFORE that step's update (the reference's ``break``, :312-320, for that system alone): ``stop_step = t``,
    ``steps_applied`` = the updates before it; a system that never gets there has ``stop_step = -1`` and T updates.
    ``count <= 0``: nothing stops.  The oracle of ``adf_*_set_per_system_stop``."""
    conv = torch.as_tensor(conv).to(torch.bool)
    if conv.dim() != 2:
        raise ValueError(f"per_system_stop_steps: [T,B] expected, got {list(conv.shape)}")
    T, B = conv.shape
    cum = torch.cumsum(conv.to(torch.int64), 0)
    hit = (cum == int(count)) & conv if count > 0 else torch.zeros_like(conv)
    any_hit = hit.any(0)
    first = torch.argmax(hit.to(torch.int64), 0)
    stop_step = torch.where(any_hit, first, torch.full_like(first, -1))
    steps = torch.where(any_hit, first, torch.full_like(first, T))
    return steps, stop_step


class DiffTorchCalc:
    """Adapter between the stepper and a trainer-like object
    (reference: denoising_torch.py:486-511)."""

    def __init__(self, model, transform=None) -> None:
        self.model = model
        self.transform = transform

    def get_denoising_prediction(self, atoms, apply_constraint: bool = True):
        predictions = self.model.predict_denoising(atoms, per_image=False, disable_tqdm=True)
        positions = predictions["positions"]
        if "positions_free" in predictions and apply_constraint:
            positions_free = predictions["positions_free"]
            positions_free[atoms.fixed.to(positions_free.device) == 1] = 0
            return positions, positions_free
        return positions

    def update_graph(self, atoms):
        raise NotImplementedError(
            "pre-computed graphs (otf_graph=False) are not part of the HIP sampling path; "
            "the graph is rebuilt on the device every step"
        )


class Denoiser:
    def __init__(
        self,
        batch,
        model: DiffTorchCalc,
        denoising_pos_params: dict,
        device: str = "cuda:0",
        save_full_traj: bool = True,
        traj_dir: Optional[Path] = None,
        traj_names=None,
        early_stop_batch: bool = False,
        logger=None,
        noise_fn: Optional[Callable[[int, int], tuple]] = None,
    ) -> None:
        self.batch = batch
        self.model = model
        self.device = device
        self.save_full = save_full_traj
        self.traj_dir = traj_dir
        self.traj_names = traj_names
        self.early_stop_batch = early_stop_batch
        self.otf_graph = model.model._unwrapped_model.otf_graph
        self.denoising_pos_params = denoising_pos_params
        self.noise_fn = noise_fn
        self.steps_applied = 0
        self.stop_step = None
        self.per_system = bool(denoising_pos_params.get("per_system", False))
        if self.per_system and denoising_pos_params.get("use_graph", False):
            raise ValueError("denoising_pos_params: per_system with use_graph - the per-system rule ends the loop by a read "
                             "of the frozen count, which a replayed graph does not make")
        self.noise_seed = denoising_pos_params.get("noise_seed")
        self._noise_keys = self._noise_site = None
        if self.noise_seed is not None:
            self._init_noise_keys()
        assert not self.traj_dir or (
            traj_dir and len(traj_names)
        ), "Trajectory names should be specified to save trajectories"
        if not self.otf_graph:
            raise NotImplementedError("the HIP sampling path requires otf_graph=True")

    def _init_noise_keys(self) -> None:
        """Keys and site indices of ``noise_seed``: checked here, before anything runs."""
        from .noising import noise_key_source, noise_keys

        batch = self.batch
        B = int(batch.natoms.shape[0])
        keys = noise_keys(batch).detach().cpu().reshape(-1)
        if noise_key_source(batch) == "index":
            logging.warning("adsorbdiff_amd: noise_seed without batch.noise_key or batch.sid: the keys are the positions in "
                            "the batch, so this run is NOT batch-invariant")
        site = getattr(batch, "site_index", None)
        site = torch.zeros(B, dtype=torch.int32) if site is None else torch.as_tensor(site).detach().cpu().reshape(-1).to(torch.int32)
        if site.numel() != B:
            raise ValueError(f"batch.site_index: [{B}] expected, got [{site.numel()}]")
        if site.numel() and (int(site.min()) < 0 or int(site.max()) >= (1 << 30)):
            raise ValueError("batch.site_index outside [0, 2^30)")
        pairs = set(zip(keys.tolist(), site.tolist()))
        if len(pairs) != B:
            raise ValueError("noise_seed: two systems of the batch share (noise key, site_index) and would be sampled "
                             "identically; give them distinct batch.noise_key / sid or batch.site_index")
        self._noise_keys, self._noise_site = keys, site

    def _keyed_draws(self, dev, T: int, place: bool = False, z_a: bool = False, z_b: bool = False):
        from .engine import sampler_draws

        return sampler_draws(int(self.noise_seed), self._noise_keys, self._noise_site, T, dev, place=place, z_a=z_a, z_b=z_b)

    # ------------------------------------------------------------------ public
    SAMPLERS = ("sde_rot", "sde", "langevin")

    def run(self):
        sampler = self.denoising_pos_params.get("sampler", "sde_rot")
        if sampler not in self.SAMPLERS:
            raise ValueError(f"denoising_pos_params['sampler'] = {sampler!r}: expected one of {self.SAMPLERS}")
        if sampler == "sde":
            self.reverse_sde_sampling()
        elif sampler == "langevin":
            self.langevin_dynamics()
        else:
            self.reverse_sde_sampling_rot()
        return self.batch

    # ------------------------------------------------------------------ loop
    def _engine(self):
        net = self.model.model._unwrapped_model
        if not hasattr(net, "engine"):
            raise RuntimeError(
                "Denoiser needs an adsorbdiff_amd score model (PaiNN with a HIP engine); got "
                f"{type(net).__name__}"
            )
        return net.engine(torch.device(self.device))

    def reverse_sde_sampling_rot(self):
        params = self.denoising_pos_params
        if "ads_std_low" not in params:
            return
        T = int(params["num_steps"])
        ode = params.get("ode", True)
        coefs = schedule_coefs(params)
        early = 10 if params.get("early_stop", True) else 0
        use_graph = bool(params.get("use_graph", False))

        def begin(eng, prep, pos):
            B, N, dev = prep.num_systems, prep.num_atoms, pos.device
            # schedule table on the device: every step is then the same launch sequence and can be replayed
            # from one captured hipGraph (`use_graph`, opt-in: measured no gain on MI355X at B=1 — the step is
            # bound by the dependent chain of ~140 small kernels on the device, not by launch overhead)
            coefs_dev = torch.tensor(
                [[c.coef_tr, c.rot_pre, c.rot_dt, c.rot_g2, c.noise_tr, c.noise_rot] for c in coefs],
                dtype=torch.float32, device=dev)

            def fused(f1, state, out_idx, poll_every, sink):
                f2 = torch.zeros(N, 3, dtype=torch.float32, device=dev)
                zt = zr = None
                if not ode and self.noise_seed is not None:   # keyed per system: z_tr = z_a, z_rot = z_b
                    _, zt, zr = self._keyed_draws(dev, T, z_a=True, z_b=True)
                elif not ode:  # device generator, drawn in the reference's order (:274-289): z_tr then z_rot, per step
                    zt = torch.empty(T, B, 3, dtype=torch.float32, device=dev)
                    zr = torch.empty(T, B, 3, dtype=torch.float32, device=dev)
                    for t_idx in range(T):
                        zt[t_idx].normal_()
                        zr[t_idx].normal_()
                eng.sample(prep, pos, f1, f2, coefs_dev, T, state, zt, zr, early_stop_count=early, poll_every=poll_every,
                           out_idx=out_idx, sink=sink, frame_every=1, split_streams=params.get("split_streams"))

            def per_step(f1, state, out_idx):
                f2 = torch.zeros(N, 3, dtype=torch.float32, device=dev)
                z_tr = z_rot = graph = keyed = None
                if not ode:
                    z_tr = torch.empty(B, 3, dtype=torch.float32, device=dev)
                    z_rot = torch.empty(B, 3, dtype=torch.float32, device=dev)
                    if self.noise_fn is None and self.noise_seed is not None:
                        keyed = self._keyed_draws(dev, T, z_a=True, z_b=True)[1:]

                def one_step():
                    eng.forward_prepared(prep, pos, f1, f2, out_idx)
                    eng.sde_step_scheduled(prep, pos, f1, f2, coefs_dev, T, state, z_tr, z_rot, early_stop_count=early)

                def step(t_idx):
                    nonlocal graph
                    if not ode:
                        if self.noise_fn is not None:
                            a, b_ = self.noise_fn(t_idx, B)
                            z_tr.copy_(a.to(dev, torch.float32))
                            z_rot.copy_(b_.to(dev, torch.float32))
                        elif keyed is not None:
                            z_tr.copy_(keyed[0][t_idx])
                            z_rot.copy_(keyed[1][t_idx])
                        else:  # device generator, like the reference (:274-289)
                            z_tr.normal_()
                            z_rot.normal_()
                    if graph is not None:
                        graph.replay()
                        return
                    one_step()
                    if use_graph and t_idx == 0 and T > 2:
                        # step 0 ran eagerly (workspaces are now allocated); capture the identical step once
                        torch.cuda.synchronize(dev)
                        graph = torch.cuda.CUDAGraph()
                        snapshot = (pos.clone(), state.clone())
                        with torch.cuda.graph(graph):
                            one_step()
                        # the capture itself does not execute; restore nothing, but make sure state is intact
                        assert torch.equal(state, snapshot[1])

                return step

            return fused, per_step

        # The fused loop needs nothing handed to the host between steps: no host noise hook, no graph replay, no step
        # hook.  A captured step replays fixed buffers: the previous-graph / current-graph swap the incremental layers'
        # comparison rests on, and the late read-back of the list lengths that picks between the list and the all-rows
        # form, do not replay.
        self._sample(T, early, begin, fused=not use_graph and self.noise_fn is None and params.get("step_hook") is None,
                     incremental=not use_graph)

    # ------------------------------------------------------------------ translation-only samplers
    def reverse_sde_sampling(self):
        """The reference's translation-only probability-flow ODE (denoising_torch.py:96-196): no noise term whatever
        ``ode`` says, the cumulative early stop of ``reverse_sde_sampling_rot`` (``early_stop`` switch as there), and
        ``pos += dcom`` on the adsorbate.  Reads head 1 only, so a single-head PaiNN works too (the reference unpacks two
        outputs there and fails for one)."""
        params = self.denoising_pos_params
        if "ads_std_low" not in params:
            return
        coefs = ode_tr_coefs(params)
        self._tr_sampling(coefs, False, None, 10 if params.get("early_stop", True) else 0)

    def langevin_dynamics(self):
        """The reference's annealed Langevin dynamics (denoising_torch.py:369-458): ``num_steps`` noise levels x
        ``n_step_each`` inner steps of dcom = step_size * score + sqrt(2 step_size) * z, no early stop, one trajectory
        frame per inner step.  The score is head 1 (``positions``) for one- and two-head models alike (the reference
        hands a two-head model's tuple to ``_get_ads_output`` and raises TypeError).  z: ``langevin_noise`` if given,
        else drawn on the device generator, one ``normal_()`` per inner step as the reference's ``randn_like``."""
        params = self.denoising_pos_params
        if "ads_std_low" not in params:
            return
        coefs = langevin_coefs(params)
        self._tr_sampling(coefs, True, params.get("langevin_noise"), 0)

    def _tr_sampling(self, coefs, langevin: bool, noise_table, early: int) -> None:
        """The translation-only samplers' parts of ``_sample``: the fused loop evaluates head 1 only, the per-step path
        the full forward (both heads of a two-head model) and then the same step kernels.  Langevin's noise table is
        drawn once, before the placement: an exact-f32 retry reuses it."""
        T = len(coefs)

        def begin(eng, prep, pos):
            B, N, dev = prep.num_systems, prep.num_atoms, pos.device
            z_all = None
            if langevin:
                if noise_table is None and self.noise_seed is not None:   # keyed per system, t = the inner-step index
                    z_all = self._keyed_draws(dev, T, z_a=True)[1]
                elif noise_table is None:  # device generator, one randn_like([B,3]) per inner step (reference :417)
                    z_all = torch.empty(T, B, 3, dtype=torch.float32, device=dev)
                    for t_idx in range(T):
                        z_all[t_idx].normal_()
                else:  # extension: caller-supplied standard normals
                    z_all = torch.as_tensor(noise_table, dtype=torch.float32)
                    if tuple(z_all.shape) != (T, B, 3):
                        raise ValueError(f"langevin_noise has shape {tuple(z_all.shape)}, expected {(T, B, 3)}")
                    z_all = z_all.to(dev).contiguous()
            coefs_dev = torch.tensor([[c.coef, c.noise] for c in coefs], dtype=torch.float32, device=dev)

            def fused(f1, state, out_idx, poll_every, sink):
                eng.tr_sample(prep, pos, f1, coefs_dev, T, state, z_all, early_stop_count=early, poll_every=poll_every,
                              out_idx=out_idx, sink=sink, frame_every=1)

            def per_step(f1, state, out_idx):
                f2 = torch.zeros(N, 3, dtype=torch.float32, device=dev) if eng.num_heads == 2 else None

                def step(t_idx):
                    eng.forward_prepared(prep, pos, f1, f2, out_idx)
                    eng.tr_step(prep, pos, f1, state, coefs_dev=coefs_dev, num_steps=T,
                                z=z_all[t_idx] if z_all is not None else None, early_stop_count=early)

                return step

            return fused, per_step

        self._sample(T, early, begin, fused=self.denoising_pos_params.get("step_hook") is None, incremental=True)

    # ------------------------------------------------------------------ the frame of every sampler
    def _sample(self, T: int, early: int, begin, fused: bool, incremental: bool) -> None:
        """Eval mode and the EMA weights, the batch on the device, the initial placement, the static-atom cache, one
        attempt of ``T`` steps - repeated in exact f32 from the placed positions if it left the f16x3 range - and the
        trajectories.  The sampler's parts come from ``begin(eng, prep, pos)``, called before the placement:
        ``fused(f1, state, out_idx, poll_every, sink)`` runs its whole loop in one library call (taken when ``fused``),
        ``per_step(f1, state, out_idx)`` returns the host-driven ``step(t)``.  ``incremental``: the sampler allows the
        incremental layers."""
        params = self.denoising_pos_params
        trainer = self.model.model
        dev = torch.device(self.device)
        # what predict_denoising does around every model call in the reference
        # (sde_denoising_trainer.py:577-580,638-639), done once around the loop here
        trainer._unwrapped_model.eval()
        ema = getattr(trainer, "ema", None)
        if ema:
            ema.store()
            ema.copy_to()
        try:
            eng = self._engine()
            batch = self.batch.to(dev)  # in place, like the reference's batch.to(self.device)
            if batch.pos.dtype != torch.float32 or not batch.pos.is_contiguous():
                batch.pos = batch.pos.to(torch.float32).contiguous()
            pos = batch.pos
            prep = eng.prepare(batch, params.get("image_repeats"))
            if prep.tags is None:
                raise ValueError("batch.tags is required (tag 2 marks the adsorbate)")
            eng.bind_condition(batch, prep.num_systems)  # conditional EquiformerV2: batch.energy, once for the whole loop
            B, N = prep.num_systems, prep.num_atoms
            fused_run, per_step = begin(eng, prep, pos)

            # initial placement: uniform noise from the CPU global generator (reference :215)
            noise = params.get("placement_noise")
            if noise is None and self.noise_seed is not None:   # extension: keyed per system
                noise = self._keyed_draws(dev, 0, place=True)[0]
            elif noise is None:
                noise = torch.rand(B, 3)
            else:  # extension: caller-supplied uniforms (sharded runs key them by global system id)
                noise = torch.as_tensor(noise, dtype=torch.float32).reshape(B, 3).cpu()
            eng.init_placement(prep, pos, noise.to(dev))
            # from here on only the adsorbate (tag 2) moves: the graph builder may cache the slab-slab part and the
            # forward the layer-0 records (loop-invariant; results are bit-identical either way)
            if params.get("static_atom_cache", True):
                eng.set_moving_atoms(prep, prep.tags == 2)
            eng.set_incremental(bool(params.get("incremental_layers", True)) and incremental)

            step_hook = params.get("step_hook")  # extension: callable(t) after every applied step (diagnostics)
            check_every = 1 if B <= 8 else 5
            ads_only = params.get("scores_on_adsorbate_only")
            if ads_only is None:
                ads_only = fused   # unobservable there: no per-atom output leaves the library
            pos0 = pos.clone()  # a run that leaves the f16x3 range is repeated in exact f32 from here

            def attempt():
                f1 = torch.zeros(N, 3, dtype=torch.float32, device=dev)
                state = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
                sys_state = None
                if self.per_system:
                    sys_state = torch.tensor([[0, 0, 0, -1]] * B, dtype=torch.int32, device=dev)
                    eng.set_per_system_stop(sys_state)
                out_idx = torch.nonzero(prep.tags == 2).reshape(-1).to(torch.int32).contiguous() if ads_only else None
                if fused:
                    self._run_fused(eng, batch, pos, state, T,
                                    lambda sink: fused_run(f1, state, out_idx, check_every if early else 0, sink), sys_state)
                    return state, None, sys_state
                frames = [] if self.traj_dir else None
                step = per_step(f1, state, out_idx)
                for t_idx in range(T):
                    step(t_idx)
                    if frames is not None and (self.save_full or t_idx == T - 1):
                        frames.append(pos.clone())
                    if step_hook is not None:
                        step_hook(t_idx)
                    if early and (t_idx % check_every == check_every - 1):
                        if int(state[1].item()):
                            break
                if frames is not None and not frames:
                    frames.append(pos.clone())
                eng.check_flags()
                return state, frames, sys_state

            try:
                state, frames, sys_state = attempt()
            except _lib.NumericRangeError:   # a decision of the whole batch, in per-system mode too
                if not eng.use_exact_f32():
                    raise
                pos.copy_(pos0)
                state, frames, sys_state = attempt()
            st = state.tolist()
            self.steps_applied = st[3]
            self.cvg_count = st[0]
            counts = None
            if sys_state is not None:
                batch.sample_steps = sys_state[:, 2].to(torch.int64)
                batch.sample_stopped = sys_state[:, 1] != 0
                self.stop_step = sys_state[:, 3].to(torch.int64)
                counts = [max(int(n), 1) for n in batch.sample_steps.tolist()]
            if frames is not None:
                # frames recorded after the break are identical copies; keep the applied ones
                frames = frames[: max(self.steps_applied, 1)] if self.save_full else frames[-1:]
                self._write_trajectories(batch, frames, counts if self.save_full else None)
            if self._pending is not None and not params.get("trajectory_async", False):
                self.wait_for_trajectories()   # like the reference: the files exist when run() returns
            batch.y = torch.zeros(B, device=dev)
            batch.force = torch.zeros(N, 3, device=dev)
        finally:
            try:
                eng = self._engine()
                try:
                    eng.set_moving_atoms(None, None)
                finally:
                    if self.per_system:
                        eng.set_per_system_stop(None)
            except Exception:
                pass
            if ema:
                ema.restore()

    def _run_fused(self, eng, batch, pos, state, T: int, run, sys_state=None) -> None:
        """``run(sink)``: a sampler's whole loop in one library call.  With a ``traj_dir`` the trajectory frames leave the
        device from inside that loop (csrc/frames.hip) and a host thread writes them while the next steps compute
        (trajectory.py)."""
        sink = writer = None
        if self.traj_dir:
            from .trajectory import FrameSink, TrajectoryWriter

            sink = FrameSink(pos.device.index, pos.shape[0],
                             slots=int(self.denoising_pos_params.get("trajectory_ring_slots", 8)))
            writer = TrajectoryWriter(sink, self.traj_dir, self._traj_meta(batch), T if self.save_full else 1)
            writer.start()
        try:
            run(sink if self.save_full else None)
            if sink is not None and not self.save_full:   # final frame only (reference :474-477 with save_full False)
                sink.push(pos, torch.cuda.current_stream(pos.device))
            eng.check_flags()
        except BaseException:
            if writer is not None:   # a failed attempt (e.g. the f16x3 range was left): drop its frames,
                writer.abort()       # publish no file (temporary files deleted), wake a blocked push
                sink.abort()
                writer.join()
                sink.close()
                if writer.error is not None:
                    # the writer died first (disk full, ...): the push error ('ring was aborted') is only
                    # its echo - surface the real cause
                    raise writer.error
            raise
        if writer is not None:
            if sys_state is not None and self.save_full:   # per-system mode: a system's file holds its own applied frames
                writer.set_frame_counts([max(int(n), 1) for n in sys_state[:, 2].tolist()])
            writer.finish(max(int(state[3].item()), 1) if self.save_full else 1)
            self._pending = (writer, sink)

    # ------------------------------------------------------------------ trajectory sink
    _pending = None

    def wait_for_trajectories(self) -> None:
        """Block until the writer thread of this run has written every file (``trajectory_async`` runs return earlier)."""
        if self._pending is not None:
            writer, sink = self._pending
            self._pending = None
            try:
                writer.join_checked()
            finally:
                sink.close()

    def _traj_meta(self, batch) -> dict:
        tags = batch.tags.cpu().numpy()
        return dict(numbers=batch.atomic_numbers.cpu().numpy(), tags=tags,
                    fixed=batch.fixed.cpu().numpy() if hasattr(batch, "fixed") else np.zeros_like(tags),
                    cell=batch.cell.cpu().numpy(), natoms=batch.natoms.cpu().numpy(), names=list(self.traj_names))

    def _write_trajectories(self, batch, frames, counts=None) -> None:
        """One file per system, written once after the loop under a temporary name and then renamed (the reference's
        ``.traj_tmp`` -> ``.traj`` protocol, :66-82).  With ``ase`` importable: genuine ASE trajectories ``<name>.traj``;
        without it the same content (positions per frame, numbers, cell, tags, fixed) goes to ``<name>.npz`` - a file
        named ``.traj`` always is one.  ``counts`` (per-system mode): system b's file holds its first ``counts[b]`` frames."""
        traj_dir = Path(self.traj_dir)
        traj_dir.mkdir(exist_ok=True, parents=True)
        stack = torch.stack(frames).cpu().numpy()  # [F,N,3]
        natoms = batch.natoms.cpu().tolist()
        Z = batch.atomic_numbers.cpu().numpy()
        tags = batch.tags.cpu().numpy()
        fixed = batch.fixed.cpu().numpy() if hasattr(batch, "fixed") else np.zeros_like(tags)
        cell = batch.cell.cpu().numpy()
        try:
            import ase  # noqa: F401
            from ase import Atoms
            from ase.constraints import FixAtoms
            from ase.io import Trajectory

            have_ase = True
        except Exception:  # pragma: no cover - ase is not installed in the build image
            have_ase = False
        start = 0
        for b, (n, name) in enumerate(zip(natoms, self.traj_names)):
            sl = slice(start, start + n)
            nf = stack.shape[0] if counts is None else min(int(counts[b]), stack.shape[0])
            tmp = traj_dir / (f"{name}.traj_tmp" if have_ase else f"{name}.npz_tmp")
            if have_ase:  # pragma: no cover
                with Trajectory(tmp, mode="w") as traj:
                    for f in range(nf):
                        traj.write(Atoms(numbers=Z[sl].astype(int), positions=stack[f, sl], tags=tags[sl],
                                         cell=cell[b], constraint=FixAtoms(mask=fixed[sl].astype(bool)),
                                         pbc=[True, True, True]))
            else:
                with open(tmp, "wb") as fh:
                    np.savez(fh, positions=stack[:nf, sl], numbers=Z[sl], tags=tags[sl], fixed=fixed[sl], cell=cell[b])
            tmp.rename(tmp.with_suffix(".traj" if have_ase else ".npz"))
            start += n

    def _get_ads_output(self, pred):
        """Per-system mean over adsorbate atoms (reference :460-467); host helper for callers."""
        m = self.batch.tags == 2
        B = int(self.batch.natoms.shape[0])
        idx = self.batch.batch[m]
        tot = torch.zeros(B, pred.shape[1], dtype=pred.dtype, device=pred.device).index_add_(0, idx, pred[m])
        cnt = torch.zeros(B, dtype=pred.dtype, device=pred.device).index_add_(
            0, idx, torch.ones(idx.shape[0], dtype=pred.dtype, device=pred.device))
        return tot / cnt.clamp(min=1)[:, None]

    def compute_metrics(self, positions):
        return

    def log(self):
        return
