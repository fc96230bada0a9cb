"""Trainer-like object for sampling — the part of the reference's ``DenoisingTrainer`` that the
stepper touches (reference: adsorbdiff/trainers/sde_denoising_trainer.py:539-652, 750-813, and
denoising_torch.py:38,491-500): ``predict_denoising(batch, per_image=False)``,
``_unwrapped_model``, ``ema``, ``scaler``, ``device``, ``config["model_attributes"]`` and
``run_relaxations`` (the ``run-relaxations`` task entry, tasks/task.py:90-100).

``train_step`` is the per-batch body of the reference's training loop (sde_denoising_trainer.py:410-441 +
base_trainer.py:787-820): noising, forward, loss, backward, gradient all-reduce, clipping, AdamW, EMA — all device
arithmetic in HIP kernels (adsorbdiff_amd/train_step.py).  ``train``, ``save``, ``load_checkpoint`` and ``update_best`` come
from ``train_loop.TrainLoopMixin`` (the reference's epoch loop, checkpoint layout of base_trainer.py:456-533, 625-704, LR
schedules of ``lr_scheduler``); datasets and data loaders stay out of scope.  ``ForcesTrainer.train_step`` is the same body for the
S2EF force field (trainers/ocp_trainer.py:115-246, loss :308-356).
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Iterable, Optional

import torch

from .ml_relaxation import ml_diffuse
from .painn_denoising import PaiNN
from .scaling import ensure_fitted
from .train_loop import TrainLoopMixin


def check_traj_files(batch, traj_dir) -> bool:
    """Resume rule of the sampler: a batch is skipped iff every <traj_dir>/<sid>.traj exists
    (reference: utils/utils.py:968-973); the ase-less sink <sid>.npz counts as well."""
    if traj_dir is None:
        return False
    traj_dir = Path(traj_dir)
    return all((traj_dir / f"{sid}.traj").exists() or (traj_dir / f"{sid}.npz").exists() for sid in batch.sid)


class DenoisingTrainer(TrainLoopMixin):
    name = "ocp"   # the task validate() evaluates under: no metrics but `loss`

    def __init__(self, model: PaiNN, device="cuda:0", config: Optional[dict] = None, ema=None, relax_loader=None):
        self.device = torch.device(device)
        self.model = model.to(self.device)
        self.ema = ema
        self.scaler = None  # fp32 path; the reference's --amp autocast is not offered
        self.relax_loader = relax_loader
        self.config = config or {}
        self.config.setdefault("model_attributes", {})
        self.config["model_attributes"].setdefault("so3_denoising", bool(model.so3_denoising))
        self.config.setdefault("task", {})
        self.config.setdefault("optim", {})

    @property
    def _unwrapped_model(self):
        module = self.model
        while hasattr(module, "module"):  # DDP / OCPDataParallel wrappers
            module = module.module
        return module

    # ---------------------------------------------------------------- inference
    def _forward_denoising(self, batch):
        """Reference: sde_denoising_trainer.py:539-553."""
        if not self.config["model_attributes"].get("so3_denoising", False):
            out = self.model(batch.to(self.device))
            # the EquiformerV2 mirror always evaluates both force blocks; a one-head run reads the first
            return {"positions": out[0] if isinstance(out, tuple) else out}
        out1, out2 = self.model(batch.to(self.device))
        return {"positions": out1, "positions_free": out2}

    @torch.no_grad()
    def predict_denoising(self, data_loader, per_image: bool = True, results_file=None, disable_tqdm: bool = False):
        """Only the ``per_image=False`` form the stepper uses (reference :555-652)."""
        if per_image:
            raise NotImplementedError("per_image=True (result-file writer) is outside the sampling path")
        ensure_fitted(self._unwrapped_model, warn=True)
        self.model.eval()
        if self.ema:
            self.ema.store()
            self.ema.copy_to()
        try:
            out = self._forward_denoising(data_loader)
            predictions = {"positions": out["positions"].detach()}
            if "positions_free" in out:
                predictions["positions_free"] = out["positions_free"].detach()
        finally:
            if self.ema:
                self.ema.restore()
        return predictions

    # ---------------------------------------------------------------- training
    def setup_training(self, denoising_pos_params: dict, lr: float = 1e-3, weight_decay: float = 0.001,
                       clip_grad_norm: float = 100.0, ema_decay: float = 0.999, tables=None,
                       noise_on_device: bool = False, noise_seed: int = 0, reproducible: bool = False) -> None:
        """Optimizer / EMA / noising parameters; defaults = configs/denoising/painn_so3.yml:56-83 (AdamW, weight decay
        1e-3 except no_weight_decay() names, clip 100, EMA 0.999).  ``noise_on_device``: ``train_step`` and ``validate``
        noise through ``noising.DeviceNoiser`` (counter-based draws keyed by ``noise_seed``, the step number and
        ``noising.noise_keys(batch)``: no host round trip, and a system's noise does not depend on its batch or rank);
        off (default): the reference's stream order on the host.  ``reproducible``: ``MultiTensorAdamW`` (ordered gradient
        norm, device step counter, torch's state layout and schedulers) in place of ``FusedAdamW``, and the embedding
        gradient summed in a fixed order: with ``noise_on_device`` a run resumed from a checkpoint retraces the
        uninterrupted one to the bit."""
        from .exponential_moving_average import ExponentialMovingAverage
        from .train_step import FusedAdamW, MultiTensorAdamW, PaiNNTrainStep

        from .equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos

        self.denoising_pos_params = dict(denoising_pos_params)
        if isinstance(self._unwrapped_model, EquiformerV2S_OC20_DenoisingPos):
            # the same contract, the EquiformerV2 operators (eqv2_train_step.py); its dropout masks are keyed by
            # (noise_seed, the trainer's step counter), so a resumed run draws the masks of the uninterrupted one
            from .eqv2_train_step import EqV2TrainStep

            self.train_engine = EqV2TrainStep(self._unwrapped_model, self.device, igso3=tables)
            self.train_engine.mask_seed = int(noise_seed)
        else:
            self.train_engine = PaiNNTrainStep(self._unwrapped_model, self.device, igso3=tables)
        self.train_engine.ordered_embedding_backward = bool(reproducible)
        self.noiser = None
        if noise_on_device:
            from .noising import DeviceNoiser

            self.noiser = DeviceNoiser(self.denoising_pos_params, self.train_engine.igso3, self.device, seed=noise_seed)
        self.noise_step = 0
        if ema_decay:
            self.ema = ExponentialMovingAverage(self._unwrapped_model.parameters(), ema_decay)
        self.optimizer = (MultiTensorAdamW if reproducible else FusedAdamW)(
            self._unwrapped_model, lr=lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm, ema=self.ema)
        self.scheduler = None
        self.step = 0

    def _noise(self, batch, params, tables, noise_step=None, draws=None):
        """The schedule ``config["model_attributes"]["so3_denoising"]`` selects, as the reference's loop does
        (sde_denoising_trainer.py:416-421): on the device where ``setup_training`` asked for it, else the host mirrors.
        The device noising numbers its calls with ``self.noise_step`` (``noise_step`` overrides; ``draws`` replaces the
        generator)."""
        from .noising import ads_COM_gaussian_schedule, tr_so3_schedule

        so3 = self.config["model_attributes"].get("so3_denoising", False)
        noiser = getattr(self, "noiser", None)
        if noiser is None:
            if draws is not None or noise_step is not None:
                raise ValueError("draws= / noise_step= need setup_training(noise_on_device=True)")
            return tr_so3_schedule(batch, params, tables) if so3 else ads_COM_gaussian_schedule(batch, params)
        if noise_step is None and draws is None:   # supplied rows or a supplied number leave the counter alone
            noise_step = self.noise_step
            self.noise_step += 1
        return (noiser.tr_so3 if so3 else noiser.com)(batch, step=noise_step, draws=draws)

    def _score_targets(self, batch) -> dict:
        keys = ("tr_sigma", "rot_sigma", "tr_score", "rot_score") \
            if self.config["model_attributes"].get("so3_denoising", False) else ("tr_sigma", "tr_score")
        targets = {k: getattr(batch, k) for k in keys}
        if "rot_sigma" in targets and getattr(batch, "rot_norm", None) is not None:
            targets["rot_norm"] = batch.rot_norm   # from the device noising: the loss needs no look-up of its own
        return targets

    def train_step(self, batch, noised: bool = False, noise_step: Optional[int] = None, draws=None) -> dict:
        """One optimisation step on ``batch`` (clean positions unless ``noised``).  Multi-GPU: one process per GPU, each
        with its own batch; gradients are averaged with a bucketed all-reduce (RCCL over xGMI under backend nccl).
        The noising and the loss follow the model: two heads, ``tr_so3_schedule`` and both score terms; one head
        (``so3_denoising=False``), ``ads_COM_gaussian_schedule`` and the translation term.  ``noise_step`` / ``draws``:
        with ``noise_on_device``, the step number of the draws (default: this trainer's counter) or the rows themselves."""
        import torch.distributed as dist

        from .train_step import GradientReducer

        self.model.train()
        batch = batch.to(self.device)
        if hasattr(batch, "pos_relaxed"):
            batch.pos = batch.pos_relaxed
        if not noised:
            batch = self._noise(batch, self.denoising_pos_params, self.train_engine.igso3, noise_step, draws)
        targets = self._score_targets(batch)
        if hasattr(self.train_engine, "mask_step"):
            self.train_engine.mask_step = int(self.step)
        self.train_engine.zero_grad()
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # the buckets' all-reduces are issued from inside the backward (heads, then layer by layer) and overlap with it
        reducer = GradientReducer(self._unwrapped_model, world)
        loss = self.train_engine.loss_and_grad(batch, targets, grads_ready=reducer.ready if world > 1 else None)
        # NaN policy of the reference loop (sde_denoising_trainer.py:428-440), mirrored: a step whose loss is NaN is
        # skipped (`continue`: warning, no update; the reference's `nan_count > 10` test sits behind the reset and can never
        # fire, so there is no such stop here either); a loss above 1e6 - an Inf loss included, isnan() is False for it -
        # logs a warning and STOPS the epoch loop (`break`): returned as "stop": True, never raised.  All ranks must take
        # the same branch, so ONE two-element flag (NaN, too high) is MAX-reduced over the ranks and read back once; the
        # fused optimizer additionally turns an update with a non-finite gradient norm into a no-op on the device
        # (csrc/train.hip: tr_adamw_kernel).
        l0 = loss.detach().reshape(-1)
        flag = torch.stack([torch.isnan(l0).any(), l0[0] > 1e6]).to(torch.int32)
        if world > 1:
            flag = flag if dist.get_backend() != "gloo" else flag.cpu()
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        is_nan, too_high = (bool(v) for v in flag.tolist())    # the step's single device-to-host read
        if is_nan:
            logging.warning("NaN loss detected, skipping step")
            self.nan_count = getattr(self, "nan_count", 0) + 1
            reducer.finish()   # every rank takes this branch: drain the buckets already in flight
            self.train_engine.zero_grad()
            return {"loss": loss, "grad_norm": None, "skipped": True, "stop": False}
        self.nan_count = 0
        if too_high:
            logging.warning("Loss too high: %s", float(l0[0]))
            reducer.finish()
            self.train_engine.zero_grad()
            return {"loss": loss, "grad_norm": None, "skipped": True, "stop": True}
        if world > 1 and loss.is_cuda:   # what the backward did not hide: time spent waiting for the last buckets
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            reducer.finish()
            e1.record()
            self.allreduce_wait_events = getattr(self, "allreduce_wait_events", [])[-63:] + [(e0, e1)]
        else:
            reducer.finish()
        grad_norm = self.optimizer.step()
        self.step += 1
        return {"loss": loss, "grad_norm": grad_norm, "skipped": False, "stop": False}

    # ---------------------------------------------------------------- evaluation
    @torch.no_grad()
    def validate(self, batches: Optional[Iterable] = None, noised: bool = False, split: str = "val",
                 disable_tqdm: bool = True, noise_step: Optional[int] = None) -> dict:
        """The reference's ``validate`` (sde_denoising_trainer.py:286-368): per batch ``pos_relaxed`` for the positions,
        ``tr_so3_schedule`` (unless ``noised``: the batch already carries its noise and scores), the inference forward and the
        score loss without a backward.  This trainer evaluates under the task "ocp", which has no metrics, so the result is
        ``{"loss": {"metric", "total", "numel"}}``: the mean over the batches, summed over the ranks.  The losses are added
        up on the device; the pass ends with one all-reduce and one read (the rotation score's norm is looked up on the
        device).  A one-head model (``so3_denoising=False``) is noised by ``ads_COM_gaussian_schedule`` and scored by the
        translation term alone.  With ``setup_training(noise_on_device=True)`` the batches are noised on the device, batch i
        with step number ``noise_step + i`` (default: the trainer's counter, which advances).  ``batches``: default
        ``val_loader`` / ``test_loader`` by ``split``; ``disable_tqdm`` is accepted for the reference's signature, there is
        no progress bar."""
        import ctypes as C

        from . import lib as _lib
        from .evaluator import DeviceMetrics, Evaluator, atom_offsets
        from .noising import device_score_norm
        from .so3_tables import Igso3Tables

        so3 = bool(self.config["model_attributes"].get("so3_denoising", False))
        ensure_fitted(self._unwrapped_model, warn=True)
        engine = getattr(self, "train_engine", None)
        tables = engine.igso3 if engine is not None else (Igso3Tables.shared() if so3 else None)
        params = getattr(self, "denoising_pos_params", None) or self.config["optim"].get("denoising_pos_params")
        if batches is None:
            batches = getattr(self, "val_loader" if split == "val" else "test_loader")
        evaluator = Evaluator(task="ocp")   # no metrics: `loss` only
        lib = _lib.load()
        dm = DeviceMetrics(self.device)
        self.model.eval()
        if self.ema:
            self.ema.store()
            self.ema.copy_to()
        try:
            for i, batch in enumerate(batches):
                batch = batch.to(self.device)
                if hasattr(batch, "pos_relaxed"):
                    batch.pos = batch.pos_relaxed
                if not noised:
                    batch = self._noise(batch, params, tables, None if noise_step is None else noise_step + i)
                out = self._forward_denoising(batch)
                if getattr(batch, "tags", None) is None:
                    raise ValueError("batch.tags is required (tag 2 marks the adsorbate)")
                tags = batch.tags.to(self.device, torch.int32).contiguous()
                atom_offset = atom_offsets(batch.natoms, self.device)
                B, N = int(batch.natoms.numel()), int(batch.pos.shape[0])
                t = {k: v.to(self.device, torch.float32).contiguous() for k, v in self._score_targets(batch).items()}
                f1 = out["positions"].contiguous()
                loss = torch.empty(3, device=self.device)
                grads = torch.empty(2, N, 3, device=self.device)   # the loss entry writes its gradients: not used here
                scratch = torch.empty(2 * B + 16, device=self.device)
                stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
                if so3:
                    rot_norm = t["rot_norm"].reshape(-1) if "rot_norm" in t else \
                        device_score_norm(t["rot_sigma"], tables, self.device)
                    f2 = out["positions_free"].contiguous()
                    with torch.cuda.device(self.device):
                        _lib.check(lib.adf_op_score_loss(
                            f1.data_ptr(), f2.data_ptr(), tags.data_ptr(), atom_offset.data_ptr(),
                            t["tr_sigma"].data_ptr(), t["rot_sigma"].data_ptr(), t["tr_score"].data_ptr(),
                            t["rot_score"].data_ptr(), rot_norm.data_ptr(), loss.data_ptr(), grads[0].data_ptr(),
                            grads[1].data_ptr(), B, scratch.data_ptr(), stream))
                else:
                    with torch.cuda.device(self.device):
                        _lib.check(lib.adf_op_score_loss_tr(
                            f1.data_ptr(), tags.data_ptr(), atom_offset.data_ptr(), t["tr_sigma"].data_ptr(),
                            t["tr_score"].data_ptr(), loss.data_ptr(), grads[0].data_ptr(), B, scratch.data_ptr(), stream))
                dm.add_value("loss", loss[:1])
        finally:
            if self.ema:
                self.ema.restore()
        return dm.all_reduce().result(evaluator.metric_names() + ["loss"])

    # ---------------------------------------------------------------- sampling entry
    def run_relaxations(self, batches: Optional[Iterable] = None):
        """``--mode run-relaxations`` (reference :750-813): for every batch of the relax loader not
        already finished on disk, run the diffusion sampler.  Returns the list of sampled batches."""
        self.model.eval()
        task = self.config["task"]
        params = self.config["optim"].get("denoising_pos_params", {})
        traj_dir = task.get("relax_opt", {}).get("traj_dir", None)
        out = []
        for batch in (batches if batches is not None else self.relax_loader):
            if check_traj_files(batch, traj_dir):
                logging.info(f"Skipping batch: {batch.sid}")
                continue
            out.append(
                ml_diffuse(
                    batch=batch, model=self, denoising_pos_params=params, traj_dir=traj_dir,
                    save_full_traj=task.get("save_full_traj", True), device=str(self.device),
                    transform=None,
                )
            )
        return out


class Normalizer:
    """Reference: modules/normalizer.py:13-60 (mean / std of a target; ``denorm`` = x * std + mean)."""

    def __init__(self, mean=0.0, std=1.0, device="cpu") -> None:
        self.mean = torch.as_tensor(mean).to(device)
        self.std = torch.as_tensor(std).to(device)

    def to(self, device) -> None:
        self.mean = self.mean.to(device)
        self.std = self.std.to(device)

    def norm(self, x):
        return torch.div(torch.sub(x, self.mean), self.std)

    def denorm(self, x):
        """the model's normalised output in target units"""
        return torch.add(torch.mul(x, self.std), self.mean)

    def state_dict(self):
        return {"mean": self.mean, "std": self.std}

    def load_state_dict(self, state_dict) -> None:
        self.mean = state_dict["mean"].to(self.mean.device)
        self.std = state_dict["std"].to(self.mean.device)


# old checkpoint keys of the normalizers -> output targets (base_trainer.py:518-530)
_NORMALIZER_KEYS = {"target": "energy", "grad_target": "forces"}


class ForcesTrainer(TrainLoopMixin):
    """The part of the reference's S2EF trainer (trainers/ocp_trainer.py:405-460, base_trainer.py:353-362) that
    ``ml_relax`` / ``TorchCalc`` touch: ``predict(batch, per_image=False)`` -> ``{"energy", "forces"}`` with the EMA weights
    swapped in for the forward and the normalizers' ``denorm`` applied, ``_unwrapped_model``, ``normalizers``.
    ``normalizers``: ``{"energy" | "target": {"mean", "stdev"}, ...}`` as in the
    dataset config (``transforms.normalizer``), or ready ``Normalizer`` objects."""

    name = "s2ef"   # the task validate() evaluates under

    def __init__(self, model, device="cuda:0", normalizers: Optional[dict] = None, ema=None, config: Optional[dict] = None):
        self.device = torch.device(device)
        self.model = model.to(self.device)
        self.ema = ema
        self.scaler = None
        self.config = dict(config or {})
        self.normalizers = {}
        for key, val in (normalizers or {}).items():
            target = _NORMALIZER_KEYS.get(key, key)
            if isinstance(val, Normalizer):
                self.normalizers[target] = val
            else:
                self.normalizers[target] = Normalizer(val.get("mean", 0), val.get("stdev", val.get("std", 1)), self.device)

    @property
    def _unwrapped_model(self):
        module = self.model
        while hasattr(module, "module"):
            module = module.module
        return module

    def load_normalizers(self, state: dict) -> None:
        """Checkpoint ``normalizers`` entry (base_trainer.py:518-530): ``target`` -> energy, ``grad_target`` -> forces;
        keys without a configured normalizer are ignored, as in the reference."""
        for key, sd in state.items():
            target = _NORMALIZER_KEYS.get(key, key)
            if target in self.normalizers:
                self.normalizers[target].load_state_dict(sd)

    # ---------------------------------------------------------------- training
    def setup_training(self, lr: float, weight_decay: float = 0.001, clip_grad_norm: float = 10.0, ema_decay: float = 0.999,
                       energy_coefficient: float = 1, force_coefficient: float = 30, loss_energy: str = "mae",
                       loss_force: str = "l2mae", train_on_free_atoms: bool = True, reproducible: bool = False,
                       mask_seed: int = 0, force_objective: str = "direct") -> None:
        """Optimizer / EMA / objective of ``train_step``.  AdamW with weight decay except ``no_weight_decay()`` names;
        clip 10 and EMA 0.999 as configs/relaxation/gemnet_oc/gemnet_relax.yml:107-108; coefficients and
        ``train_on_free_atoms`` as the reference's defaults (utils/utils.py:1227,1257, base_trainer.py:382-390; the shipped
        YAMLs pass force_coefficient 100).  The targets are normalised with this trainer's ``normalizers``.  Only the loss
        names the shipped configs use are offered (energy "mae", forces "l2mae"); any other name is refused here.
        ``reproducible``: as ``DenoisingTrainer.setup_training``.  An ``EquiformerV2_OC20`` trains through
        ``EqV2S2EFTrainStep``, everything else through ``PaiNNS2EFTrainStep``; ``mask_seed`` keys the
        EquiformerV2 step's dropout / drop-path masks together with the trainer's step counter, so a resumed run draws the
        masks of the uninterrupted one.  ``force_objective``: ``"direct"`` puts the force head's output into the loss;
        ``"energy_gradient"`` puts ``-d(energy.sum())/d(pos)`` there (``PaiNNGradForceTrainStep``, DESIGN.md 6j: the force
        targets are then normalised with mean 0 and the energy normaliser's stdev) and requires
        ``model.force_mode == "energy_gradient"``, so that ``validate`` / ``predict`` / ``ml_relax`` evaluate what was
        trained; it is not offered for EquiformerV2."""
        from .equiformer_v2_oc20 import EquiformerV2_OC20
        from .exponential_moving_average import ExponentialMovingAverage
        from .train_step import FusedAdamW, MultiTensorAdamW, PaiNNGradForceTrainStep, PaiNNS2EFTrainStep

        if force_objective not in ("direct", "energy_gradient"):
            raise ValueError(f"force_objective is 'direct' or 'energy_gradient', got {force_objective!r}")

        if loss_energy != "mae" or loss_force != "l2mae":
            raise NotImplementedError(
                f"the S2EF step offers energy loss 'mae' with force loss 'l2mae', got {loss_energy!r} / {loss_force!r} "
                "(mse, atomwisel2 and torch module names are not offered)")
        step_class = PaiNNS2EFTrainStep
        if isinstance(self._unwrapped_model, EquiformerV2_OC20):
            if force_objective == "energy_gradient":
                raise NotImplementedError("force_objective='energy_gradient' is not offered for EquiformerV2")
            from .eqv2_train_step import EqV2S2EFTrainStep as step_class
        elif force_objective == "energy_gradient":
            if getattr(self._unwrapped_model, "force_mode", "direct") != "energy_gradient":
                raise ValueError(
                    "force_objective='energy_gradient' requires model.force_mode='energy_gradient' (it is "
                    f"{getattr(self._unwrapped_model, 'force_mode', 'direct')!r}): set both switches, so that validate / "
                    "predict / ml_relax evaluate the forces that were trained")
            step_class = PaiNNGradForceTrainStep
        self.train_engine = step_class(self._unwrapped_model, self.device, normalizers=self.normalizers,
                                       energy_coefficient=energy_coefficient, force_coefficient=force_coefficient,
                                       train_on_free_atoms=train_on_free_atoms)
        if hasattr(self.train_engine, "mask_seed"):
            self.train_engine.mask_seed = int(mask_seed)
        self.train_engine.ordered_embedding_backward = bool(reproducible)
        # a falsy ema_decay trains without an EMA: one that was loaded or set up earlier is dropped, not updated on
        self.ema = ExponentialMovingAverage(self._unwrapped_model.parameters(), ema_decay) if ema_decay else None
        self.optimizer = (MultiTensorAdamW if reproducible else FusedAdamW)(
            self._unwrapped_model, lr=lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm, ema=self.ema)
        self.scheduler = None
        self.step = 0

    def train_step(self, batch) -> dict:
        """One optimisation step on ``batch`` (targets ``energy``, ``forces``, ``fixed``): the per-batch body of
        ``OCPTrainer.train`` (trainers/ocp_trainer.py:115-246; update: base_trainer.py:787-820).  Multi-GPU: one process
        per GPU, each with its own batch; the system and loss-atom counts are summed over the ranks before the loss (the
        divisors of DDPLoss, modules/loss.py:88-99) and the gradients averaged with the bucketed all-reduce of the
        denoiser's trainer.  A non-finite loss skips the update on every rank (the reference zeroes non-finite predictions
        instead, loss.py:77-81); the OCP loop has no "loss too high" stop, so ``stop`` is always False."""
        import torch.distributed as dist

        from .train_step import GradientReducer

        eng = self.train_engine
        self.model.train()
        batch = batch.to(self.device)
        if hasattr(eng, "mask_step"):
            eng.mask_step = int(self.step)
        eng.zero_grad()
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        counts = None
        if world > 1:
            # one all-reduce of (systems, loss atoms, 1): the sum of the ones is the world size; no host read
            n_sys = int(batch.natoms.numel())
            fixed = getattr(batch, "fixed", None)
            if eng.train_on_free_atoms and fixed is not None:
                n_loss = (fixed == 0).sum().to(torch.int64)
            else:
                n_loss = torch.tensor(int(batch.pos.shape[0]), dtype=torch.int64, device=self.device)
            counts = torch.stack([torch.tensor(n_sys, dtype=torch.int64, device=self.device), n_loss.reshape(()),
                                  torch.tensor(1, dtype=torch.int64, device=self.device)])
            if dist.get_backend() == "gloo" and counts.is_cuda:   # test configuration: several ranks on one GPU
                host = counts.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM)
                counts = host.to(self.device)
            else:
                dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        reducer = GradientReducer(self._unwrapped_model, world)
        loss = eng.loss_and_grad(batch, grads_ready=reducer.ready if world > 1 else None, counts=counts)
        # all ranks must take the same branch: one flag, MAX-reduced, read back once (the step's single device-to-host
        # read); the fused optimizer additionally turns an update with a non-finite gradient norm into a no-op
        flag = (~torch.isfinite(loss.detach())).any().reshape(1).to(torch.int32)
        if world > 1:
            flag = flag if dist.get_backend() != "gloo" else flag.cpu()
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        reducer.finish()
        if bool(flag.item()):
            logging.warning("non-finite loss detected, skipping step")
            eng.zero_grad()
            return {"loss": loss, "grad_norm": None, "skipped": True, "stop": False, "metrics": eng.metrics}
        grad_norm = self.optimizer.step()
        self.step += 1
        return {"loss": loss, "grad_norm": grad_norm, "skipped": False, "stop": False, "metrics": eng.metrics}

    # ---------------------------------------------------------------- evaluation
    def _objective(self) -> dict:
        """The S2EF objective's settings: ``setup_training``'s, or its defaults where it was not called."""
        eng = getattr(self, "train_engine", None)
        if eng is not None:
            return dict(norm=dict(eng.norm), energy_coefficient=eng.energy_coefficient, force_coefficient=eng.force_coefficient,
                        train_on_free_atoms=eng.train_on_free_atoms)
        norm = {}
        for key in ("energy", "forces"):
            nz = self.normalizers.get(key)
            norm[key] = (float(nz.mean), float(nz.std)) if nz else (0.0, 1.0)
        return dict(norm=norm, energy_coefficient=1.0, force_coefficient=30.0, train_on_free_atoms=True)

    def _rank_counts(self, num_systems: int, num_atoms: int, fixed, free_only: bool):
        """Device int64 (systems, loss atoms, 1) summed over the ranks - the divisors of DDPLoss, as ``train_step`` forms
        them - or None for one rank."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
            return None
        if free_only and fixed is not None:
            n_loss = (fixed == 0).sum().to(torch.int64)
        else:
            n_loss = torch.tensor(num_atoms, dtype=torch.int64, device=self.device)
        counts = torch.stack([torch.tensor(num_systems, dtype=torch.int64, device=self.device), n_loss.reshape(()),
                              torch.tensor(1, dtype=torch.int64, device=self.device)])
        if dist.get_backend() == "gloo" and counts.is_cuda:   # test configuration: several ranks on one GPU
            host = counts.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            return host.to(self.device)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        return counts

    @torch.no_grad()
    def validate(self, batches: Optional[Iterable] = None, split: str = "val", disable_tqdm: bool = True) -> dict:
        """``BaseTrainer.validate`` for the S2EF task (trainers/base_trainer.py:712-785 with
        ``OCPTrainer._compute_metrics``, ocp_trainer.py:358-402): per batch the inference forward ``predict`` uses (EMA
        weights swapped in, restored at the end), the objective of ``train_step`` without its backward, and the eight
        metrics of ``Evaluator.task_metrics["s2ef"]`` over the free atoms, all added up on the device; the pass ends with one
        all-reduce over the ranks and one read.  Returns ``{name: {"metric", "total", "numel"}}`` for the eight names and
        ``loss`` (the mean of the batches' losses).  With ``force_mode == "energy_gradient"`` the forces are denormalised as
        ``predict`` denormalises them (energy std, no mean).  A system without a free atom counts a force maximum of 0
        (the reference raises).  ``batches``: default ``val_loader`` / ``test_loader`` by ``split``."""
        import ctypes as C

        from . import lib as _lib
        from .evaluator import DeviceMetrics, Evaluator, atom_offsets

        ensure_fitted(self._unwrapped_model, warn=True)
        model = self._unwrapped_model
        obj = self._objective()
        (mean_e, std_e), (mean_f, std_f) = obj["norm"]["energy"], obj["norm"]["forces"]
        norm_f_eval = (0.0, std_e) if getattr(model, "force_mode", "direct") == "energy_gradient" else (mean_f, std_f)
        if batches is None:
            batches = getattr(self, "val_loader" if split == "val" else "test_loader")
        evaluator = Evaluator(task="s2ef")
        lib = _lib.load()
        dm = DeviceMetrics(self.device)
        self.model.eval()
        if self.ema is not None:
            self.ema.store()
            self.ema.copy_to()
        try:
            for batch in batches:
                batch = batch.to(self.device)
                out = self.model(batch)
                if "forces" not in out:
                    raise NotImplementedError("the s2ef metrics need forces (regress_forces or force_mode='energy_gradient')")
                atom_offset = atom_offsets(batch.natoms, self.device)
                fixed = batch.fixed.to(self.device, torch.int32).contiguous() if getattr(batch, "fixed", None) is not None else None
                B, N = int(batch.natoms.numel()), int(batch.pos.shape[0])
                e_pred, f_pred = out["energy"].reshape(B).contiguous(), out["forces"].reshape(N, 3).contiguous()
                e_tgt = batch.energy.to(self.device, torch.float32).reshape(-1).contiguous()
                f_tgt = batch.forces.to(self.device, torch.float32).reshape(N, 3).contiguous()
                if e_tgt.numel() != B:
                    raise ValueError(f"batch.energy has {e_tgt.numel()} entries for {B} systems")
                free_only = obj["train_on_free_atoms"]
                if free_only and fixed is None:
                    raise ValueError("batch.fixed is required with train_on_free_atoms")
                counts = self._rank_counts(B, N, fixed, free_only)
                loss, unused = torch.empty(3, device=self.device), torch.empty(2, device=self.device)
                grads = torch.empty(B + 3 * N, device=self.device)   # the loss entry writes dE, dF: not used here
                scratch = torch.empty(int(lib.adf_op_s2ef_loss_scratch(B)), device=self.device)
                with torch.cuda.device(self.device):
                    _lib.check(lib.adf_op_s2ef_loss(
                        e_pred.data_ptr(), f_pred.data_ptr(), e_tgt.data_ptr(), f_tgt.data_ptr(),
                        fixed.data_ptr() if fixed is not None else None, atom_offset.data_ptr(), B,
                        1 if free_only else 0, C.c_float(mean_e), C.c_float(std_e), C.c_float(mean_f), C.c_float(std_f),
                        C.c_float(obj["energy_coefficient"]), C.c_float(obj["force_coefficient"]),
                        counts.data_ptr() if counts is not None else None, loss.data_ptr(), grads.data_ptr(),
                        grads[B:].data_ptr(), unused.data_ptr(), scratch.data_ptr(),
                        C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
                dm.add_s2ef(e_pred, f_pred, e_tgt, f_tgt, atom_offset, fixed=fixed, free_only=True,
                            norm_energy=(mean_e, std_e), norm_forces=norm_f_eval)
                dm.add_value("loss", loss[:1])
        finally:
            if self.ema is not None:
                self.ema.restore()
        return dm.all_reduce().result(evaluator.metric_names() + ["loss"])

    @torch.no_grad()
    def evaluate_relaxed(self, relaxed_batch, metrics: Optional[tuple] = None) -> tuple:
        """The ``split == "val"`` block of ``OCPTrainer.run_relaxations`` (ocp_trainer.py:607-642) for what ``ml_relax`` /
        ``ml_relax_sharded`` return, once the DFT targets ``pos_relaxed`` and ``y_relaxed`` are attached: ``pos`` against
        ``pos_relaxed`` over the free atoms (is2rs) and ``y`` against ``y_relaxed`` (is2re), added into two ``DeviceMetrics``.
        ``metrics``: the pair a previous call returned (None: two fresh ones); returns ``(is2rs, is2re)``.  Nothing is read
        back: ``result(Evaluator(task).metric_names())`` of each, after an ``all_reduce()`` when several ranks relaxed."""
        from .evaluator import DeviceMetrics, atom_offsets

        is2rs, is2re = metrics if metrics is not None else (DeviceMetrics(self.device), DeviceMetrics(self.device))
        b = relaxed_batch.to(self.device)
        fixed = b.fixed.to(self.device, torch.int32).contiguous() if getattr(b, "fixed", None) is not None else None
        B = int(b.natoms.numel())
        is2rs.add_is2rs(b.pos, b.pos_relaxed, b.cell.reshape(B, 3, 3), atom_offsets(b.natoms, self.device), fixed=fixed)
        is2re.add_is2re(b.y.reshape(-1), b.y_relaxed.reshape(-1))
        return is2rs, is2re

    @torch.no_grad()
    def predict(self, data_loader, per_image: bool = False, results_file=None, disable_tqdm: bool = False):
        if per_image:
            raise NotImplementedError("per_image=True (result-file writer) is outside the relaxation path")
        ensure_fitted(self._unwrapped_model, warn=True)
        self.model.eval()
        if self.ema is not None:
            self.ema.store()
            self.ema.copy_to()
        try:
            out = self.model(data_loader.to(self.device) if hasattr(data_loader, "to") else data_loader)
            predictions = {}
            # forces that are the gradient of the model's energy stay the gradient of the energy returned here: scaled by the
            # energy normaliser's std (no mean), and the forces normaliser is not applied
            gradient_forces = getattr(self._unwrapped_model, "force_mode", "direct") == "energy_gradient"
            for key in ("energy", "forces"):
                if key not in out:
                    continue
                pred = out[key]
                if key == "forces" and gradient_forces:
                    if self.normalizers.get("energy", False):
                        pred = torch.mul(pred, self.normalizers["energy"].std)
                elif self.normalizers.get(key, False):
                    pred = self.normalizers[key].denorm(pred)
                predictions[key] = pred.detach()
        finally:
            if self.ema is not None:
                self.ema.restore()
        return predictions
