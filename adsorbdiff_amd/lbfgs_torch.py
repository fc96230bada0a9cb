"""``LBFGS`` / ``TorchCalc`` — the batched L-BFGS relaxer of ``ml_relax`` on the device.

Drop-in for ``adsorbdiff.relaxation.optimizers.lbfgs_torch`` (reference: relaxation/optimizers/lbfgs_torch.py:22-240):
same constructor signatures, same ``run(fmax, steps) -> batch`` contract (``batch.pos`` relaxed in place, ``batch.y`` the
energies and ``batch.force`` the unconstrained forces of one final forward), same iteration rule (a convergence check
every iteration, no step on the last one).  The optimizer state and arithmetic live in the HIP library
(``csrc/lbfgs.hip``, ``adf_lbfgs_*``): fp64 history rings, the batch-global two-loop recursion with fixed-order
reductions, ``determine_step``, the skip of a near-zero step and the masked position update.  The optimizer reads one
int32 from the device per iteration (the all-converged flag), plus the [B] max forces when INFO logging is on.

The optimizer is model-agnostic: any ``TorchCalc`` whose trainer's ``predict`` returns forces on the ROCm device works
(the S2EF PaiNN of ``adsorbdiff_amd.painn`` through ``trainer.ForcesTrainer``, or any torch model).

Two modes.  The default is the reference's recursion: the systems of one batch are coupled through dot products over the
whole flattened batch (one ``rho``, one ``alpha``, one skip decision), so a relaxation split over several batches or
devices does not reproduce the single run.  With ``per_system=True`` every system keeps its own history, step counter
and decisions (``adf_lbfgs_set_per_system``): a system takes exactly the steps the reference's ``LBFGS`` would take if it
were alone in its batch, and the summation order of its dot products depends on its atom count alone.  Given a force
model whose rows do not depend on the other systems of the batch, a per-system relaxation is then bit-identical alone, in
any batch, after ``ml_relax``'s out-of-memory split and on any shard (``ml_relaxation.ml_relax_sharded``).
``early_stop_batch`` cannot be combined with it.

Trajectories (``traj_dir``): ``<sid>.npz`` per system with ``positions`` [F, n, 3], ``energy`` [F], ``forces`` [F, n, 3]
(the constrained fp64 forces the optimizer saw) plus ``numbers``, ``tags``, ``fixed`` and ``cell``; frames follow the
reference's rule (:114-122, 204-212): with ``save_full_traj`` every iteration of a system that has not converged yet,
otherwise the first and the last iteration.  Written as ``<sid>.npz_tmp`` and renamed once the run has finished.
"""
from __future__ import annotations

import ctypes as C
import logging
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import lib as _lib


class LBFGS:
    # the reference's constructor signature; force_consistent is accepted and unused, as there
    def __init__(
        self,
        batch,
        model: "TorchCalc",
        maxstep: float = 0.01,
        memory: int = 100,
        damping: float = 0.25,
        alpha: float = 100.0,
        force_consistent=None,
        device: str = "cuda:0",
        save_full_traj: bool = True,
        traj_dir: Optional[Path] = None,
        traj_names=None,
        early_stop_batch: bool = False,
        per_system: bool = False,
    ) -> None:
        if per_system and early_stop_batch:
            raise ValueError("per_system cannot be combined with early_stop_batch: it moves converged systems while others "
                             "run, so a system alone and in a batch would differ")
        if traj_dir is not None and not traj_names:
            raise AssertionError("traj_dir needs traj_names: one trajectory file per system")
        unwrapped = getattr(model.model, "_unwrapped_model", None)
        self.otf_graph = getattr(unwrapped, "otf_graph", True)
        if not self.otf_graph:
            raise ValueError("the device L-BFGS runs models that build their graph on the fly (otf_graph=True)")
        self.batch, self.model = batch, model
        self.memory, self.maxstep, self.damping, self.alpha = memory, maxstep, damping, alpha
        self.H0 = 1.0 / alpha
        self.force_consistent = force_consistent
        self.device = torch.device(device)
        self.save_full, self.early_stop_batch, self.per_system = save_full_traj, early_stop_batch, bool(per_system)
        self.traj_dir = None if traj_dir is None else Path(traj_dir)
        self.traj_names = traj_names
        logging.info("iteration, then the max |force| of every system (eV/A)")
        self.lib = _lib.load()
        self.handle = None
        self.max_force_log = []   # device f64 [B] per iteration (the update masks are max_force >= fmax)

    # ------------------------------------------------------------------ device state
    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _setup(self) -> None:
        b = self.batch
        if not b.pos.is_cuda:
            raise RuntimeError(f"batch.pos is on {b.pos.device}: the device L-BFGS has no CPU fallback")
        self.device = b.pos.device
        if b.pos.dtype != torch.float32 or not b.pos.is_contiguous():
            b.pos = b.pos.to(torch.float32).contiguous()
        natoms = b.natoms.to(self.device, torch.int64).reshape(-1)
        self.num_systems = int(natoms.shape[0])
        self.num_atoms = int(b.pos.shape[0])
        self.atom_offset = torch.zeros(self.num_systems + 1, dtype=torch.int32, device=self.device)
        self.atom_offset[1:] = torch.cumsum(natoms, 0).to(torch.int32)
        self.atom_batch = b.batch.to(self.device, torch.int64)
        self.close()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_create(self.num_atoms, self.num_systems, int(self.memory), float(self.maxstep),
                                                 float(self.damping), float(self.alpha), 1 if self.early_stop_batch else 0,
                                                 C.byref(h)))
        self.handle = h
        if self.per_system:
            self.set_per_system(True)
        self._max_force = torch.empty(self.num_systems, dtype=torch.float64, device=self.device)
        self._all_conv = torch.empty(1, dtype=torch.int32, device=self.device)
        self._all_conv_host = torch.empty(1, dtype=torch.int32, pin_memory=True)

    def close(self) -> None:
        if getattr(self, "handle", None):
            with torch.cuda.device(self.device):
                torch.cuda.current_stream(self.device).synchronize()
                self.lib.adf_lbfgs_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ reference interface
    def get_energy_and_forces(self, apply_constraint: bool = True):
        return self.model.get_energy_and_forces(self.batch, apply_constraint)

    def set_positions(self, update, update_mask) -> None:
        """Move the batch by ``update`` (f64 [N,3]) in f32, masked unless early_stop_batch (reference :63-68).  The
        optimizer's own update runs on the device; this is for callers that move the batch by hand."""
        delta = update.to(torch.float32)
        if not self.early_stop_batch:
            delta = delta.masked_fill(~update_mask.reshape(-1, 1), 0.0)
        self.batch.pos.add_(delta)

    def check_convergence(self, iteration, forces=None, energy=None):
        """Reference :70-88: (update_mask [N] bool on the device, energy, forces).  The per-system max force and the mask
        stay on the device (``adf_lbfgs_converge``); the mask is also kept in the handle for the next ``step``."""
        if forces is None or energy is None:
            energy, forces = self.get_energy_and_forces()
        if self.handle is None:
            self._setup()
        f32 = forces.detach().to(torch.float32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_converge(self.handle, self.atom_offset.data_ptr(), f32.data_ptr(),
                                                   float(self.fmax), self._max_force.data_ptr(),
                                                   self._all_conv.data_ptr(), self._stream()))
        max_forces_ = self._max_force.clone()
        self.max_force_log.append(max_forces_)
        if logging.getLogger().isEnabledFor(logging.INFO):
            logging.info("%d %s", iteration, " ".join("%.3f" % v for v in max_forces_.tolist()))
        return max_forces_[self.atom_batch].ge(self.fmax), energy, f32

    def _all_converged(self) -> bool:
        self._all_conv_host.copy_(self._all_conv, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return bool(int(self._all_conv_host[0]))

    def run(self, fmax, steps):
        self.fmax = fmax
        self.steps = steps
        self._setup()
        self.max_force_log = []
        self.frames = None
        if self.traj_dir:
            self.traj_dir.mkdir(exist_ok=True, parents=True)
            self.frames = [[] for _ in range(self.num_systems)]

        # every iteration checks convergence; the trajectory gets the first, the last and (save_full_traj) every
        # unconverged iteration; no step after convergence or on the last iteration
        self.iterations = 0
        try:
            for it in range(steps):
                mask, energy, forces = self.check_convergence(it)
                self.iterations = it + 1
                done = self._all_converged()
                last = it + 1 == steps
                if self.frames is not None and (self.save_full or done or last or it == 0):
                    self.write(energy, forces, mask)
                if done:
                    break
                if not last:
                    self.step(it, forces, mask)
        finally:
            self.close()
        if self.frames is not None:
            self._write_files()
        self.batch.y, self.batch.force = self.get_energy_and_forces(apply_constraint=False)
        return self.batch

    def step(self, iteration: int, forces: Optional[torch.Tensor], update_mask: Optional[torch.Tensor] = None) -> None:
        """Reference :134-189 (``adf_lbfgs_step``).  The update mask is the one of the last ``check_convergence`` (kept on
        the device); ``update_mask`` is accepted for the reference's signature."""
        if forces is None:
            _, forces = self.get_energy_and_forces()
        if self.handle is None:
            raise RuntimeError("LBFGS.step: call check_convergence first (it sets the update mask)")
        f32 = forces.detach().to(torch.float32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_step(self.handle, self.atom_offset.data_ptr(), self.batch.pos.data_ptr(),
                                               f32.data_ptr(), int(iteration), self._stream()))

    def last_step_max(self) -> torch.Tensor:
        """max |dr| over the batch of the last step, device f64 scalar (below 1e-7: the step was skipped); per-system mode:
        over the systems that attempted a step."""
        out = torch.empty((), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_last_step_max(self.handle, out.data_ptr(), self._stream()))
        return out

    def set_per_system(self, on: bool) -> None:
        """Switch the handle's mode (``adf_lbfgs_set_per_system``); ValueError after a step or with early_stop_batch."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_set_per_system(self.handle, 1 if on else 0))
        self.per_system = bool(on)

    def step_state(self):
        """Per-system mode: (steps_taken int32 [B], last_absmax f64 [B]) on the device - the steps every system has
        attempted and the largest |dr| of its last attempt (below 1e-7: skipped; -1: its mask was clear in the last step)."""
        steps = torch.empty(self.num_systems, dtype=torch.int32, device=self.device)
        absmax = torch.empty(self.num_systems, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_get_step_state(self.handle, steps.data_ptr(), absmax.data_ptr(), self._stream()))
        return steps, absmax

    def reset(self) -> None:
        """Forget the history (``adf_lbfgs_reset``): the next step must have iteration 0."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_reset(self.handle, self._stream()))

    def update_mask(self) -> torch.Tensor:
        """The per-system update mask of the last check_convergence, int32 [B] on the device (``adf_lbfgs_get_mask``)."""
        out = torch.empty(self.num_systems, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_lbfgs_get_mask(self.handle, out.data_ptr(), self._stream()))
        return out

    # ------------------------------------------------------------------ trajectories
    def write(self, energy, forces, update_mask) -> None:
        """Reference :204-212: a frame per system whose mask is set, or every system without ``save_full_traj``."""
        self.batch.y, self.batch.force = energy, forces
        offs = self.atom_offset.tolist()
        pos = self.batch.pos.detach().cpu().numpy()
        e = energy.detach().to(torch.float64).cpu().numpy().reshape(-1)
        f = forces.detach().to(torch.float64).cpu().numpy()
        m = update_mask.detach().cpu().numpy()
        for b in range(self.num_systems):
            a0, a1 = offs[b], offs[b + 1]
            if (a1 > a0 and m[a0]) or not self.save_full:
                self.frames[b].append((pos[a0:a1].copy(), float(e[b]), f[a0:a1].copy()))

    def _write_files(self) -> None:
        b = self.batch
        offs = self.atom_offset.tolist()
        numbers = b.atomic_numbers.detach().cpu().numpy()
        tags = b.tags.detach().cpu().numpy() if hasattr(b, "tags") and b.tags is not None else np.zeros(len(numbers), np.int64)
        fixed = b.fixed.detach().cpu().numpy() if hasattr(b, "fixed") and b.fixed is not None else np.zeros(len(numbers), np.int64)
        cell = b.cell.detach().cpu().numpy().reshape(-1, 3, 3)
        for i, name in enumerate(self.traj_names):
            a0, a1 = offs[i], offs[i + 1]
            fr = self.frames[i]
            n = a1 - a0
            tmp = self.traj_dir / f"{name}.npz_tmp"
            with open(tmp, "wb") as fh:
                np.savez(fh,
                         positions=np.stack([p for p, _, _ in fr]) if fr else np.zeros((0, n, 3), np.float32),
                         energy=np.asarray([e for _, e, _ in fr], np.float64),
                         forces=np.stack([f for _, _, f in fr]) if fr else np.zeros((0, n, 3), np.float64),
                         numbers=numbers[a0:a1], tags=tags[a0:a1], fixed=fixed[a0:a1], cell=cell[i])
            tmp.rename(self.traj_dir / f"{name}.npz")


class TorchCalc:
    def __init__(self, model, transform=None) -> None:
        self.model = model
        self.transform = transform

    def get_energy_and_forces(self, atoms, apply_constraint: bool = True):
        """(energy [B], forces [N,3]) from the trainer's ``predict``; with ``apply_constraint`` the rows of fixed atoms are
        zeroed in place (reference :219-228), by a masked fill on the device (no host read of the fixed-atom indices)."""
        out = self.model.predict(atoms, per_image=False, disable_tqdm=True)
        if apply_constraint:
            out["forces"].masked_fill_((atoms.fixed == 1).reshape(-1, 1), 0)
        return out["energy"], out["forces"]

    def update_graph(self, atoms):
        raise NotImplementedError("precomputed graphs (otf_graph=False) are not offered on the HIP path")
