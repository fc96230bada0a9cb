"""Evaluation metrics on the device — the reference's ``Evaluator`` (adsorbdiff/modules/evaluator.py) for device tensors.

The reference reads one number per metric and batch back to the host, walks the systems of a batch in Python for
``energy_forces_within_threshold`` and takes every system to numpy for ``average_distance_within_threshold``.  Here a
task's metrics are one or two kernel launches (csrc/evaluate.hip) that ADD into a ``DeviceMetrics`` accumulator, so a whole
validation pass reads the device once, at its end.

``Evaluator(task).eval(prediction, target, prev_metrics)`` keeps the reference's interface (dicts of tensors in, a dict
``{name: {"metric", "total", "numel"}}`` out, chained through ``prev_metrics``) at one host read per call; the trainers'
``validate`` drive the accumulator directly.  Only the default metric sets are offered.  There is no host fallback: the
tensors must be on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import lib as _lib

# slot of each metric name in the accumulator: the ADF_EVAL_* enum of include/adsorbdiff_hip.h
SLOTS = {
    "energy_mae": 0,
    "forcesx_mae": 1,
    "forcesy_mae": 2,
    "forcesz_mae": 3,
    "forces_mae": 4,
    "forces_cosine_similarity": 5,
    "forces_magnitude_error": 6,
    "energy_forces_within_threshold": 7,
    "positions_average_distance_within_threshold": 8,
    "positions_mae": 9,
    "positions_mse": 10,
    "energy_mse": 11,
    "energy_within_threshold": 12,
    "loss": 13,
}
NUM_SLOTS = 14
# metrics whose total is a count
COUNTING = ("energy_forces_within_threshold", "positions_average_distance_within_threshold", "energy_within_threshold")


def metric_name(target_property: str, fn: str) -> str:
    """The key a metric function's result is stored under (Evaluator.eval): the property is prefixed unless the function's
    name already carries it."""
    return fn if target_property in fn or target_property == "misc" else f"{target_property}_{fn}"


def distance_thresholds() -> np.ndarray:
    """The table of ``average_distance_within_threshold``, built as the reference builds it (its entries are arange's, not
    0.01 + k * 0.001 rounded)."""
    return np.arange(0.01, 0.5, 0.001)


class DeviceMetrics:
    """The accumulator pair of csrc/evaluate.hip on ``device``: ``total`` float64 [NUM_SLOTS], ``numel`` int64 [NUM_SLOTS]."""

    def __init__(self, device) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"DeviceMetrics needs a ROCm device, got {self.device} (no CPU fallback)")
        self.lib = _lib.load()
        self.total = torch.zeros(NUM_SLOTS, dtype=torch.float64, device=self.device)
        self.numel = torch.zeros(NUM_SLOTS, dtype=torch.int64, device=self.device)
        self._scratch = torch.empty(0, dtype=torch.float64, device=self.device)
        self._thresholds = None

    def zero(self) -> "DeviceMetrics":
        self.total.zero_()
        self.numel.zero_()
        return self

    # ------------------------------------------------------------------ plumbing
    def _s(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _scratch_for(self, B: int) -> torch.Tensor:
        n = int(self.lib.adf_eval_scratch(B))
        if self._scratch.numel() < n:
            self._scratch = torch.empty(n, dtype=torch.float64, device=self.device)
        return self._scratch

    def _f32(self, t: torch.Tensor, *shape) -> torch.Tensor:
        if not t.is_cuda:
            raise RuntimeError("the evaluation kernels take device tensors (no CPU fallback)")
        return t.detach().to(self.device, torch.float32).reshape(*shape).contiguous()

    def thresholds(self) -> torch.Tensor:
        if self._thresholds is None:
            self._thresholds = torch.from_numpy(distance_thresholds()).to(self.device)
        return self._thresholds

    # ------------------------------------------------------------------ the entries
    def add_s2ef(self, e_pred, f_pred, e_tgt, f_tgt, atom_offset, fixed=None, free_only: bool = True,
                 norm_energy=(0.0, 1.0), norm_forces=(0.0, 1.0)) -> None:
        """``adf_eval_s2ef``: normalised predictions ``e_pred [B]``, ``f_pred [N,3]`` (denormalised in the kernel with
        ``(mean, std)``), targets in target units, ``atom_offset [B+1]`` int32, ``fixed [N]`` int32 or None."""
        B = int(atom_offset.numel()) - 1
        N = int(f_pred.shape[0])
        e_pred, e_tgt = self._f32(e_pred, B), self._f32(e_tgt, B)
        f_pred, f_tgt = self._f32(f_pred, N, 3), self._f32(f_tgt, N, 3)
        if fixed is not None and (fixed.dtype != torch.int32 or int(fixed.numel()) != N):
            raise ValueError("fixed: an int32 tensor with one entry per atom")
        if atom_offset.dtype != torch.int32:
            raise ValueError("atom_offset: an int32 tensor [B + 1]")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eval_s2ef(
                e_pred.data_ptr(), f_pred.data_ptr(), e_tgt.data_ptr(), f_tgt.data_ptr(),
                fixed.data_ptr() if fixed is not None else None, atom_offset.data_ptr(), B, N, 1 if free_only else 0,
                C.c_float(norm_energy[0]), C.c_float(norm_energy[1]), C.c_float(norm_forces[0]), C.c_float(norm_forces[1]),
                self.total.data_ptr(), self.numel.data_ptr(), self._scratch_for(B).data_ptr(), self._s()))

    def add_is2rs(self, pos_pred, pos_tgt, cell, atom_offset, fixed=None) -> None:
        """``adf_eval_is2rs`` over the atoms with ``fixed == 0`` (None: all atoms)."""
        B = int(atom_offset.numel()) - 1
        N = int(pos_pred.shape[0])
        pos_pred, pos_tgt, cell = self._f32(pos_pred, N, 3), self._f32(pos_tgt, N, 3), self._f32(cell, B, 3, 3)
        if fixed is not None and (fixed.dtype != torch.int32 or int(fixed.numel()) != N):
            raise ValueError("fixed: an int32 tensor with one entry per atom")
        if atom_offset.dtype != torch.int32:
            raise ValueError("atom_offset: an int32 tensor [B + 1]")
        thr = self.thresholds()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eval_is2rs(
                pos_pred.data_ptr(), pos_tgt.data_ptr(), cell.data_ptr(), fixed.data_ptr() if fixed is not None else None,
                atom_offset.data_ptr(), B, N, thr.data_ptr(), int(thr.numel()), self.total.data_ptr(), self.numel.data_ptr(),
                self._scratch_for(B).data_ptr(), self._s()))

    def add_is2re(self, e_pred, e_tgt) -> None:
        B = int(e_pred.numel())
        e_pred, e_tgt = self._f32(e_pred, B), self._f32(e_tgt, B)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eval_is2re(e_pred.data_ptr(), e_tgt.data_ptr(), B, self.total.data_ptr(),
                                               self.numel.data_ptr(), self._s()))

    def add_value(self, name: str, value: torch.Tensor) -> None:
        """``Evaluator.update`` with a plain number: the first element of the device float tensor ``value`` is added to
        ``name``'s total and 1 to its numel."""
        value = self._f32(value, -1)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eval_add(value.data_ptr(), SLOTS[name], self.total.data_ptr(), self.numel.data_ptr(),
                                             self._s()))

    # ------------------------------------------------------------------ reading
    def all_reduce(self) -> "DeviceMetrics":
        """SUM of both tensors over the ranks (BaseTrainer.validate's aggregation); a no-op without a process group.
        Under gloo (several ranks on one GPU, the test configuration) it goes through the host, as ``train_step``'s flags."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
            return self
        for t in (self.total, self.numel):
            if dist.get_backend() == "gloo":
                host = t.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM)
                t.copy_(host)
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return self

    def result(self, names: Optional[Iterable[str]] = None) -> Dict[str, dict]:
        """``{name: {"metric", "total", "numel"}}`` of ``names`` (default: every slot that was written) with ONE
        device-to-host read; ``metric`` = total / numel (NaN for an empty slot)."""
        host = torch.cat([self.total, self.numel.to(torch.float64)]).cpu()   # (counts are exact in float64 below 2^53)
        total, numel = host[:NUM_SLOTS].tolist(), [int(v) for v in host[NUM_SLOTS:].tolist()]
        out = {}
        for name in (names if names is not None else [k for k, i in SLOTS.items() if numel[i] > 0]):
            i = SLOTS[name]
            t = int(total[i]) if name in COUNTING else total[i]
            out[name] = {"metric": t / numel[i] if numel[i] else float("nan"), "total": t, "numel": numel[i]}
        return out


def atom_offsets(natoms: torch.Tensor, device) -> torch.Tensor:
    off = torch.zeros(int(natoms.numel()) + 1, dtype=torch.int32, device=device)
    off[1:] = torch.cumsum(natoms.to(device).reshape(-1), 0).to(torch.int32)
    return off


class Evaluator:
    """``Evaluator(task)`` of the reference with its names and values; ``task`` in "s2ef", "is2rs", "is2re", "ocp".  The
    "ocp" task - the one the denoising trainer evaluates under - has a primary-metric entry (None) and NO metrics, so a
    validation under it reports ``loss`` alone.  A custom ``eval_metrics`` is refused by name."""

    task_metrics = {
        "s2ef": {
            "energy": ["mae"],
            "forces": ["forcesx_mae", "forcesy_mae", "forcesz_mae", "mae", "cosine_similarity", "magnitude_error",
                       "energy_forces_within_threshold"],
        },
        "is2rs": {"positions": ["average_distance_within_threshold", "mae", "mse"]},
        "is2re": {"energy": ["mae", "mse", "energy_within_threshold"]},
    }
    task_primary_metric = {
        "s2ef": "energy_forces_within_threshold",
        "is2rs": "average_distance_within_threshold",
        "is2re": "energy_mae",
        "ocp": None,
    }

    def __init__(self, task: Optional[str] = None, eval_metrics: Optional[dict] = None) -> None:
        default = self.task_metrics.get(task, {})
        if eval_metrics and eval_metrics != default:
            extra = sorted(metric_name(p, fn) for p, fns in eval_metrics.items() for fn in fns
                           if fn not in default.get(p, []))
            raise NotImplementedError(
                f"only the default metric set of a task is offered on the device; not offered: {', '.join(extra) or eval_metrics}")
        self.task = task
        self.target_metrics = default

    def metric_names(self):
        return [metric_name(p, fn) for p, fns in self.target_metrics.items() for fn in fns]

    def eval(self, prediction: Dict[str, torch.Tensor], target: Dict[str, torch.Tensor], prev_metrics: Optional[dict] = None):
        """The reference's call: ``prediction`` / ``target`` as ``_compute_metrics`` and ``run_relaxations`` build them
        (denormalised, already cut to the free atoms, ``natoms`` = atoms per system after the cut), on the device."""
        metrics = prev_metrics if prev_metrics is not None else {}
        if not self.target_metrics:
            return metrics
        if self.task == "s2ef":
            dev = prediction["forces"].device
            dm = DeviceMetrics(dev)
            dm.add_s2ef(prediction["energy"], prediction["forces"], target["energy"], target["forces"],
                        atom_offsets(target["natoms"], dev), fixed=None, free_only=False)
        elif self.task == "is2rs":
            if "pbc" in target and not all(bool(v) for v in torch.as_tensor(target["pbc"]).reshape(-1).tolist()):
                raise NotImplementedError("average_distance_within_threshold is offered for pbc = (True, True, True)")
            dev = prediction["positions"].device
            dm = DeviceMetrics(dev)
            dm.add_is2rs(prediction["positions"], target["positions"], target["cell"], atom_offsets(prediction["natoms"], dev))
        else:
            dm = DeviceMetrics(prediction["energy"].device)
            dm.add_is2re(prediction["energy"], target["energy"])
        # (the key of is2rs's primary metric is "positions_average_distance_within_threshold": the property is prefixed)
        for name, stat in dm.result(self.metric_names()).items():
            metrics = self.update(name, stat, metrics)
        return metrics

    def update(self, key, stat, metrics):
        """Adds ``stat`` (a {"total", "numel"} dict, or a plain number counted once) under ``key``."""
        entry = metrics.setdefault(key, {"metric": None, "total": 0, "numel": 0})
        if isinstance(stat, dict):
            entry["total"] += stat["total"]
            entry["numel"] += stat["numel"]
        elif isinstance(stat, (float, int)):
            entry["total"] += stat
            entry["numel"] += 1
        else:
            raise NotImplementedError(f"cannot add a {type(stat).__name__} to the metrics")
        entry["metric"] = entry["total"] / entry["numel"] if entry["numel"] else float("nan")
        return metrics
