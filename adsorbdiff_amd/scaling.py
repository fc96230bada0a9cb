"""ScaleFactor: forward-time scalar multiply, scale-file loader / writer and the fit.

Mirrors the reference's ``adsorbdiff.modules.scaling`` (scale_factor.py:29-172,
compat.py:52-77, fit.py:157-224): a 0-dim ``scale_factor`` parameter that multiplies
only when it has been fitted (value != 0), the observation protocol a fit drives
(``fit_context_`` / ``_observe`` / ``fit_``) and ``fit_scale_factors``, the loop of
fit.py without its prompts and its checkpoint-path handling:

* every factor is fitted alone, in computation order, over the first ``num_batches``
  batches, with the factors before it already in force and those after it still the
  identity (a factor changes the input of every later layer, so one pass for all of
  them gives other values);
* a batch of ``n`` rows adds ``mean_c(var_rows(x[:, c])) * n`` to ``variance_out`` and
  ``n`` to ``variance_in`` and ``n_samples`` (no ``ref=``); the fitted value is
  ``sqrt(1 / (variance_out / variance_in))``;
* a PaiNN of this package (``PaiNNHost``) is measured on the device: one
  ``PaiNNEngine.forward_observe(data, upto=l)`` per batch runs layers ``0..l`` and the
  float64 column-variance kernel (``csrc/scale_fit.hip``); any other ``nn.Module`` that
  holds ``ScaleFactor``s runs the reference's generic loop through the protocol.

A one-row batch has no variance (NaN in torch): here it raises ``ValueError`` naming
the batch.  Out of scope: fitting under DDP (the reference asserts against it) and the
consistency check of ``load_state_dict`` (``_enforce_consistency``).
"""
from __future__ import annotations

import json
import logging
import math
from contextlib import contextmanager
from itertools import islice
from pathlib import Path
from typing import Callable, Dict, Optional, Union

import torch
from torch import nn

IndexFn = Callable[[], None]


class NoVarianceError(ValueError):
    """A batch of fewer than two rows was observed: the unbiased variance over its rows does not exist."""


class ScaleFactor(nn.Module):
    scale_factor: torch.Tensor

    def __init__(self, name: Optional[str] = None) -> None:
        super().__init__()
        self.name = name
        self.index_fn: Optional[IndexFn] = None
        self.stats: Optional[Dict[str, float]] = None
        # a frozen 0-dim Parameter like the reference (scale_factor.py:47-49), so
        # parameter counts and checkpoint keys agree
        self.scale_factor = nn.Parameter(torch.tensor(0.0), requires_grad=False)

    @property
    def fitted(self) -> bool:
        return bool((self.scale_factor != 0.0).item())

    @torch.no_grad()
    def set_(self, scale: Union[float, torch.Tensor]) -> None:
        self.scale_factor.fill_(float(scale))

    @torch.no_grad()
    def reset_(self) -> None:
        self.scale_factor.zero_()

    def initialize_(self, *, index_fn: Optional[IndexFn] = None) -> None:
        """``index_fn`` is called at every forward (the fit uses it to learn the computation order); None removes it."""
        self.index_fn = index_fn

    @contextmanager
    def fit_context_(self):
        """Observe while inside: ``forward`` (or ``_observe``) accumulates into ``stats`` (scale_factor.py:106-112)."""
        self.stats = dict(variance_in=0.0, variance_out=0.0, n_samples=0)
        try:
            yield
        finally:
            self.stats = None

    def fit_(self):
        """-> (stats, ratio, value) and sets the factor (scale_factor.py:114-133); inside ``fit_context_`` only."""
        if not self.stats:
            raise ValueError("ScaleFactor.fit_: stats not set (call it inside fit_context_())")
        for k, v in self.stats.items():
            if not v > 0:
                raise ValueError(f"ScaleFactor.fit_: {k} is {v}")
        self.stats["variance_in"] = self.stats["variance_in"] / self.stats["n_samples"]
        self.stats["variance_out"] = self.stats["variance_out"] / self.stats["n_samples"]
        ratio = self.stats["variance_out"] / self.stats["variance_in"]
        value = math.sqrt(1 / ratio)
        self.set_(value)
        return dict(**self.stats), ratio, value

    def _add_observation(self, variance_out: float, n_samples: int, variance_in: Optional[float] = None) -> None:
        """One batch's statistic: ``variance_out`` (and ``variance_in``, 1 without a ``ref``) weighted by its rows."""
        self.stats["variance_out"] += variance_out * n_samples
        self.stats["variance_in"] += n_samples if variance_in is None else variance_in * n_samples
        self.stats["n_samples"] += n_samples

    @torch.no_grad()
    def _observe(self, x: torch.Tensor, ref: Optional[torch.Tensor] = None) -> None:
        if self.stats is None:
            return
        n_samples = x.shape[0]
        if n_samples < 2:
            raise NoVarianceError(f"ScaleFactor{'' if self.name is None else ' ' + repr(self.name)}: a batch of "
                                  f"{n_samples} row has no variance over its rows")
        self._add_observation(torch.mean(torch.var(x, dim=0)).item(), n_samples,
                              None if ref is None else torch.mean(torch.var(ref, dim=0)).item())

    def forward(self, x: torch.Tensor, *, ref: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.index_fn is not None:
            self.index_fn()
        if self.fitted:
            x = x * self.scale_factor
        if self.stats is not None:
            self._observe(x, ref=ref)
        return x


def _load_scale_dict(scale_file: Union[str, Path, Dict[str, float]]):
    if isinstance(scale_file, dict):
        return scale_file
    path = Path(scale_file)
    if not path.exists():
        raise ValueError(f"Scale file '{path}' does not exist.")
    if path.suffix == ".pt":
        scale_dict = torch.load(path, map_location="cpu")
    elif path.suffix == ".json":
        with open(path) as f:
            scale_dict = json.load(f)
        if isinstance(scale_dict, dict):
            scale_dict.pop("comment", None)
    else:
        raise ValueError(f"Unsupported scale file extension '{path.suffix}'")
    return scale_dict


def load_scales_compat(module: nn.Module, scale_file: Union[str, Path, Dict[str, float], None]) -> None:
    """Set every ``ScaleFactor`` sub-module named in ``scale_file`` (name -> value)."""
    if not scale_file:
        return
    scale_dict = _load_scale_dict(scale_file)
    if not scale_dict:
        logging.warning("No scale factors found in the scale file.")
        return
    factors = {name: m for name, m in module.named_modules() if isinstance(m, ScaleFactor)}
    for name, scale in scale_dict.items():
        if name not in factors:
            logging.warning(f"Scale factor '{name}' in the scale file has no matching module; ignored.")
            continue
        value = scale.item() if torch.is_tensor(scale) else float(scale)
        factors[name].set_(value)


def ensure_fitted(module: nn.Module, warn: bool = False) -> None:
    """Reference: adsorbdiff/modules/scaling/util.py:8-23."""
    unfitted = [name for name, m in module.named_modules() if isinstance(m, ScaleFactor) and not m.fitted]
    if unfitted:
        msg = "Unfitted scale factors: " + ", ".join(unfitted)
        if warn:
            logging.warning(msg)
        else:
            raise ValueError(msg)


# values of configs/scaling_factors/painn_nb6_scaling_factors.pt in the reference tree.
PAINN_NB6_SCALE_FACTORS = {
    "upd_out_scalar_scale_0": 1.0364354848861694,
    "upd_out_scalar_scale_1": 0.8951448202133179,
    "upd_out_scalar_scale_2": 0.8934778571128845,
    "upd_out_scalar_scale_3": 0.8899308443069458,
    "upd_out_scalar_scale_4": 0.8886106610298157,
    "upd_out_scalar_scale_5": 0.8822302222251892,
}


# ---------------------------------------------------------------------------------------------------------------- the fit
FIT_MODES = ("all", "unfitted")


def fitted_scale_dict(model: nn.Module) -> Dict[str, float]:
    """name -> value of every fitted ``ScaleFactor`` of ``model`` (what a scale file holds)."""
    return {name: float(m.scale_factor.item()) for name, m in model.named_modules()
            if isinstance(m, ScaleFactor) and m.fitted}


def save_scale_file(model: nn.Module, path: Union[str, Path]) -> Path:
    """Write the fitted factors of ``model`` as name -> float to a ``.pt`` or ``.json`` file that ``load_scales_compat``
    (and the reference's) reads back.  Unfitted factors raise: a scale file that names only some of them would leave the
    rest at the identity without a word."""
    ensure_fitted(model)
    path = Path(path)
    scales = fitted_scale_dict(model)
    if path.suffix == ".pt":
        torch.save(scales, path)
    elif path.suffix == ".json":
        with open(path, "w") as f:
            json.dump(scales, f, indent=2)
    else:
        raise ValueError(f"Unsupported scale file extension '{path.suffix}'")
    return path


def _fit_batches(batches, num_batches: int):
    """``islice(loader, num_batches)`` once per fitted factor, as fit.py:211; a one-shot iterator is read once and kept."""
    if iter(batches) is batches:
        batches = list(islice(batches, num_batches))
    return lambda: islice(batches, num_batches)


def _batch_label(i: int, batch) -> str:
    sid = getattr(batch, "sid", None)
    return f"batch {i}" + (f" (sid={sid})" if sid is not None else "")


def _result(stats: dict, ratio: float, value: float) -> dict:
    return dict(variance_in=stats["variance_in"], variance_out=stats["variance_out"], n_samples=stats["n_samples"],
                ratio=ratio, value=value)


def _fit_generic(model: nn.Module, factors: Dict[str, ScaleFactor], each_pass, mode: str, device) -> Dict[str, dict]:
    """fit.py:168-220 for any module: one pass to learn the order the factors are computed in, then one factor at a
    time."""
    def run(batch):
        with torch.no_grad():
            model(batch.to(device) if device is not None and hasattr(batch, "to") else batch)

    order: Dict[str, int] = {}
    for name, module in factors.items():
        def index_fn(name: str = name) -> None:
            order.setdefault(name, len(order))

        module.initialize_(index_fn=index_fn)
    try:
        first = next(iter(each_pass()), None)
        if first is None:
            raise ValueError("fit_scale_factors: no batches")
        run(first)
    finally:
        for module in factors.values():
            module.initialize_(index_fn=None)
    out = {}
    for name, module in sorted(factors.items(), key=lambda kv: order.get(kv[0], math.inf)):
        if mode == "unfitted" and module.fitted:
            continue
        with module.fit_context_():
            for i, batch in enumerate(each_pass()):
                try:
                    run(batch)
                except NoVarianceError as e:
                    raise NoVarianceError(f"fit_scale_factors: {_batch_label(i, batch)}: {e}") from None
            out[name] = _result(*module.fit_())
    return out


def _fit_painn(model, factors: Dict[str, ScaleFactor], each_pass, mode: str, device) -> Dict[str, dict]:
    """The same loop with the measurement on the device.  The factors are computed in layer order; factor l is observed by
    ``forward_observe(data, upto=l)``, which stops after layer l.  ``set_()`` changes the parameter, so the next
    ``model.engine()`` call sees another weights version and binds the new multipliers."""
    if device is None:
        device = model.atom_emb.embeddings.weight.device
    out = {}
    for l in range(model.num_layers):
        name = "upd_out_scalar_scale_%d" % l
        module = factors[name]
        if mode == "unfitted" and module.fitted:
            continue
        engine = model.engine(device)   # after the previous factor's set_(): re-bound once per factor, not per batch
        with module.fit_context_():
            for i, batch in enumerate(each_pass()):
                data = batch.to(device)
                n = int(data.pos.shape[0])
                if n < 2:
                    raise NoVarianceError(f"fit_scale_factors: {_batch_label(i, batch)} has {n} atom: no variance over the atoms")
                var = engine.forward_observe(data, upto=l)
                module._add_observation(float(var[l].item()), n)
            out[name] = _result(*module.fit_())
    return out


def fit_scale_factors(model: nn.Module, batches, num_batches: int = 16, mode: str = "all", device=None) -> Dict[str, dict]:
    """Fit the ``ScaleFactor``s of ``model`` (module docstring) on the first ``num_batches`` of ``batches`` (raw batches, the
    model's current weights, ``model.eval()`` for the duration).  ``mode``: ``"all"`` resets every factor first,
    ``"unfitted"`` leaves the fitted ones as they are and in force.  -> ``{name: {"variance_in", "variance_out",
    "n_samples", "ratio", "value"}}`` of the factors fitted here, in the order they were fitted."""
    if mode not in FIT_MODES:
        raise ValueError(f"fit_scale_factors: mode must be one of {FIT_MODES}, got {mode!r}")
    from .painn_denoising import PaiNNHost

    factors = {name: m for name, m in model.named_modules() if isinstance(m, ScaleFactor)}
    each_pass = _fit_batches(batches, int(num_batches))
    was_training = model.training
    model.eval()
    try:
        if mode == "all":
            for module in factors.values():
                module.reset_()
        fit = _fit_painn if isinstance(model, PaiNNHost) else _fit_generic
        out = fit(model, factors, each_pass, mode, device)
    finally:
        model.train(was_training)
    ensure_fitted(model)
    return out
