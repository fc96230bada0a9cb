"""TEST INFRASTRUCTURE - generate tests/golden/scale_fit.npz by running the REAL reference's scale-factor fit on CPU: its
``ScaleFactor`` modules (adsorbdiff/modules/scaling/scale_factor.py) inside its two PaiNN classes, driven by the loop of
modules/scaling/fit.py:157-224 (restated in ``ref_fit`` below without the trainer, the prompts and the checkpoint handling:
``model.eval()``, factors reset in mode "all", one pass with ``index_fn`` for the computation order, then one factor at a
time over ``islice(batches, num_batches)`` inside its ``fit_context_`` and ``fit_()``).  Run in the build container only
(needs the reference sources on the import path, as tools/make_golden_relax.py does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_scale_fit.py

Models and batches are those of tests/helpers_scale_fit.py: H = 128, three layers, 32 radial functions, cutoff 6 A, weights
drawn from a seed and rescaled to trained-like magnitudes (NOT stored: the mirror classes draw the same, checked here and
again in the tests by per-tensor sums); three ragged batches of 9- to 40-atom systems, one of them a single system.  For
each model ("denoiser": painn_denoising.PaiNN with two heads; "s2ef": painn.PaiNN) the file holds, per factor in layer
order:

    <m>_seq32_*   variance_out / n_samples / ratio / value of the sequential fit in float32 (what fit.py computes)
    <m>_seq64_*   the same loop with the model in float64 on the float32 graph of each batch (the tests' reference)
    <m>_unf64_*   mode "unfitted" with factor 1 preset to PRESET (value of factor 1 = PRESET, untouched)
    <m>_single64_value   one pass observing all factors at once (not what fit.py does; asserted to differ by > 1e-3)
    <m>_obs_scales, <m>_obs_var32 / _obs_var64 [batch, layer]   per-layer statistics of each batch with the float32-rounded
                  seq64 values in force
    <m>_sums      per-tensor sums of the weights

and for the host tests (plain torch, tests/helpers_scale_fit.py::StandIn and standin_batches):

    proto_*       one reference ScaleFactor observing the stand-in tensors directly: variance_out, n_samples, ratio, value
    standin_*     the loop on StandIn built around the reference's ScaleFactor: mode "all", and "unfitted" with scale_1 preset
"""
from __future__ import annotations

import math
import sys
from itertools import islice
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from tools.make_golden_relax import GOLD, write_npz  # noqa: E402

NUM_BATCHES = 16


def ref_fit(model, factors, batches, mode, run, num_batches=NUM_BATCHES):
    """fit.py:157-224 on ``factors`` (name -> the reference's ScaleFactor) of ``model``; ``run(batch)`` is its _train_batch."""
    model.eval()
    if mode == "all":
        for f in factors.values():
            f.reset_()
    order = {}
    for name, f in factors.items():
        def index_fn(name=name):
            order.setdefault(name, len(order))

        f.initialize_(index_fn=index_fn)
    run(next(iter(batches)))
    for f in factors.values():
        f.initialize_(index_fn=None)
    out = {}
    for name, f in sorted(factors.items(), key=lambda kv: order.get(kv[0], math.inf)):
        if mode == "unfitted" and f.fitted:
            out[name] = dict(variance_out=math.nan, n_samples=0, ratio=math.nan, value=float(f.scale_factor.item()))
            continue
        with f.fit_context_():
            for batch in islice(batches, num_batches):
                run(batch)
            stats, ratio, value = f.fit_()
        out[name] = dict(variance_out=stats["variance_out"], n_samples=stats["n_samples"], ratio=ratio, value=value)
    assert all(f.fitted for f in factors.values())
    return [out[n] for n in sorted(out, key=lambda n: order[n])]


def single_pass(model, factors, batches, run):
    """All factors observed in ONE pass over the batches, every one still the identity: not the reference's protocol."""
    from contextlib import ExitStack

    for f in factors.values():
        f.reset_()
    with ExitStack() as st:
        for f in factors.values():
            st.enter_context(f.fit_context_())
        for batch in batches:
            run(batch)
        return [f.fit_()[2] for f in factors.values()]


def observe_layers(factors, batch, run):
    """mean(var(x)) after every factor for one batch, with the factors as they are."""
    from contextlib import ExitStack

    with ExitStack() as st:
        for f in factors.values():
            st.enter_context(f.fit_context_())
        run(batch)
        return [f.stats["variance_out"] / f.stats["n_samples"] for f in factors.values()]


def pack(prefix, rows):
    return {f"{prefix}_{k}": np.array([r[k] for r in rows], dtype=np.float64) for k in ("variance_out", "n_samples", "ratio", "value")}


def main() -> None:
    from oracle import refshim

    refshim.install()
    from adsorbdiff.models.painn.painn import PaiNN as RefS2EF
    from adsorbdiff.models.painn.painn_denoising import PaiNN as RefDenoiser
    from adsorbdiff.modules.scaling import ScaleFactor as RefScaleFactor
    from adsorbdiff.utils.utils import radius_graph_pbc

    from oracle import painn_oracle
    from tests import helpers_scale_fit as S

    torch.set_num_threads(8)
    batches = S.make_batches()
    for b in batches:
        print("batch", b.natoms.tolist())
    assert all(9 <= int(n) <= 40 for b in batches for n in b.natoms) and any(len(b.natoms) == 1 for b in batches)
    for b in batches:   # no exact tie at the K-th neighbour: the reference's graph is the lowest-candidate-index one (the oracle's)
        ei, co, _ = radius_graph_pbc(b.clone(), S.HP["cutoff"], S.HP["max_neighbors"], True)
        oe = painn_oracle.radius_graph_pbc(b.pos, b.cell.reshape(-1, 3, 3), b.natoms, S.HP["cutoff"], S.HP["max_neighbors"])
        rows = lambda e, c: sorted(map(tuple, torch.cat([e.t(), c.long()], 1).tolist()))
        assert rows(ei, co) == rows(oe[0], oe[1]), "a batch has an exact neighbour tie: pick another BATCH_SEED"
    fx = {}

    def run32(model):
        def run(batch):
            with torch.no_grad():
                model(batch.clone())
        return run

    def run64(model):
        """float64 model on the float32 graph of the batch (the reference's own radius_graph_pbc), passed in"""
        graphs = {}

        def run(batch):
            key = id(batch)
            if key not in graphs:
                dd = torch.get_default_dtype()
                torch.set_default_dtype(torch.float32)
                graphs[key] = radius_graph_pbc(batch.clone(), S.HP["cutoff"], S.HP["max_neighbors"], True)
                torch.set_default_dtype(dd)
            ei, co, nb = graphs[key]
            b = batch.clone()
            b.edge_index, b.cell_offsets, b.neighbors = ei, co.to(torch.float64), nb
            b.pos, b.cell = b.pos.double(), b.cell.double()
            with torch.no_grad():
                model(b)
        return run

    for kind, cls in (("denoiser", RefDenoiser), ("s2ef", RefS2EF)):
        ref = S.build_model(kind, cls)
        mir = S.build_model(kind)
        sd_r, sd_m = ref.state_dict(), mir.state_dict()
        assert all(torch.equal(sd_r[k], sd_m[k]) for k in sd_r if k != "atom_radii"), "the mirror draws other weights"
        factors = {n: getattr(ref, n) for n in S.NAMES}
        assert all(isinstance(f, RefScaleFactor) for f in factors.values())
        fx[f"{kind}_sums"] = S.weight_sums(ref).numpy()

        seq32 = ref_fit(ref, factors, batches, "all", run32(ref))
        torch.set_default_dtype(torch.float64)
        ref.double()
        ref.otf_graph = False
        try:
            r64 = run64(ref)
            seq64 = ref_fit(ref, factors, batches, "all", r64)
            for f in factors.values():
                f.reset_()
            factors[S.NAMES[1]].set_(S.PRESET)
            unf64 = ref_fit(ref, factors, batches, "unfitted", r64)
            assert unf64[1]["value"] == S.PRESET
            single64 = single_pass(ref, factors, batches, r64)
            scales = np.array([r["value"] for r in seq64], dtype=np.float32)
            for f in factors.values():
                f.reset_()
            for f, v in zip(factors.values(), scales):
                f.set_(float(v))
            var64 = [observe_layers(factors, b, r64) for b in batches]
        finally:
            ref.float()
            ref.otf_graph = True
            torch.set_default_dtype(torch.float32)
        for f in factors.values():
            f.reset_()
        for f, v in zip(factors.values(), scales):
            f.set_(float(v))
        var32 = [observe_layers(factors, b, run32(ref)) for b in batches]

        v32 = np.array([r["value"] for r in seq32])
        v64 = np.array([r["value"] for r in seq64])
        s64 = np.array(single64)
        print(f"[{kind}] sequential f64 {v64}  f32-vs-f64 {np.abs(v32 / v64 - 1).max():.2e}")
        print(f"[{kind}] single-pass f64 {s64}  rel to sequential {np.abs(s64 / v64 - 1)}")
        print(f"[{kind}] unfitted (factor 1 = {S.PRESET}) {[r['value'] for r in unf64]}")
        assert np.abs(s64 / v64 - 1).max() > 1e-3, "sequential and single-pass fits agree: pick other weights"
        assert np.abs(v64 - 1).min() > 1e-3, "a factor stayed at 1: pick other weights"
        assert np.abs(v32 / v64 - 1).max() < 1e-5
        fx.update(pack(f"{kind}_seq32", seq32))
        fx.update(pack(f"{kind}_seq64", seq64))
        fx.update(pack(f"{kind}_unf64", unf64))
        fx[f"{kind}_single64_value"] = s64
        fx[f"{kind}_obs_scales"] = scales
        fx[f"{kind}_obs_var32"] = np.array(var32, dtype=np.float64)
        fx[f"{kind}_obs_var64"] = np.array(var64, dtype=np.float64)

    # ---- host tests: the protocol alone, and the loop on a plain torch module
    tensors = S.standin_batches()
    f = RefScaleFactor()
    with f.fit_context_():
        for t in tensors:
            f(t)
        acc = dict(f.stats)
        stats, ratio, value = f.fit_()
    fx.update(proto_acc_variance_out=acc["variance_out"], proto_acc_n_samples=acc["n_samples"],
              proto_variance_out=stats["variance_out"], proto_n_samples=stats["n_samples"], proto_ratio=ratio, proto_value=value)
    net = S.StandIn(scale_cls=RefScaleFactor)
    nf = {n: m for n, m in net.named_modules() if isinstance(m, RefScaleFactor)}

    def run_net(t):
        with torch.no_grad():
            net(t)

    fx.update(pack("standin_all", ref_fit(net, nf, tensors, "all", run_net)))
    for m in nf.values():
        m.reset_()
    nf["scale_1"].set_(S.PRESET)
    fx.update(pack("standin_unf", ref_fit(net, nf, tensors, "unfitted", run_net)))
    print("stand-in:", fx["standin_all_value"], fx["standin_unf_value"])
    write_npz(GOLD / "scale_fit.npz", fx)
    print("wrote", GOLD / "scale_fit.npz")


if __name__ == "__main__":
    main()
