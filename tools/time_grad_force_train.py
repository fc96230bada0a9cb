"""Time a training step on energy-gradient forces (PaiNNGradForceTrainStep) against the direct-force step in
the same process, and write profiles/grad_force_train.json.

    python tools/time_grad_force_train.py                  # 256 x 200 atoms, H = 512, 6 layers, K = 50
    python tools/time_grad_force_train.py --systems 64     # a smaller batch

Medians of ``--passes`` alternating passes (gradient-force step, direct step, one forward_energy_gradient), each timed with
device events around ``--steps`` calls after one warm-up call; the peak device memory of each; and, in a further pass of the
gradient-force step, the share of the two dual message kernels and of the stacked products (events around every call of
``adf_op_message_dual_fwd`` / ``_bwd`` and of the step's ``_lin2`` / ``_lin2_bwd``)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from adsorbdiff_amd.painn import PaiNN  # noqa: E402
from adsorbdiff_amd.synthetic import make_batch  # noqa: E402
from adsorbdiff_amd.train_step import PaiNNGradForceTrainStep, PaiNNS2EFTrainStep  # noqa: E402


def timed(fn, steps):
    fn()   # warm-up: workspaces, scratch, weight images
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, torch.cuda.max_memory_allocated() / 2**20


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--neighbors", type=int, default=50)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grad_force_train.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(3)
    model = PaiNN(None, 50, 1, hidden_channels=args.hidden, num_layers=args.layers, num_rbf=128, cutoff=12.0,
                  max_neighbors=args.neighbors).to(dev)
    batch = make_batch(args.systems, n_slab=args.atoms - 4, n_ads=4, seed=1000)
    g = torch.Generator().manual_seed(4)
    B, N = int(batch.natoms.numel()), int(batch.pos.shape[0])
    batch.energy, batch.forces = torch.randn(B, generator=g), torch.randn(N, 3, generator=g)
    batch = batch.to(dev)

    model.force_mode = "direct"
    direct = PaiNNS2EFTrainStep(model, dev, force_coefficient=100)
    model.force_mode = "energy_gradient"
    grad = PaiNNGradForceTrainStep(model, dev, force_coefficient=100)

    def run_grad():
        grad.zero_grad()
        grad.loss_and_grad(batch)

    def run_direct():
        direct.zero_grad()
        direct.loss_and_grad(batch)

    def run_forward():
        model.engine(dev, refresh=False).forward_energy_gradient(batch)

    rows = {"grad_force_step": [], "direct_step": [], "forward_energy_gradient": []}
    peaks = {k: 0.0 for k in rows}
    for _ in range(args.passes):
        for key, fn in (("grad_force_step", run_grad), ("direct_step", run_direct), ("forward_energy_gradient", run_forward)):
            ms, peak = timed(fn, args.steps)
            rows[key].append(ms)
            peaks[key] = max(peaks[key], peak)

    # shares: events around the message kernels and the stacked products of one more gradient-force step
    spans = {"message_dual": [], "stacked_products": []}

    def wrap(fn, key):
        def inner(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            spans[key].append((e0, e1))
            return out
        return inner

    class LibProxy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            return wrap(fn, "message_dual") if name in ("adf_op_message_dual_fwd", "adf_op_message_dual_bwd") else fn

    grad.lib = LibProxy(grad.lib)
    grad._lin2, grad._lin2_bwd = wrap(grad._lin2, "stacked_products"), wrap(grad._lin2_bwd, "stacked_products")
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    run_grad()
    t1.record()
    torch.cuda.synchronize()
    total = t0.elapsed_time(t1)
    shares = {k: sum(a.elapsed_time(b) for a, b in v) / total for k, v in spans.items()}

    med = {k: statistics.median(v) for k, v in rows.items()}
    result = {
        "config": {k: getattr(args, k) for k in ("systems", "atoms", "hidden", "layers", "neighbors", "steps", "passes")},
        "atoms_total": N, "edges": int(model.engine(dev, refresh=False).build_graph(batch)),
        "ms": med, "ms_all_passes": rows, "peak_mib": peaks,
        "ratio_grad_force_to_direct": med["grad_force_step"] / med["direct_step"],
        "share_of_grad_force_step": shares,
    }
    print(json.dumps(result))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
