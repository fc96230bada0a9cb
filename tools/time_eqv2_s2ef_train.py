"""Timing of one training step of the EquiformerV2 S2EF force field at the shipped width
(tests/helpers_s2ef.FULL_KW: lmax 4, mmax 2, 128 sphere channels, 8 blocks, 8 heads, 128 edge channels, K = 20, cutoff 12) on
12 systems of the synthetic 200-atom slabs.  A record, not a gate.  Prints one JSON line:

  train_step_ms      zero_grad + loss_and_grad of ``EqV2S2EFTrainStep`` (forward, loss, backward; no optimizer): median, min,
                     max of --reps runs after a warm-up, each between two device synchronisations
  forward_ms         the inference forward (``model(batch)``: the handle's fused f16x3 path) of the same batch in the same
                     process, alternating with the training step run by run
  ratio              median train_step_ms / median forward_ms
  graphs_per_s       systems / median train_step_ms
  peak_memory_mib    torch's peak allocation over the training steps (the handle's own workspaces are not in this figure)
  first_layers       on the same edges, the Gaussian part of the 1 + num_layers + 1 first radial layers, forward and weight
                     gradient: ``window_ms`` through adf_op_eq_radial_gauss_fwd / _bwd (the sorted permutation formed once,
                     as in a step), ``dense_ms`` through the route the denoiser's step takes and this model's would have
                     taken (adf_op_eq_edge_scalars + adf_op_eq_linear_fwd, and again + adf_op_eq_linear_bwd, K = 600 +
                     2 EC), run by run in alternation; ``dense_over_window`` = the ratio of the medians

The child process runs under its own time limit; a child that fails ends the tool.

    python tools/time_eqv2_s2ef_train.py [--systems 12] [--atoms 200] [--reps 7] [--layers 8]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEV = "cuda:0"


def _spread(xs, nd=2):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], nd), "min": round(xs[0], nd), "max": round(xs[-1], nd)}


def child(a) -> dict:
    import torch

    from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20
    from adsorbdiff_amd.eqv2_train_step import EqGraph, EqOps, EqV2S2EFTrainStep
    from adsorbdiff_amd.synthetic import make_batch
    from tests.helpers_s2ef import FULL_KW

    torch.manual_seed(0)
    model = EquiformerV2_OC20(None, None, None, **dict(FULL_KW, num_layers=a.layers)).to(DEV)
    batch = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000)
    z = batch.atomic_numbers.clone()
    z[z >= int(model.max_num_elements)] = 47.0
    batch.atomic_numbers = z
    g = torch.Generator().manual_seed(5)
    B, N = a.systems, int(batch.pos.shape[0])
    batch.energy = torch.randn(B, generator=g)
    batch.forces = torch.randn(N, 3, generator=g)
    batch = batch.to(DEV)
    step = EqV2S2EFTrainStep(model, DEV, normalizers={"energy": {"mean": -0.7, "stdev": 1.9}, "forces": {"mean": 0.0, "stdev": 2.1}},
                             force_coefficient=100)
    train_ms, fwd_ms = [], []
    for rnd in range(a.reps + 1):
        model.train()
        torch.cuda.synchronize()
        if rnd == 1:
            torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        step.zero_grad()
        loss = step.loss_and_grad(batch)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        model.eval()
        with torch.no_grad():
            model(batch)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rnd:
            train_ms.append((t1 - t0) * 1e3)
            fwd_ms.append((t2 - t1) * 1e3)
    if not bool(torch.isfinite(loss).all()):
        raise SystemExit("non-finite loss")
    peak = round(torch.cuda.max_memory_allocated() / 2**20, 1)

    # ---- operator level: the Gaussian part of the first layers, both routes, on the step's own edges
    eng = model.engine(DEV, refresh=False)
    ops = EqOps(eng)
    gr = EqGraph(eng, batch, eng.prepare(batch))
    E, EC, NB = gr.E, ops.EC, ops.NB
    IN = NB + 2 * EC
    nrad = a.layers + 2
    mod = model.edge_degree_embedding
    W0 = mod.rad_func.net[0].weight.detach()
    b0 = mod.rad_func.net[0].bias.detach()
    semb, temb = mod.source_embedding.weight.detach(), mod.target_embedding.weight.detach()
    dh0 = torch.randn(E, EC, device=DEV)
    h0, dW0 = torch.zeros(E, EC, device=DEV), torch.zeros(EC, IN, device=DEV)
    ops.edge_distances(gr)

    def window():
        for _ in range(nrad):
            ops.gauss_fwd(gr, W0, h0)
            ops.gauss_bwd(gr, dh0, dW0)

    def dense():
        for _ in range(nrad):
            scal = ops.edge_scalars(gr, semb, temb)
            ops.linear(scal, W0, b0, h0, E, EC, IN)
            scal = ops.edge_scalars(gr, semb, temb)
            ops.linear_bwd(scal, W0, dh0, E, EC, IN, dW=dW0)

    win_ms, den_ms = [], []
    for rnd in range(a.reps + 1):
        for fn, acc in ((window, win_ms), (dense, den_ms)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                acc.append((time.perf_counter() - t0) * 1e3)
    tm, fm, wm, dm = _spread(train_ms), _spread(fwd_ms), _spread(win_ms), _spread(den_ms)
    return {"atoms_total": N, "edges": E, "train_step_ms": tm, "forward_ms": fm, "ratio": round(tm["median"] / fm["median"], 2),
            "graphs_per_s": round(B / tm["median"] * 1e3, 2), "peak_memory_mib": peak,
            "first_layers": {"radial_functions": nrad, "window_ms": wm, "dense_ms": dm,
                             "dense_over_window": round(dm["median"] / wm["median"], 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=12)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--limit", type=int, default=400, help="seconds granted to the child")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a)), flush=True)
        return
    res = {"systems": a.systems, "atoms": a.atoms, "layers": a.layers, "reps": a.reps}
    cmd = [sys.executable, __file__, "--child", "--systems", str(a.systems), "--atoms", str(a.atoms), "--reps", str(a.reps),
           "--layers", str(a.layers)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    if p.returncode != 0:
        raise SystemExit(f"child: exit status {p.returncode}\n{p.stderr[-3000:]}")
    res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
