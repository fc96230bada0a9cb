"""Timing of one training step of the EquiformerV2 denoiser at the shipped shape
(configs/denoising/eqv2_conditional.yml: lmax 4, mmax 2, 128 sphere channels, 8 blocks, 8 heads, K = 20, cutoff 12,
conditional, alpha_drop = drop_path_rate = 0.1) on 12 systems (the YAML's batch size) of the synthetic 200-atom slabs.
A record, not a gate.  Prints one JSON line:

  train_step_ms      zero_grad + loss_and_grad of ``EqV2TrainStep`` (forward, loss, backward; no optimizer): median, min, max
                     of --reps runs after a warm-up, each between two device synchronisations
  forward_ms         the inference forward (``model(batch)``: the handle's fused f16x3 path) of the same batch in the same
                     process, alternating with the training step run by run
  ratio              median train_step_ms / median forward_ms
  graphs_per_s       systems / median train_step_ms
  peak_memory_mib    torch's peak allocation over the training steps (activations are kept per edge, no recomputation; the
                     handle's own workspaces are not torch's and are not in this figure)

The child process runs under its own time limit; a child that fails ends the tool.

    python tools/time_eqv2_train.py [--systems 12] [--atoms 200] [--reps 7] [--layers 8]
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

    from adsorbdiff_amd.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos
    from adsorbdiff_amd.eqv2_train_step import EqV2TrainStep
    from adsorbdiff_amd.so3_tables import Igso3Tables
    from adsorbdiff_amd.synthetic import make_batch

    torch.manual_seed(0)
    model = EquiformerV2S_OC20_DenoisingPos(
        None, None, None, max_neighbors=20, max_radius=12.0, max_num_elements=90, num_layers=a.layers, sphere_channels=128,
        attn_hidden_channels=64, num_heads=8, attn_alpha_channels=64, attn_value_channels=16, ffn_hidden_channels=128,
        norm_type="layer_norm_sh", lmax_list=[4], mmax_list=[2], grid_resolution=18, edge_channels=128, attn_activation="silu",
        ffn_activation="silu", use_grid_mlp=True, use_sep_s2_act=True, alpha_drop=0.1, drop_path_rate=0.1, weight_init="uniform",
        so3_denoising=True, FOR_denoising=True, energy_encoding="scalar").to(DEV)
    batch = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000)
    z = batch.atomic_numbers.clone()
    z[(z == 36) | (z == 54) | (z >= 85)] = 47.0   # elements without a tabulated radius
    batch.atomic_numbers = z
    g = torch.Generator().manual_seed(5)
    B = a.systems
    batch.energy = torch.randn(B, generator=g)
    tr_sigma = 0.1 * (10.0 / 0.1) ** torch.rand(B, 1, generator=g)
    rot_sigma = 0.01 * (1.55 / 0.01) ** torch.rand(B, 1, generator=g)
    targets = {"tr_sigma": tr_sigma, "rot_sigma": rot_sigma, "tr_score": torch.randn(B, 3, generator=g) / tr_sigma,
               "rot_score": torch.randn(B, 3, generator=g) / rot_sigma, "rot_norm": torch.ones(B)}
    batch = batch.to(DEV)
    step = EqV2TrainStep(model, DEV, igso3=Igso3Tables(None, None, None, None))
    train_ms, fwd_ms = [], []
    edges = None
    for rnd in range(a.reps + 1):
        model.train()
        torch.cuda.synchronize()
        if rnd == 1:
            torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        step.zero_grad()
        loss = step.loss_and_grad(batch, targets)
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
        if edges is None:
            edges = int(model.engine(DEV, refresh=False).export_graph(batch)[1].numel())
    if not bool(torch.isfinite(loss).all()):
        raise SystemExit("non-finite loss")
    tm, fm = _spread(train_ms), _spread(fwd_ms)
    return {"atoms_total": int(batch.pos.shape[0]), "edges": edges, "train_step_ms": tm, "forward_ms": fm,
            "ratio": round(tm["median"] / fm["median"], 2), "graphs_per_s": round(B / tm["median"] * 1e3, 2),
            "peak_memory_mib": round(torch.cuda.max_memory_allocated() / 2**20, 1)}


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
