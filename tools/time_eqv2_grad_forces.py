"""Timing of the energy-gradient forward of the EquiformerV2 S2EF force field at the shipped width
(tests/helpers_s2ef.FULL_KW: lmax 4, mmax 2, 128 sphere channels, 8 blocks, 8 heads, 128 edge channels, K = 20, cutoff 12) on
12 systems of the synthetic 200-atom slabs.  A record, not a gate.  Prints one JSON line:

  grad_forward_ms    ``model(batch)`` with ``force_mode = "energy_gradient"`` (forward, backward with respect to the edge
                     geometry, forces): median, min, max of --reps runs after a warm-up, each between two synchronisations
  forward_ms         the direct inference forward (``force_mode = "direct"``: the handle's fused f16x3 path) of the same batch
  train_step_ms      zero_grad + loss_and_grad of ``EqV2S2EFTrainStep`` on the same batch; the three alternate run by run in
                     one process
  peak_memory_mib    torch's peak allocation over the energy-gradient forwards / over the training steps (the handle's own
                     workspaces are in neither figure)
  geo_entries_ms     device time of the five entries of csrc/eqv2_geo.h inside one energy-gradient forward, each call between
                     two synchronisations (so their sum is an upper bound of their share), and ``geo_share`` = sum / median
  memory_per_system_mib, largest_batch_estimate
                     peak memory at --systems and at twice as many, the slope per system, and the number of 200-atom
                     systems that slope fits into the device's free memory: an extrapolation, not a run at that size

The child process runs under its own time limit; a child that fails ends the tool.

    python tools/time_eqv2_grad_forces.py [--systems 12] [--atoms 200] [--reps 5] [--layers 8]
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
GEO = ("adf_op_eq_rotate_in_bwd_wig", "adf_op_eq_rotate_out_bwd_wig", "adf_op_eq_radial_gauss_dgrad", "adf_op_eq_wigner_bwd",
       "adf_op_eq_edge_grad_to_atoms")


def _spread(xs, nd=2):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], nd), "min": round(xs[0], nd), "max": round(xs[-1], nd)}


def child(a) -> dict:
    import torch

    from adsorbdiff_amd import lib as _lib
    from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20
    from adsorbdiff_amd.eqv2_train_step import EqV2S2EFTrainStep
    from adsorbdiff_amd.synthetic import make_batch
    from tests.helpers_s2ef import FULL_KW

    def make(systems):
        batch = make_batch(systems, n_slab=a.atoms - 4, n_ads=4, seed=1000)
        z = batch.atomic_numbers.clone()
        z[z >= int(model.max_num_elements)] = 47.0
        batch.atomic_numbers = z
        g = torch.Generator().manual_seed(5)
        batch.energy = torch.randn(systems, generator=g)
        batch.forces = torch.randn(int(batch.pos.shape[0]), 3, generator=g)
        return batch.to(DEV)

    torch.manual_seed(0)
    model = EquiformerV2_OC20(None, None, None, **dict(FULL_KW, num_layers=a.layers)).to(DEV)
    batch = make(a.systems)
    B, N = a.systems, int(batch.pos.shape[0])
    step = EqV2S2EFTrainStep(model, DEV, normalizers={"energy": {"mean": -0.7, "stdev": 1.9}, "forces": {"mean": 0.0, "stdev": 2.1}},
                             force_coefficient=100)

    def grad_forward(b):
        model.eval()
        model.force_mode = "energy_gradient"
        try:
            return model(b)
        finally:
            model.force_mode = "direct"

    grad_ms, fwd_ms, train_ms = [], [], []
    peak_grad = peak_train = 0.0
    for rnd in range(a.reps + 1):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = grad_forward(batch)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        peak_grad = max(peak_grad, torch.cuda.max_memory_allocated() / 2**20)
        with torch.no_grad():
            model(batch)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        torch.cuda.reset_peak_memory_stats()
        model.train()
        step.zero_grad()
        step.loss_and_grad(batch)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        peak_train = max(peak_train, torch.cuda.max_memory_allocated() / 2**20)
        if rnd:
            grad_ms.append((t1 - t0) * 1e3)
            fwd_ms.append((t2 - t1) * 1e3)
            train_ms.append((t3 - t2) * 1e3)
    if not bool(torch.isfinite(out["forces"]).all()):
        raise SystemExit("non-finite forces")
    step.zero_grad()
    for p in model.parameters():
        p.grad = None

    # ---- the five new entries inside one energy-gradient forward, each call between two synchronisations
    lib = _lib.load()
    spent = {name: 0.0 for name in GEO}
    originals = {name: getattr(lib, name) for name in GEO}

    def timed(name, fn):
        def call(*args):
            torch.cuda.synchronize()
            t = time.perf_counter()
            st = fn(*args)
            torch.cuda.synchronize()
            spent[name] += (time.perf_counter() - t) * 1e3
            return st
        return call

    for name, fn in originals.items():
        setattr(lib, name, timed(name, fn))
    try:
        grad_forward(batch)
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)

    # ---- memory per system: the same forward on twice as many systems
    del out
    torch.cuda.empty_cache()
    big = make(2 * a.systems)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    grad_forward(big)
    torch.cuda.synchronize()
    peak_big = torch.cuda.max_memory_allocated() / 2**20
    per_system = (peak_big - peak_grad) / a.systems
    free, total = torch.cuda.mem_get_info()
    room = (free + torch.cuda.memory_reserved()) / 2**20
    gm, fm, tm = _spread(grad_ms), _spread(fwd_ms), _spread(train_ms)
    geo = {k: round(v, 2) for k, v in spent.items()}
    return {"atoms_total": N, "grad_forward_ms": gm, "forward_ms": fm, "train_step_ms": tm,
            "grad_over_forward": round(gm["median"] / fm["median"], 2), "grad_over_train": round(gm["median"] / tm["median"], 3),
            "peak_memory_mib": {"grad_forward": round(peak_grad, 1), "train_step": round(peak_train, 1),
                                f"grad_forward_{2 * a.systems}_systems": round(peak_big, 1)},
            "geo_entries_ms": geo, "geo_share": round(sum(spent.values()) / gm["median"], 3),
            "memory_per_system_mib": round(per_system, 1), "device_memory_mib": round(total / 2**20),
            "largest_batch_estimate": int((room - (peak_grad - per_system * a.systems)) / max(per_system, 1e-9))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=12)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
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
