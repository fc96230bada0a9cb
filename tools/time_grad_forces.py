"""Timing of forces as the gradient of the energy (PaiNN.force_mode = "energy_gradient", adf_painn_forward_energy_gradient)
at the OC20 PaiNN width (H=512, 6 layers, 128 rbf, cutoff 12, K=50; seeded weights).  Warm-up, then timed passes between
device synchronisations, the legs alternating in the same process.  Prints one JSON line:

  forward_ms            one direct S2EF forward (energy + force head, adf_painn_forward_energy incl. its flag check)
  gradient_ms           one gradient evaluation (energy + forces = -dE/dpos, incl. its flag check)
  ratio                 gradient_ms / forward_ms (a forward plus a data-gradient backward: expected around 2...3)
  train_step_ms         PaiNNTrainStep.loss_and_grad of the denoiser at the same width on the same batch: the same forward
                        and data gradients plus the weight gradients this path omits, minus its geometry product
  not_slower_than_train gradient_ms <= train_step_ms
  geo_ms, geo_tflops    the edge-geometry kernel (csrc/message_geo.hip), all layers of one evaluation: HIP events around its
                        launches (the handle's profiling, category "message") and its issued MFMA rate from the shapes, as
                        bench.py computes the message kernel's: contracted k length x 32-column blocks x 32 x 32 x 2 x 3 products
  workspace_gb          library-owned device memory of the gradient evaluation at this shape
  iterations_per_s      LBFGS.run iterations per second with gradient forces

One object per shape; the list is printed as one JSON line and written to --out.

    python tools/time_grad_forces.py [--shapes 1000x200,64x200] [--reps 5] [--no-train] [--out profiles/grad_forces.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc  # noqa: E402
from adsorbdiff_amd.painn import PaiNN  # noqa: E402
from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS  # noqa: E402
from adsorbdiff_amd.synthetic import make_batch  # noqa: E402
from adsorbdiff_amd.trainer import ForcesTrainer  # noqa: E402

DEV = "cuda:0"
HP = dict(hidden_channels=512, num_layers=6, num_rbf=128, cutoff=12.0, max_neighbors=50)
OPT = dict(maxstep=0.04, memory=50, damping=1.0, alpha=70.0)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def measure(systems, atoms, reps, run_steps, with_train):
    torch.manual_seed(0)
    model = PaiNN(None, 50, 1, scale_file=dict(PAINN_NB6_SCALE_FACTORS), **HP).to(DEV).eval()
    b = make_batch(systems, n_slab=atoms - 4, n_ads=4, seed=1000).to(DEV)
    N, B = int(b.pos.shape[0]), systems
    eng = model.engine(DEV)
    out = {"systems": B, "atoms": N, **HP}
    out["workspace_gb"] = eng.energy_gradient_workspace_bytes(N) / 1e9

    legs = {"forward_ms": lambda: eng.forward_energy(b), "gradient_ms": lambda: eng.forward_energy_gradient(b)}
    den = step = None
    if with_train:
        from adsorbdiff_amd.painn_denoising import PaiNN as Denoiser
        from adsorbdiff_amd.train_step import PaiNNTrainStep

        torch.manual_seed(0)
        den = Denoiser(None, 50, 1, so3_denoising=True, scale_file=dict(PAINN_NB6_SCALE_FACTORS), **HP).to(DEV)
        step = PaiNNTrainStep(den, DEV)
        g = torch.Generator().manual_seed(2)
        targets = dict(tr_sigma=torch.rand(B, 1, generator=g) + 0.5, rot_sigma=torch.rand(B, 1, generator=g) * 0.5 + 0.1,
                       tr_score=torch.randn(B, 3, generator=g), rot_score=torch.randn(B, 3, generator=g))
        step.zero_grad()
        legs["train_step_ms"] = lambda: step.loss_and_grad(b, targets)
    times = {k: [] for k in legs}
    for k, fn in legs.items():   # warm-up: engines, workspaces, weight images
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    for k, v in times.items():
        out[k] = median(v)
        out[k.replace("_ms", "_min_ms")] = min(v)
    out["ratio"] = out["gradient_ms"] / out["forward_ms"]
    if "train_step_ms" in out:
        out["not_slower_than_train"] = bool(out["gradient_ms"] <= out["train_step_ms"])
    del den, step

    # the geometry kernel alone: its launches are the only ones of a gradient evaluation under the "message" category
    E = eng.build_graph(b)
    out["edges"] = E
    eng.profile_enable(True)
    eng.profile_read()
    eng.forward_energy_gradient(b)
    prof = eng.profile_read()
    eng.profile_enable(False)
    geo_ms, launches = prof["message"]
    out["geo_ms"], out["geo_launches"] = geo_ms, launches
    out["geo_issued_tflop"] = prof["message_ksteps"] * 32 * 32 * 2.0 * 3 / 1e12
    out["geo_tflops"] = out["geo_issued_tflop"] / (geo_ms * 1e-3) if geo_ms > 0 else 0.0

    tr = ForcesTrainer(model, device=DEV)
    model.force_mode = "energy_gradient"
    b2 = make_batch(systems, n_slab=atoms - 4, n_ads=4, seed=1000).to(DEV)
    opt = LBFGS(b2, TorchCalc(tr), device=DEV, **OPT)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt.run(fmax=1e-9, steps=run_steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["run_iterations"] = opt.iterations
    out["iterations_per_s"] = opt.iterations / dt
    out["lbfgs_iteration_ms"] = 1e3 * dt / opt.iterations
    opt.close()
    eng.close()
    model._engine = None
    torch.cuda.empty_cache()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x200,64x200", help="systems x atoms per system, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=4)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    results = []
    for shape in a.shapes.split(","):
        systems, atoms = (int(t) for t in shape.split("x"))
        results.append(measure(systems, atoms, a.reps, a.run_steps, not a.no_train))
    line = json.dumps(results)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
