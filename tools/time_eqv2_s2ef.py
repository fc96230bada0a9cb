"""Timing of the EquiformerV2 S2EF force field at the relaxation shape (default 64 systems x 200 atoms, config-4 width
with lmax_list=[4]: 8 blocks, C = 128, cutoff 12, K = 20; weights refilled by name).  Prints one JSON line per mode:

  --model s2ef       EquiformerV2_OC20: forward wall time (profile off), then with the HIP-event profile on the time of
                     the radial functions per forward, per radial function (10 of them) and as a share of the forward;
                     with --relax also LBFGS.run iterations (forward + convergence check + step, configs/relaxation
                     settings: maxstep 0.04, memory 50, damping 1.0, alpha 70) in ms per iteration
  --model denoiser   the denoiser mirror at the same width with ``atom_radii`` zeroed before the first forward, so that
                     its distance basis is live and weight binding picks the per-edge radial path by itself (11 radial
                     functions): the baseline the S2EF model's fused first radial layer is measured against
  --model denoiser-tabulated   the denoiser as shipped (radial functions tabulated per element pair): what live
                     distances cost on top

    python tools/time_eqv2_s2ef.py --model s2ef [--systems 64] [--atoms 200] [--reps 5] [--relax]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from adsorbdiff_amd.synthetic import make_batch  # noqa: E402
from tests.helpers import CFG4_KW, refill_parameters_by_name  # noqa: E402

DEV = "cuda:0"
OPT = dict(maxstep=0.04, memory=50, damping=1.0, alpha=70.0)


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("s2ef", "denoiser", "denoiser-tabulated"), default="s2ef")
    ap.add_argument("--systems", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--relax", action="store_true")
    ap.add_argument("--run-steps", type=int, default=6)
    a = ap.parse_args()
    torch.manual_seed(0)
    if a.model == "s2ef":
        from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20

        kw = {k: v for k, v in dict(CFG4_KW, lmax_list=[4]).items() if k != "FOR_denoising"}
        model = refill_parameters_by_name(EquiformerV2_OC20(None, None, None, **kw).eval(), 300.0)
        n_rad = 1 + kw["num_layers"] + 1
    else:
        from adsorbdiff_amd.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos

        kw = dict(CFG4_KW, lmax_list=[4])
        model = refill_parameters_by_name(EquiformerV2S_OC20_DenoisingPos(None, None, None, **kw).eval(), 300.0)
        if a.model == "denoiser":
            with torch.no_grad():
                model.atom_radii.zero_()
        n_rad = 1 + kw["num_layers"] + 2
    model = model.to(DEV)
    b = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000).to(DEV)
    out = {"model": a.model, "systems": a.systems, "atoms": int(b.pos.shape[0]), "radial_functions": n_rad}
    with torch.no_grad():
        for _ in range(2):
            model(b)   # engine, workspaces
        out["forward_ms"] = wall(lambda: model(b), a.reps)
        eng = model.engine()
        out["edges"] = int(eng.counters().num_edges)
        eng.profile_enable(True)
        for _ in range(a.reps):
            model(b)
        prof = eng.profile_read()
        eng.profile_enable(False)
    total = sum(ms for ms, _ in prof.values())
    out["profile_ms_per_forward"] = {k: round(ms / a.reps, 3) for k, (ms, _) in prof.items() if ms > 0}
    out["radial_ms_per_forward"] = prof["radial"][0] / a.reps
    out["radial_ms_per_function"] = prof["radial"][0] / a.reps / n_rad if a.model != "denoiser-tabulated" else None
    out["radial_share_of_profiled"] = prof["radial"][0] / total
    if a.relax and a.model == "s2ef":
        from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc
        from adsorbdiff_amd.trainer import ForcesTrainer

        tr = ForcesTrainer(model, device=DEV)
        b2 = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000).to(DEV)
        opt = LBFGS(b2, TorchCalc(tr), device=DEV, **OPT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.run(fmax=1e-9, steps=a.run_steps)   # fmax tiny: no system converges
        torch.cuda.synchronize()
        # run() ends with one more forward (the unconstrained forces of the final positions)
        out["run_iterations"] = opt.iterations
        out["ms_per_iteration"] = (time.perf_counter() - t0) * 1e3 / (opt.iterations + 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
