"""Timing of the sampler's early stop, coupled against per system, on the workload whose adsorbates stall:
the benchmark's PaiNN (H = 512, 6 layers) with its NATURAL head gain (bench.py --random-init-heads, not the x100 heads of
the headline), 256 systems x 200 atoms, T = 50, probability-flow ODE, one global placement table.  Prints one JSON line:

  coupled / per_system
                the default rule (one allclose over the batch) and denoising_pos_params["per_system"] = True.  The two
                alternate run by run in one process; wall_ms = median, min and max of --reps runs after a warm-up round,
                each between two device synchronisations; steps_applied; sum_steps = sum_b sample_steps[b] (coupled:
                B x steps_applied); inc_fraction = inc_rows / inc_rows_full of the incremental layers over the timed
                runs; stopped
  per_system    also: whether the systems that applied as many steps as the coupled run got the coupled run's bits
                (the run that also timed drop_frozen on and off is recorded in profiles/NOTES.md; the switch was retired)
  step_us       one step on resident scores, no forward: "three_launch" (coupled reduce / decide / apply) and "two_launch"
                (the per-system kernel + its finish launch), alternating round by round: median, min, max over
                --step-rounds rounds of --step-reps host-enqueued calls each, one synchronisation per round

Every child process runs under its own time limit; a child that fails ends the tool.

    python tools/time_sampler_per_system.py [--systems 256] [--atoms 200] [--steps 50] [--reps 7] [--step-reps 2000]
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


def _setup(a):
    import torch

    from adsorbdiff_amd.painn_denoising import PaiNN
    from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS
    from adsorbdiff_amd.synthetic import make_batch
    from adsorbdiff_amd.trainer import DenoisingTrainer

    torch.manual_seed(0)
    model = PaiNN(None, 50, 1, hidden_channels=512, num_layers=6, num_rbf=128, cutoff=10.0, max_neighbors=50,
                  scale_file=PAINN_NB6_SCALE_FACTORS, so3_denoising=True).eval()
    trainer = DenoisingTrainer(model, device=DEV)
    batch = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000)
    params = dict(num_steps=a.steps, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  placement_noise=torch.rand(a.systems, 3, generator=torch.Generator().manual_seed(0)))
    return model, trainer, batch, params


CONFIGS = (("coupled", dict(per_system=False)), ("per_system", dict(per_system=True)))


def _spread(xs, nd=2):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], nd), "min": round(xs[0], nd), "max": round(xs[-1], nd)}


def child_runs(a) -> dict:
    """The configurations in ONE process, alternating run by run (coupled, per_system, coupled, ...), so that drift of the
    machine falls on both alike; --reps rounds after one warm-up round."""
    import torch

    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc

    model, trainer, batch, params = _setup(a)
    eng = model.engine(torch.device(DEV))
    acc = {name: {"ms": [], "rows": 0, "rows_full": 0} for name, _ in CONFIGS}
    last = {}
    for rnd in range(a.reps + 1):
        for name, extra in CONFIGS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            den = Denoiser(batch.clone(), DiffTorchCalc(trainer), dict(params, **extra), device=DEV)
            out = den.run()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            c = eng.counters()   # totals since the run's set_incremental
            last[name] = (out, den)
            if rnd == 0:
                continue         # warm-up round: workspaces, packed weights
            acc[name]["ms"].append(ms)
            acc[name]["rows"] += int(c.inc_rows)
            acc[name]["rows_full"] += int(c.inc_rows_full)
    B, n = a.systems, a.atoms
    res = {}
    for name, extra in CONFIGS:
        out, den = last[name]
        per_system = extra["per_system"]
        r = {"wall_ms": _spread(acc[name]["ms"]), "steps_applied": int(den.steps_applied),
             "sum_steps": int(out.sample_steps.sum()) if per_system else B * int(den.steps_applied),
             "inc_fraction": round(acc[name]["rows"] / max(acc[name]["rows_full"], 1), 4)}
        if per_system:
            r["stopped"] = int(out.sample_stopped.sum())
        res[name] = r
    ps, cp = last["per_system"][0], last["coupled"]
    same = [i for i in range(B) if int(ps.sample_steps[i]) == int(cp[1].steps_applied)]
    res["per_system"]["systems_with_the_coupled_step_count"] = len(same)
    res["per_system"]["their_sites_equal_the_coupled_run"] = all(
        torch.equal(ps.pos[i * n:(i + 1) * n], cp[0].pos[i * n:(i + 1) * n]) for i in same)
    return res


def child_step(a) -> dict:
    """The step alone on resident scores: three launches (coupled) against two (per system)."""
    import torch

    from adsorbdiff_amd.denoising_torch import schedule_coefs

    model, trainer, batch, params = _setup(a)
    dev = torch.device(DEV)
    eng = model.engine(dev)
    b = batch.to(dev)
    prep = eng.prepare(b)
    B, N = prep.num_systems, prep.num_atoms
    pos = b.pos.clone().contiguous()
    eng.init_placement(prep, pos, params["placement_noise"].to(dev))
    coefs = schedule_coefs(params)
    coefs_dev = torch.tensor([[c.coef_tr, c.rot_pre, c.rot_dt, c.rot_g2, c.noise_tr, c.noise_rot] for c in coefs],
                             dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(1)
    f1 = (1e-3 * torch.randn(N, 3, generator=g)).to(dev)
    f2 = (1e-3 * torch.randn(N, 3, generator=g)).to(dev)
    times = {"three_launch": [], "two_launch": []}
    for rnd in range(a.step_rounds + 1):   # the two variants alternate round by round; round 0 is the warm-up
        for label, per_system in (("three_launch", False), ("two_launch", True)):
            state = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
            sys_state = torch.tensor([[0, 0, 0, -1]] * B, dtype=torch.int32, device=dev)
            eng.set_per_system_stop(sys_state if per_system else None)
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.step_reps):
                    eng.sde_step_scheduled(prep, pos, f1, f2, coefs_dev, a.steps, state, early_stop_count=0)
                torch.cuda.synchronize()
                if rnd:
                    times[label].append((time.perf_counter() - t0) * 1e6 / a.step_reps)
            finally:
                eng.set_per_system_stop(None)
    return {"step_us": {k: _spread(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-reps", type=int, default=2000)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--child", choices=("runs", "step"))
    ap.add_argument("--limit", type=int, default=400, help="seconds granted to each child")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps({"runs": child_runs, "step": child_step}[a.child](a)), flush=True)
        return
    res = {"systems": a.systems, "atoms": a.atoms, "steps": a.steps, "reps": a.reps, "head_gain": "natural"}
    for child in ("runs", "step"):
        cmd = [sys.executable, __file__, "--child", child, "--systems", str(a.systems), "--atoms", str(a.atoms), "--steps",
               str(a.steps), "--reps", str(a.reps), "--step-reps", str(a.step_reps), "--step-rounds", str(a.step_rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        if p.returncode != 0:
            raise SystemExit(f"{child}: exit status {p.returncode}\n{p.stderr[-3000:]}")
        res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
