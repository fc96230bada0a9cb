"""Timing of ml_relax at the relaxation shape: 1000 systems x 200 atoms, the OC20 PaiNN width (H=512, 6 layers, 128 rbf,
cutoff 12, K=50; seeded weights) and the L-BFGS settings of configs/relaxation/gemnet_oc/gemnet_relax.yml:28-32
(maxstep 0.04, memory 50, damping 1.0, alpha 70).  Prints one JSON line:

  forward_ms          one S2EF forward (energy + forces, adf_painn_forward_energy incl. its error-flag check)
  lbfgs_step_ms       one adf_lbfgs_step alone with a full history (50 entries: 1 + 2 x 50 + 2 launches)
  lbfgs_converge_ms   one adf_lbfgs_converge (per-system max force and update mask, 1 launch without the flag)
  torch_step_ms       the same step in eager torch ops on the same GPU (TorchOpsLBFGS below)
  iterations_per_s    LBFGS.run iterations per second (forward + convergence check + step)

With --per-system, in the same process (the default-mode figures above stay as they are):

  lbfgs_step_ms_per_system      one adf_lbfgs_step in per-system mode with a full history (one launch)
  lbfgs_step_ms_per_system_b1   the same for ONE system of --atoms atoms (one workgroup walks the whole step)
  lbfgs_step_ms_b1              the coupled step for that one system
  iterations_to_convergence     LBFGS.run iterations in both modes on the harmonic fixture (relax_harmonic.npz) and on the
                                relax_run.npz batch with the small seeded S2EF PaiNN, --converge-steps at the most

With --drop-converged, INSTEAD of the figures above (one process, the same model and shape): LBFGS.run with
set_drop_converged off and on, alternating, --drop-repeats each, under a convergence SCHEDULE - a calculator wrapper zeroes
the force rows of system b from a seeded iteration c_b on, so that its mask clears there.  This is a schedule, not physics:
it fixes which systems are dropped when, and the forward that is timed is the real one.  Two legs: "overhead" (c_b =
--drop-steps for every system: nothing drops early) and "staggered" (c_b uniform over 1 .. --drop-steps).  One JSON line per
run (wall_ms, iterations, system_forwards, atom_forwards from LBFGS.forward_log, compaction_ms_per_iteration = the device
time of build + gather + scatter) and one summary line per leg (on / off time ratio, evaluated-atom share, the spread of
the off setting); --out writes the same lines as a JSON array.

    python tools/time_relax.py [--systems 1000] [--atoms 200] [--reps 20] [--per-system]
    python tools/time_relax.py --drop-converged [--drop-steps 20] [--drop-repeats 2] [--out profiles/relax_drop_converged.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from adsorbdiff_amd import lib as _lib  # noqa: E402
from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc  # noqa: E402
from adsorbdiff_amd.painn import PaiNN  # noqa: E402
from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS  # noqa: E402
from adsorbdiff_amd.synthetic import make_batch  # noqa: E402
from adsorbdiff_amd.trainer import ForcesTrainer  # noqa: E402

DEV = "cuda:0"
OPT = dict(maxstep=0.04, memory=50, damping=1.0, alpha=70.0)


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


class TorchOpsLBFGS:
    """Baseline: the batched L-BFGS step restated with torch tensor ops on the GPU, one op per algorithmic step as an
    eager implementation issues them - what adf_lbfgs_step replaces.  History: python lists trimmed to `memory`
    entries, oldest first; curvature pairs (ds, dg) with weights w = 1 / <dg, ds>; the direction comes from the two-loop
    recursion with the scalar initial inverse Hessian h0 = 1 / alpha; each system's direction is rescaled so that its
    longest atomic displacement is at most `max_len`, then damped; a step whose largest component is below 1e-7 is dropped
    (a device-to-host read, as in an eager loop), else it is added to the masked atoms in f32."""

    def __init__(self, atom_sys, n_sys, memory, max_len, damping, alpha):
        self.atom_sys, self.n_sys, self.memory = atom_sys, n_sys, memory
        self.max_len, self.damping, self.h0 = max_len, damping, 1.0 / alpha
        self.ds, self.dg, self.w = [], [], []
        self.prev_x = self.prev_g = None

    def _remember(self, x, grad):
        ds = torch.sub(x, self.prev_x).reshape(-1)
        dg = torch.sub(grad, self.prev_g).reshape(-1)
        for lst, v in ((self.ds, ds), (self.dg, dg), (self.w, torch.dot(dg, ds).reciprocal())):
            lst.append(v)
            if len(lst) > self.memory:
                lst.pop(0)

    def direction(self, grad, n_hist):
        v = grad.reshape(-1).clone()
        a = grad.new_empty(n_hist)
        for j in reversed(range(n_hist)):
            a[j] = self.w[j] * torch.dot(self.ds[j], v)
            v -= a[j] * self.dg[j]
        v = self.h0 * v
        for j in range(n_hist):
            b = self.w[j] * torch.dot(self.dg[j], v)
            v += self.ds[j] * (a[j] - b)
        return -v.reshape(-1, 3)

    def scaled(self, d):
        atom_len = torch.linalg.vector_norm(d, dim=1)
        longest = torch.zeros(self.n_sys, dtype=d.dtype, device=d.device).scatter_reduce_(
            0, self.atom_sys, atom_len, "amax", include_self=False).index_select(0, self.atom_sys)
        factor = torch.minimum(longest, torch.full_like(longest, self.max_len)) * torch.reciprocal(longest + 1e-7)
        return d * factor.unsqueeze(1) * self.damping

    def step(self, pos, forces64, it, atom_mask):
        x = pos.to(torch.float64)
        grad = -forces64                         # the gradient of the energy
        if it > 0:
            self._remember(x, grad)
        move = self.scaled(self.direction(grad, min(self.memory, it)))
        if float(move.abs().max()) < 1e-7:
            return
        pos.add_(move.masked_fill(~atom_mask.unsqueeze(1), 0.0).to(torch.float32))
        self.prev_x, self.prev_g = x, grad


def time_device_step(natoms, pos0, fs, reps, per_system):
    """(step ms, converge ms) of adf_lbfgs_step / adf_lbfgs_converge with a full history, in either mode."""
    lib = _lib.load()
    B, N = int(natoms.shape[0]), int(pos0.shape[0])
    off = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    off[1:] = torch.cumsum(natoms, 0).to(torch.int32)
    h = C.c_void_p()
    _lib.check(lib.adf_lbfgs_create(N, B, OPT["memory"], OPT["maxstep"], OPT["damping"], OPT["alpha"], 0, C.byref(h)))
    if per_system:
        _lib.check(lib.adf_lbfgs_set_per_system(h, 1))
    pos = pos0.clone().float().contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mf = torch.empty(B, dtype=torch.float64, device=DEV)
    it = [0]

    def dev_converge():
        _lib.check(lib.adf_lbfgs_converge(h, off.data_ptr(), fs[it[0] % 4].data_ptr(), 1e-9, mf.data_ptr(), None, stream))

    def dev_step():
        _lib.check(lib.adf_lbfgs_step(h, off.data_ptr(), pos.data_ptr(), fs[it[0] % 4].data_ptr(), it[0], stream))
        it[0] += 1

    for _ in range(OPT["memory"] + 1):
        dev_converge()
        dev_step()
    dev_converge()   # the update mask of the timed steps (every system moves: fmax 1e-9)
    step_ms = timed(dev_step, reps)
    conv_ms = timed(dev_converge, reps)
    torch.cuda.synchronize()
    lib.adf_lbfgs_destroy(h)
    return step_ms, conv_ms


class HarmonicTrainer:
    """F = -k (x - x*) per system (the calculator of tests/golden/relax_harmonic.npz)."""

    def __init__(self, fx):
        self._unwrapped_model = type("M", (), {"otf_graph": True})()
        self.xstar = torch.from_numpy(fx["xstar"]).to(DEV)
        self.k = torch.from_numpy(fx["k"]).to(DEV)

    def predict(self, batch, per_image=False, disable_tqdm=True):
        kk = self.k[batch.batch].reshape(-1, 1)
        d = batch.pos - self.xstar
        e = torch.zeros(int(batch.natoms.shape[0]), device=DEV).index_add_(0, batch.batch, (0.5 * kk * d * d).sum(1))
        return {"energy": e, "forces": -kk * d}


def fixture_batch(fx):
    from adsorbdiff_amd.data import Batch

    b = Batch()
    b.pos = torch.from_numpy(fx["pos_in"]).float().clone()
    b.atomic_numbers = torch.from_numpy(fx["atomic_numbers"]).float()
    for k in ("tags", "fixed", "natoms", "batch"):
        setattr(b, k, torch.from_numpy(fx[k]).long())
    b.cell = torch.from_numpy(fx["cell"]).float()
    b.sid = [str(i) for i in range(len(b.natoms))]
    return b.to(DEV)


def iterations_to_convergence(max_steps):
    """LBFGS.run iterations (and the systems still unconverged at the end) in both modes: report only."""
    import numpy as np

    gold = Path(__file__).resolve().parent.parent / "tests" / "golden"
    res = {}
    with np.load(gold / "relax_harmonic.npz") as z:
        fx = {k: z[k] for k in z.files}
    cases = [("harmonic", fx, HarmonicTrainer(fx))]
    with np.load(gold / "relax_run.npz") as z:
        fx = {k: z[k] for k in z.files}
    torch.manual_seed(int(fx["seed"]))
    small = PaiNN(None, 50, 1, hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20,
                  scale_file={"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}).to(DEV).eval()
    cases.append(("relax_run", fx, ForcesTrainer(small, device=DEV)))
    for name, fx, tr in cases:
        for mode, per_system in (("coupled", False), ("per_system", True)):
            opt = LBFGS(fixture_batch(fx), TorchCalc(tr), maxstep=0.04, memory=int(fx["memory"]), damping=1.0, alpha=70.0,
                        device=DEV, per_system=per_system)
            opt.run(fmax=float(fx["fmax"]), steps=max_steps)
            last = opt.max_force_log[-1]
            res[f"{name}_{mode}"] = {"iterations": opt.iterations, "unconverged": int((last >= float(fx["fmax"])).sum()),
                                     "per_system_iterations": torch.stack(opt.max_force_log).ge(float(fx["fmax"])).sum(0).tolist()}
    return res


class ScheduledCalc(TorchCalc):
    """TorchCalc whose forces of system b are zero from call number c_b on (looked up by ``sid``, so it works on the compact
    batches of drop_converged too).  A schedule of convergence, not physics."""

    def __init__(self, trainer, sids, cutoff):
        super().__init__(trainer)
        self.row = {s: i for i, s in enumerate(sids)}
        self.cutoff = torch.as_tensor(cutoff, dtype=torch.int64, device=DEV)
        self.calls = 0

    def get_energy_and_forces(self, atoms, apply_constraint=True):
        energy, forces = super().get_energy_and_forces(atoms, apply_constraint)
        rows = torch.tensor([self.row[s] for s in atoms.sid], dtype=torch.int64).to(DEV)
        done = self.cutoff[rows] <= self.calls
        self.calls += 1
        return energy, forces.masked_fill(done[atoms.batch].reshape(-1, 1), 0)


def drop_converged_legs(model, a):
    """The two legs of --drop-converged; returns the JSON-able lines."""
    tr = ForcesTrainer(model, device=DEV)
    cpu_batch = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000)
    B, steps = a.systems, a.drop_steps
    g = torch.Generator().manual_seed(7)
    legs = {"overhead": [steps] * B, "staggered": torch.randint(1, steps + 1, (B,), generator=g).tolist()}
    lines = []

    def run(cutoff, drop, n_steps):
        b = cpu_batch.clone().to(DEV)
        opt = LBFGS(b, ScheduledCalc(tr, b.sid, cutoff), device=DEV, **OPT)
        opt.set_drop_converged(drop)
        opt.time_compaction = drop
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.run(fmax=1e-9, steps=n_steps)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return opt, b, ms

    settings = {"both": (False, True), "off": (False,), "on": (True,)}[a.drop_only]
    if a.drop_leg != "both":
        legs = {a.drop_leg: legs[a.drop_leg]}
    if not a.drop_no_warmup:
        for drop in settings:       # workspaces, allocator: not timed
            run(legs[next(iter(legs))], drop, 3)
    for leg, cutoff in legs.items():
        res = {False: [], True: []}
        for rep in range(a.drop_repeats):
            for drop in settings:
                opt, b, ms = run(cutoff, drop, steps)
                line = {"leg": leg, "setting": "on" if drop else "off", "repeat": rep, "schedule": "seeded, not physics",
                        "systems": B, "atoms": int(b.pos.shape[0]), "steps": steps, "wall_ms": ms,
                        "iterations": opt.iterations, "model_calls": len(opt.forward_log),
                        "system_forwards": sum(s for s, _ in opt.forward_log),
                        "atom_forwards": sum(n for _, n in opt.forward_log)}
                if drop:
                    line["compaction_ms_per_iteration"] = opt.compaction_ms() / max(1, opt.iterations)
                res[drop].append((line, b.pos.clone(), torch.stack(opt.max_force_log)))
                lines.append(line)
                print(json.dumps(line), flush=True)
        if len(settings) < 2:       # one setting alone (a kernel-trace run of its own): no comparison to print
            continue
        off = [r[0]["wall_ms"] for r in res[False]]
        on = [r[0]["wall_ms"] for r in res[True]]
        summary = {"leg": leg, "summary": True,
                   "off_ms_mean": sum(off) / len(off), "on_ms_mean": sum(on) / len(on),
                   "off_spread_ms": max(off) - min(off), "on_spread_ms": max(on) - min(on),
                   "on_over_off": (sum(on) / len(on)) / (sum(off) / len(off)),
                   "evaluated_atom_share": res[True][0][0]["atom_forwards"] / res[False][0][0]["atom_forwards"],
                   "same_positions_and_max_forces": bool(torch.equal(res[True][0][1], res[False][0][1])
                                                         and torch.equal(res[True][0][2], res[False][0][2]))}
        lines.append(summary)
        print(json.dumps(summary), flush=True)
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=1000)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run-steps", type=int, default=8)
    ap.add_argument("--per-system", action="store_true", help="also time the per-system mode and count iterations in both")
    ap.add_argument("--converge-steps", type=int, default=200)
    ap.add_argument("--drop-converged", action="store_true", help="time LBFGS.run with set_drop_converged off and on")
    ap.add_argument("--drop-steps", type=int, default=20)
    ap.add_argument("--drop-repeats", type=int, default=2)
    ap.add_argument("--drop-only", choices=("both", "off", "on"), default="both",
                    help="one setting alone, for a profiler run of its own (no summary line)")
    ap.add_argument("--drop-leg", choices=("both", "overhead", "staggered"), default="both")
    ap.add_argument("--drop-no-warmup", action="store_true", help="skip the untimed warm-up runs (kernel traces)")
    ap.add_argument("--out", type=Path, default=None, help="--drop-converged: also write the lines as a JSON array")
    a = ap.parse_args()
    torch.manual_seed(0)
    model = PaiNN(None, 50, 1, hidden_channels=512, num_layers=6, num_rbf=128, cutoff=12.0, max_neighbors=50,
                  scale_file=dict(PAINN_NB6_SCALE_FACTORS)).to(DEV).eval()
    if a.drop_converged:
        lines = drop_converged_legs(model, a)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            a.out.write_text(json.dumps(lines, indent=1) + "\n")
        return
    b = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000).to(DEV)
    N, B = int(b.pos.shape[0]), a.systems
    out = {"systems": B, "atoms": N, **OPT}

    with torch.no_grad():
        model(b)   # engine, workspaces
        out["forward_ms"] = timed(lambda: model(b), a.reps)

    # one adf_lbfgs_step with a full history (synthetic forces; the arithmetic does not depend on their values)
    g = torch.Generator(device=DEV).manual_seed(1)
    fs = [torch.randn(N, 3, device=DEV, generator=g) * 0.1 for _ in range(4)]
    step_ms, conv_ms = time_device_step(b.natoms.to(DEV), b.pos, fs, a.reps, per_system=False)
    out["lbfgs_step_ms"], out["lbfgs_converge_ms"] = step_ms, conv_ms
    if a.per_system:
        out["lbfgs_step_ms_per_system"] = time_device_step(b.natoms.to(DEV), b.pos, fs, a.reps, per_system=True)[0]
        one = b.natoms[:1].to(DEV)
        n1 = int(one[0])
        fs1 = [f[:n1].contiguous() for f in fs]
        out["lbfgs_step_ms_b1"] = time_device_step(one, b.pos[:n1], fs1, a.reps, per_system=False)[0]
        out["lbfgs_step_ms_per_system_b1"] = time_device_step(one, b.pos[:n1], fs1, a.reps, per_system=True)[0]
        out["iterations_to_convergence"] = iterations_to_convergence(a.converge_steps)

    # the same step in eager torch ops, full history
    base = TorchOpsLBFGS(b.batch.to(DEV), B, OPT["memory"], OPT["maxstep"], OPT["damping"], OPT["alpha"])
    pos_t = b.pos.clone().float()
    mask = torch.ones(N, dtype=torch.bool, device=DEV)
    itt = [0]

    def torch_step():
        base.step(pos_t, fs[itt[0] % 4].double(), itt[0], mask)
        itt[0] += 1

    for _ in range(OPT["memory"] + 1):
        torch_step()
    out["torch_step_ms"] = timed(torch_step, a.reps)
    del base

    # LBFGS.run iterations per second (fmax tiny: no system converges)
    tr = ForcesTrainer(model, device=DEV)
    b2 = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=1000).to(DEV)
    opt = LBFGS(b2, TorchCalc(tr), device=DEV, **OPT)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt.run(fmax=1e-9, steps=a.run_steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["run_iterations"] = opt.iterations
    out["iterations_per_s"] = opt.iterations / dt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
