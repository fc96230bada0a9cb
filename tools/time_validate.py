"""Timing of the evaluation path (csrc/evaluate.hip, adsorbdiff_amd/evaluator.py) next to the same metrics written as eager
torch ops on the device with the reference's algorithm (modules/evaluator.py, OCPTrainer._compute_metrics): one ``.item()``
per metric, a Python loop over the systems with a ``.max()`` each for energy_forces_within_threshold, one ``.item()`` per
system for the free-atom counts, every system taken to numpy and a host loop over the 490 thresholds for
average_distance_within_threshold.  256 systems of 80 atoms (make_batch(256, n_slab=76, n_ads=4)); H=512, 6 layers, 128 rbf,
cutoff 10, K=50 for the full validate batch.  Wall-clock times between device synchronisations (the eager leg is host-bound:
its device time says nothing), medians over ``--reps`` after a warm-up.  Prints one JSON line:

  kernels_s2ef_us / _is2rs_us / _is2re_us     one call of the entry (its launches), enqueued 20 times back to back
  kernels_all_with_read_us                    the three entries and one ``result()`` read
  eager_s2ef_us / _is2rs_us / _is2re_us       the eager restatement of the same metrics, reads included
  validate_batch_ms                           ``ForcesTrainer.validate`` on one batch (forward, loss, metrics, read)
  predict_batch_ms                            ``ForcesTrainer.predict`` on the same batch (the forward alone)
  eager_validate_batch_ms                     ``predict`` + the eager s2ef metrics

No speed-up is asserted anywhere; the figures go into DESIGN.md section 6c.

    python tools/time_validate.py [--systems 256] [--reps 7] [--out profiles/validate.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from adsorbdiff_amd.evaluator import DeviceMetrics, Evaluator, atom_offsets, distance_thresholds  # noqa: E402
from adsorbdiff_amd.painn import PaiNN  # noqa: E402
from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS  # noqa: E402
from adsorbdiff_amd.synthetic import make_batch  # noqa: E402
from adsorbdiff_amd.trainer import ForcesTrainer  # noqa: E402

DEV = "cuda:0"
HP = dict(hidden_channels=512, num_layers=6, num_rbf=128, cutoff=10.0, max_neighbors=50)
NORMALIZERS = {"energy": {"mean": -0.7, "stdev": 2.3}, "forces": {"mean": 0.0, "stdev": 1.7}}


def wall_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


# ---------------------------------------------------------------------------------------- the eager restatement
def eager_free_counts(fixed, natoms):
    mask = fixed == 0
    out, s = [], 0
    for n in natoms.tolist():
        out.append(torch.sum(mask[s:s + n]).item())
        s += n
    return mask, out


def eager_stat(err):
    return {"metric": torch.mean(err).item(), "total": torch.sum(err).item(), "numel": err.numel()}


def eager_s2ef(e_pred, f_pred, e_tgt, f_tgt, fixed, natoms):
    mask, nfree = eager_free_counts(fixed, natoms)
    p, t = f_pred[mask], f_tgt[mask]
    m = {"energy_mae": eager_stat((e_tgt - e_pred).abs())}
    for k, name in enumerate(("forcesx_mae", "forcesy_mae", "forcesz_mae")):
        m[name] = eager_stat((t[:, k] - p[:, k]).abs())
    m["forces_mae"] = eager_stat((t - p).abs())
    m["forces_cosine_similarity"] = eager_stat(torch.cosine_similarity(p, t))
    m["forces_magnitude_error"] = eager_stat((p.norm(dim=-1) - t.norm(dim=-1)).abs())
    ef, ee = (t - p).abs(), (e_tgt - e_pred).abs()
    ok, s = 0, 0
    for i, n in enumerate(nfree):
        if ee[i] < 0.02 and ef[s:s + n].max() < 0.03:
            ok += 1
        s += n
    m["energy_forces_within_threshold"] = {"metric": ok / len(nfree), "total": ok, "numel": len(nfree)}
    return m


def eager_is2rs(pos_pred, pos_tgt, cell, fixed, natoms):
    mask, nfree = eager_free_counts(fixed, natoms)
    p, t = pos_pred[mask], pos_tgt[mask]
    means = []
    for i, (a, b) in enumerate(zip(torch.split(p, nfree), torch.split(t, nfree))):
        c = cell[i].detach().cpu().numpy()
        frac = np.linalg.solve(c.T, (a.detach().cpu().numpy() - b.detach().cpu().numpy()).T).T
        frac %= 1.0
        frac %= 1.0
        frac[frac > 0.5] -= 1
        means.append(np.mean(np.linalg.norm(frac @ c, axis=1)))
    ok = 0
    for thr in distance_thresholds():
        ok += sum(np.array(means) < thr)
    total = len(means) * len(distance_thresholds())
    return {"positions_average_distance_within_threshold": {"metric": ok / total, "total": ok, "numel": total},
            "positions_mae": eager_stat((t - p).abs()), "positions_mse": eager_stat((t - p) ** 2)}


def eager_is2re(e_pred, e_tgt):
    err = (e_tgt - e_pred).abs()
    ok = (err < 0.02).sum().item()
    return {"energy_mae": eager_stat(err), "energy_mse": eager_stat((e_tgt - e_pred) ** 2),
            "energy_within_threshold": {"metric": ok / err.numel(), "total": ok, "numel": err.numel()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()

    b = make_batch(a.systems, n_slab=76, n_ads=4, seed=3000).to(DEV)
    B, N = a.systems, int(b.pos.shape[0])
    g = torch.Generator().manual_seed(2)
    b.energy = (NORMALIZERS["energy"]["mean"] + NORMALIZERS["energy"]["stdev"] * torch.randn(B, generator=g)).to(DEV)
    b.forces = (NORMALIZERS["forces"]["stdev"] * torch.randn(N, 3, generator=g)).to(DEV)
    e_pred = b.energy + 0.03 * torch.randn(B, generator=g).to(DEV)
    f_pred = b.forces + 0.02 * torch.randn(N, 3, generator=g).to(DEV)
    pos_pred = b.pos + 0.1 * torch.randn(N, 3, generator=g).to(DEV)
    off, fixed = atom_offsets(b.natoms, DEV), b.fixed.to(torch.int32)
    cell = b.cell.reshape(B, 3, 3)
    dm = DeviceMetrics(DEV)
    legs = {
        "s2ef": (lambda: dm.add_s2ef(e_pred, f_pred, b.energy, b.forces, off, fixed=fixed),
                 lambda: eager_s2ef(e_pred, f_pred, b.energy, b.forces, b.fixed, b.natoms)),
        "is2rs": (lambda: dm.add_is2rs(pos_pred, b.pos, cell, off, fixed=fixed),
                  lambda: eager_is2rs(pos_pred, b.pos, cell, b.fixed, b.natoms)),
        "is2re": (lambda: dm.add_is2re(e_pred, b.energy), lambda: eager_is2re(e_pred, b.energy)),
    }
    out = {"systems": B, "atoms": N, "reps": a.reps}
    agree = {}
    for task, (kernel, eager) in legs.items():
        dm.zero()
        kernel()
        got, want = dm.result(Evaluator(task).metric_names()), eager()
        agree[task] = max(abs(got[k]["total"] - want[k]["total"]) / max(abs(want[k]["total"]), 1e-30) for k in want)
        for _ in range(2):
            kernel()
        out[f"kernels_{task}_us"] = median([wall_us(lambda: [kernel() for _ in range(20)]) / 20 for _ in range(max(a.reps, 15))])
        out[f"eager_{task}_us"] = median([wall_us(eager) for _ in range(a.reps)])
    out["kernel_vs_eager_worst_relative_difference"] = agree

    def all_with_read():
        dm.zero()
        for kernel, _ in legs.values():
            kernel()
        dm.result()

    out["kernels_all_with_read_us"] = median([wall_us(all_with_read) for _ in range(max(a.reps, 15))])

    # one full validation batch
    torch.manual_seed(0)
    ff = PaiNN(None, 50, 1, scale_file=dict(PAINN_NB6_SCALE_FACTORS), **HP).to(DEV)
    tr = ForcesTrainer(ff, device=DEV, normalizers=NORMALIZERS)

    def eager_validate():
        o = tr.predict(b)
        eager_s2ef(o["energy"], o["forces"], b.energy, b.forces, b.fixed, b.natoms)

    for fn in (lambda: tr.validate([b]), lambda: tr.predict(b), eager_validate):
        fn()
        fn()
    out["validate_batch_ms"] = 1e-3 * median([wall_us(lambda: tr.validate([b])) for _ in range(a.reps)])
    out["predict_batch_ms"] = 1e-3 * median([wall_us(lambda: tr.predict(b)) for _ in range(a.reps)])
    out["eager_validate_batch_ms"] = 1e-3 * median([wall_us(eager_validate) for _ in range(a.reps)])
    out.update(HP)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
