"""Timing of the S2EF training step of the force field (PaiNNS2EFTrainStep) next to the denoiser's step (PaiNNTrainStep) on
the synthetic batch `bench.py --mode train` builds (make_batch(systems, seed=2000); H=512, 6 layers, 128 rbf, cutoff 10,
K=50; seeded weights).  Warm-up, then timed passes between device synchronisations, the two legs alternating in the same
process.  Prints one JSON line:

  s2ef_step_ms            PaiNNS2EFTrainStep.zero_grad + loss_and_grad: one gated force head, the energy head, the S2EF loss
  denoiser_step_ms        PaiNNTrainStep.zero_grad + loss_and_grad on the same batch: two gated heads, the score loss
  ratio                   s2ef_step_ms / denoiser_step_ms (expected at most 1.05: 2 % box noise, the rest for the extra loss
                          and energy-head launches)
  within_5_percent        ratio <= 1.05
  s2ef_train_step_ms      ForcesTrainer.train_step (the step plus flag read, clip, AdamW, EMA)
  graphs_per_s            systems / s2ef_train_step_ms
  energy_head_bwd_us      adf_op_energy_head_bwd alone at this shape (both launches): 20 calls back to back per timing
  energy_head_bwd_gbs     its algorithmic bytes (one read of he0 [N, H/2], one write of d(he0)) over that time
  loss_us                 adf_op_s2ef_loss alone (three launches)

    python tools/time_s2ef_train.py [--systems 256] [--reps 7] [--out profiles/s2ef_train.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from adsorbdiff_amd import lib as _lib  # noqa: E402
from adsorbdiff_amd.painn import PaiNN  # noqa: E402
from adsorbdiff_amd.painn_denoising import PaiNN as Denoiser  # noqa: E402
from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS  # noqa: E402
from adsorbdiff_amd.synthetic import make_batch  # noqa: E402
from adsorbdiff_amd.train_step import PaiNNS2EFTrainStep, PaiNNTrainStep  # noqa: E402
from adsorbdiff_amd.trainer import ForcesTrainer  # noqa: E402

DEV = "cuda:0"
HP = dict(hidden_channels=512, num_layers=6, num_rbf=128, cutoff=10.0, max_neighbors=50)
NORMALIZERS = {"energy": {"mean": -0.7, "stdev": 2.3}, "forces": {"mean": 0.0, "stdev": 1.7}}


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()

    b = make_batch(a.systems, seed=2000).to(DEV)
    B, N = a.systems, int(b.pos.shape[0])
    g = torch.Generator().manual_seed(2)
    b.energy = (NORMALIZERS["energy"]["mean"] + NORMALIZERS["energy"]["stdev"] * torch.randn(B, generator=g)).to(DEV)
    b.forces = (NORMALIZERS["forces"]["stdev"] * torch.randn(N, 3, generator=g)).to(DEV)
    targets = dict(tr_sigma=torch.rand(B, 1, generator=g) + 0.5, rot_sigma=torch.rand(B, 1, generator=g) * 0.5 + 0.1,
                   tr_score=torch.randn(B, 3, generator=g), rot_score=torch.randn(B, 3, generator=g))
    torch.manual_seed(0)
    ff = PaiNN(None, 50, 1, scale_file=dict(PAINN_NB6_SCALE_FACTORS), **HP).to(DEV)
    torch.manual_seed(0)
    den = Denoiser(None, 50, 1, so3_denoising=True, scale_file=dict(PAINN_NB6_SCALE_FACTORS), **HP).to(DEV)
    s2ef = PaiNNS2EFTrainStep(ff, DEV, normalizers=NORMALIZERS, force_coefficient=100)
    score = PaiNNTrainStep(den, DEV)

    def s2ef_leg():
        s2ef.zero_grad()
        s2ef.loss_and_grad(b)

    def score_leg():
        score.zero_grad()
        score.loss_and_grad(b, targets)

    legs = {"s2ef_step_ms": s2ef_leg, "denoiser_step_ms": score_leg}
    for fn in legs.values():   # warm-up: engines, workspaces, weight images
        fn()
        fn()
    times = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    out = {"systems": B, "atoms": N, **HP, "reps": a.reps}
    for k, v in times.items():
        out[k] = median(v)
        out[k.replace("_ms", "_min_ms")] = min(v)
    out["ratio"] = out["s2ef_step_ms"] / out["denoiser_step_ms"]
    out["within_5_percent"] = bool(out["ratio"] <= 1.05)
    del score, den

    # the two new operators alone at this shape
    lib = _lib.load()
    H2 = HP["hidden_channels"] // 2
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    eng = ff.engine(DEV, refresh=False)
    prep = eng.prepare(b)
    he0 = torch.randn(N, H2, device=DEV)
    dhe0, dE = torch.empty(N, H2, device=DEV), torch.randn(B, device=DEV)
    w2, dW2, db2 = torch.randn(H2, device=DEV), torch.zeros(H2, device=DEV), torch.zeros(1, device=DEV)
    scratch = torch.empty(int(lib.adf_op_energy_head_bwd_scratch(N, H2)), device=DEV)

    def head():
        _lib.check(lib.adf_op_energy_head_bwd(he0.data_ptr(), w2.data_ptr(), dE.data_ptr(), prep.batch.data_ptr(),
                                              dhe0.data_ptr(), dW2.data_ptr(), db2.data_ptr(), 1, N, H2, scratch.data_ptr(),
                                              stream))

    e_pred, f_pred = torch.randn(B, device=DEV), torch.randn(N, 3, device=DEV)
    loss, dF, met = torch.empty(3, device=DEV), torch.empty(N, 3, device=DEV), torch.empty(2, device=DEV)
    lscratch = torch.empty(int(lib.adf_op_s2ef_loss_scratch(B)), device=DEV)
    f = C.c_float

    def loss_op():
        _lib.check(lib.adf_op_s2ef_loss(e_pred.data_ptr(), f_pred.data_ptr(), b.energy.data_ptr(), b.forces.data_ptr(),
                                        prep.fixed.data_ptr(), prep.atom_offset.data_ptr(), B, 1, f(-0.7), f(2.3), f(0.0), f(1.7),
                                        f(1.0), f(100.0), None, loss.data_ptr(), dE.data_ptr(), dF.data_ptr(), met.data_ptr(),
                                        lscratch.data_ptr(), stream))

    for fn in (head, loss_op):
        for _ in range(3):
            fn()
    out["energy_head_bwd_us"] = 1e3 * median([timed(lambda: [head() for _ in range(20)]) / 20 for _ in range(max(a.reps, 15))])
    out["energy_head_bwd_bytes"] = 2 * 4 * N * H2
    out["energy_head_bwd_gbs"] = out["energy_head_bwd_bytes"] / (out["energy_head_bwd_us"] * 1e-6) / 1e9
    out["loss_us"] = 1e3 * median([timed(lambda: [loss_op() for _ in range(20)]) / 20 for _ in range(max(a.reps, 15))])

    # the trainer's whole step
    tr = ForcesTrainer(ff, device=DEV, normalizers=NORMALIZERS)
    tr.setup_training(1e-4, force_coefficient=100)
    for _ in range(2):
        tr.train_step(b)
    out["s2ef_train_step_ms"] = median([timed(lambda: tr.train_step(b)) for _ in range(a.reps)])
    out["graphs_per_s"] = B / (out["s2ef_train_step_ms"] * 1e-3)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
