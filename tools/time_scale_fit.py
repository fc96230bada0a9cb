"""Timing of one full scale-factor fit (adsorbdiff_amd/scaling.py::fit_scale_factors, csrc/scale_fit.hip) at the benchmark
width: the denoiser with H = 512, 6 layers, 128 radial functions, cutoff 12 A, 50 neighbours; 16 batches of 64 systems of
200 atoms.  Taken once with HIP events around the whole fit (after one warm-up fit of a single batch, which creates the
engine and grows its workspaces), and the column-variance kernel alone on one [12800, 512] table.  Prints one JSON line:

  fit_ms                 mode "all": 6 factors x 16 batches, factor l costing l + 1 layers per batch; weight re-binding,
                         host reads (one per batch and factor) and batch preparation included
  fit_value              the six fitted values
  observe_full_ms        one forward_observe of one batch through all six layers
  forward_ms             one plain forward of the same batch (heads included)
  column_variance_us     the four launches of adf_op_column_variance on [12800, 512], mean of 20 back to back

A record, not a gate: nothing asserts these figures; they go into DESIGN.md section 6f.

    python tools/time_scale_fit.py [--out profiles/scale_fit.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from adsorbdiff_amd import lib as L  # noqa: E402
from adsorbdiff_amd.painn_denoising import PaiNN  # noqa: E402
from adsorbdiff_amd.scaling import fit_scale_factors  # noqa: E402
from adsorbdiff_amd.synthetic import make_batch  # noqa: E402

DEV = "cuda:0"
HP = dict(hidden_channels=512, num_layers=6, num_rbf=128, cutoff=12.0, max_neighbors=50)


def event_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=64)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()

    torch.manual_seed(0)
    m = PaiNN(None, 50, 1, so3_denoising=True, **HP).to(DEV).eval()
    batches = [make_batch(a.systems, seed=4000 + i).to(DEV) for i in range(a.batches)]
    fit_scale_factors(m, batches[:1])          # warm-up: engine, workspaces
    res = {}

    def fit():
        res.update(fit_scale_factors(m, batches, num_batches=a.batches))

    out = {"systems": a.systems, "atoms": int(batches[0].pos.shape[0]), "batches": a.batches, **HP}
    out["fit_ms"] = event_ms(fit)
    out["fit_value"] = [r["value"] for r in res.values()]
    eng = m.engine(DEV)
    out["exact_f32"] = bool(eng.exact_f32)     # True: an activation left the fp16 range and the engine switched
    eng.forward_observe(batches[0])
    out["observe_full_ms"] = event_ms(lambda: eng.forward_observe(batches[0]), 3)
    m(batches[0])
    out["forward_ms"] = event_ms(lambda: m(batches[0]), 3)

    lib = L.load()
    N, H = out["atoms"], HP["hidden_channels"]
    x = torch.randn(N, H, device=DEV)
    var = torch.empty(1, dtype=torch.float64, device=DEV)
    scratch = torch.empty(int(lib.adf_op_column_variance_scratch(N, H)) // 8, dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def kernel():
        L.check(lib.adf_op_column_variance(x.data_ptr(), N, H, var.data_ptr(), scratch.data_ptr(), stream))

    kernel()
    out["column_variance_us"] = 1e3 * event_ms(kernel, 20)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
