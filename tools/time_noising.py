"""Timing of the forward noising of a training batch at the training shape: 256 systems x 200 atoms (synthetic slabs +
4-atom adsorbates).  Prints one JSON line:

  host_tr_so3_ms      noising.tr_so3_schedule on a batch resident on the device (the default path of train_step): wall
                      time per call between two device synchronisations, the mean of --reps calls after a warm-up.  It
                      contains the two stream synchronisations of that path (rot_sigma to the host, rotations and scores back)
  device_tr_so3_ms    DeviceNoiser.tr_so3 (draws + adf_noise_tr_so3), same clock; nothing is read back
  device_com_ms       DeviceNoiser.com (draws + adf_noise_com), same clock
  train_step_ms       {"host": ..., "device": ...}: DenoisingTrainer.train_step of the benchmark's model (H = 512, 6 layers)
                      with noise_on_device off and on, in ONE process, --steps steps after --warmup each

Every measurement runs in a child process of its own under its own time limit; a child that fails ends the tool.

    python tools/time_noising.py [--systems 256] [--atoms 200] [--reps 20] [--steps 10] [--warmup 3] [--skip-train]
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
PARAMS = dict(ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55)


def wall_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def child_noising(a) -> dict:
    import numpy as np
    import torch

    from adsorbdiff_amd import noising
    from adsorbdiff_amd.so3_tables import Igso3Tables
    from adsorbdiff_amd.synthetic import make_batch

    tables = Igso3Tables.shared()
    b = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=2000).to(DEV)
    torch.manual_seed(0)
    np.random.seed(0)
    nz = noising.DeviceNoiser(PARAMS, tables, DEV, seed=0)
    keys = noising.noise_keys(b).to(DEV)
    step = [0]

    def dev(fn):
        step[0] += 1
        return fn(b.clone(), step=step[0], keys=keys)

    return {"host_tr_so3_ms": round(wall_ms(lambda: noising.tr_so3_schedule(b.clone(), PARAMS, tables), a.reps), 4),
            "device_tr_so3_ms": round(wall_ms(lambda: dev(nz.tr_so3), a.reps), 4),
            "device_com_ms": round(wall_ms(lambda: dev(nz.com), a.reps), 4)}


def child_train(a) -> dict:
    import numpy as np
    import torch

    from adsorbdiff_amd.painn_denoising import PaiNN
    from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS
    from adsorbdiff_amd.so3_tables import Igso3Tables
    from adsorbdiff_amd.synthetic import make_batch
    from adsorbdiff_amd.trainer import DenoisingTrainer

    out = {}
    batch = make_batch(a.systems, n_slab=a.atoms - 4, n_ads=4, seed=2000).to(DEV)
    for label, on in (("host", False), ("device", True)):
        torch.manual_seed(0)
        np.random.seed(2000)
        model = PaiNN(None, 50, 1, hidden_channels=512, num_layers=6, num_rbf=128, cutoff=10.0, max_neighbors=50,
                      scale_file=PAINN_NB6_SCALE_FACTORS, so3_denoising=True)
        tr = DenoisingTrainer(model, device=DEV)
        tr.setup_training(PARAMS, lr=1e-4, tables=Igso3Tables.shared(), noise_on_device=on)
        for _ in range(a.warmup):
            tr.train_step(batch.clone())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.train_step(batch.clone())
        torch.cuda.synchronize()
        out[label] = round((time.perf_counter() - t0) * 1e3 / a.steps, 3)
        del tr, model
    return {"train_step_ms": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--child", choices=("noising", "train"))
    ap.add_argument("--limit", type=int, default=300, help="seconds granted to each child")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps({"noising": child_noising, "train": child_train}[a.child](a)), flush=True)
        return
    res = {"systems": a.systems, "atoms": a.atoms, "reps": a.reps}
    for child in ("noising",) + (() if a.skip_train else ("train",)):
        cmd = [sys.executable, __file__, "--child", child, "--systems", str(a.systems), "--atoms", str(a.atoms), "--reps",
               str(a.reps), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        if p.returncode != 0:
            raise SystemExit(f"{child}: exit status {p.returncode}\n{p.stderr[-3000:]}")
        res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
