"""Timing of flag_anomalies at the relaxation shape: 1000 systems x 200 atoms (synthetic slabs + adsorbates, a seeded radius
table in [0.3, 1.6] A, final frame = initial + 0.1 A noise with every fourth adsorbate lifted by 4.5 A).  Prints one JSON line:

  flag_anomalies_ms   device time of one flag_anomalies call (adf_flag_anomalies and the host plumbing around it), the mean
                      of --reps calls after a warm-up
  torch_ms            the same definition in batched torch ops on the same GPU (torch_flags below), mean of --reps / 10 calls
  agree               share of systems whose four flags are the same in both (the torch version is float32 too; systems
                      within rounding of a threshold may differ)
  images              lattice images tried per pair (both versions)

    python tools/time_flag_anomaly.py [--systems 1000] [--atoms 200] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from adsorbdiff_amd import flag_anomaly as FA  # noqa: E402
from adsorbdiff_amd.engine import batch_pbc, cell_repeats  # noqa: E402
from adsorbdiff_amd.synthetic import make_batch  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_flags(pos0, pos1, Z, tags, cell, radii, reps, n, skin=0.3, s_mult=1.5, d_mult=1.5, chunk=125):
    """The contract of include/adsorbdiff_hip.h for B systems of n atoms each, in batched torch ops."""
    B = cell.shape[0]
    out = []
    shifts = torch.tensor([[a, b, c] for a in range(-reps[0], reps[0] + 1) for b in range(-reps[1], reps[1] + 1)
                           for c in range(-reps[2], reps[2] + 1)], dtype=torch.float32, device=pos0.device)
    zero = int((shifts.abs().sum(1) == 0).nonzero()[0])
    per = torch.tensor([r > 0 for r in reps], device=pos0.device)
    eye = torch.eye(n, dtype=torch.bool, device=pos0.device)
    for c0 in range(0, B, chunk):
        sl = slice(c0, min(B, c0 + chunk))
        cl = cell[sl]
        inv = torch.linalg.inv(cl)
        T = shifts @ cl                                           # [b, S, 3]
        R = radii[Z.view(B, n)[sl].long()]
        tg = tags.view(B, n)[sl]
        sumR = R[:, :, None] + R[:, None, :]

        def dmin(p):
            p = p.view(B, n, 3)[sl]
            d = p[:, None, :, :] - p[:, :, None, :]
            f = d @ inv[:, None]
            f = torch.where(per, f - torch.round(f), f)
            d = f @ cl[:, None]
            best = torch.full(d.shape[:3], float("inf"), device=d.device)
            for k in range(T.shape[1]):
                dist = (d + T[:, k, None, None, :]).norm(dim=-1)
                if k == zero:
                    dist = dist.masked_fill(eye, float("inf"))
                best = torch.minimum(best, dist)
            return best

        d0, d1 = dmin(pos0), dmin(pos1)
        ads, slab, frozen = tg == 2, tg != 2, tg == 0
        thr = lambda m: m * sumR + 2 * skin
        aa = ads[:, :, None] & ads[:, None, :]
        as_ = ads[:, :, None] & slab[:, None, :]
        af = ads[:, :, None] & frozen[:, None, :]
        ss = slab[:, :, None] & slab[:, None, :]
        dis = (((d0 < thr(1)) != (d1 < thr(1))) & aa).flatten(1).any(1)
        des = ~((d1 < thr(d_mult)) & as_).flatten(1).any(1)
        sur = ((((d1 < thr(1)) & ~(d0 < thr(s_mult))) | ((d0 < thr(1)) & ~(d1 < thr(s_mult)))) & ss).flatten(1).any(1)
        itc = ((d1 < thr(1)) & af).flatten(1).any(1)
        out.append(torch.stack([dis, des, sur, itc], 1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=1000)
    ap.add_argument("--atoms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    n_ads = 4
    b = make_batch(a.systems, n_slab=a.atoms - n_ads, n_ads=n_ads, seed=1).to(DEV)
    g = torch.Generator().manual_seed(2)
    final = b.pos + 0.1 * torch.randn(b.pos.shape, generator=g).to(DEV)
    lifted = (b.tags == 2) & (b.batch % 4 == 0)
    final[lifted, 2] += 4.5
    radii = np.random.default_rng(11).uniform(0.3, 1.6, size=119)
    radii_t = torch.tensor(radii, dtype=torch.float32, device=DEV)
    Z = b.atomic_numbers.long()
    reach = 1.5 * 2 * float(radii_t[Z].max()) + 0.6 + 0.01
    reps = cell_repeats(b.cell, reach, batch_pbc(b))
    flags = FA.flag_anomalies(b, final, radii=radii)
    ms = timed(lambda: FA.flag_anomalies(b, final, radii=radii), a.reps)
    cell = b.cell.reshape(-1, 3, 3).float()
    ref = torch_flags(b.pos, final, Z, b.tags, cell, radii_t, reps, a.atoms)
    ms_torch = timed(lambda: torch_flags(b.pos, final, Z, b.tags, cell, radii_t, reps, a.atoms), max(1, a.reps // 10))
    print(json.dumps({"systems": a.systems, "atoms": a.atoms, "images": (2 * reps[0] + 1) * (2 * reps[1] + 1) * (2 * reps[2] + 1),
                      "flag_anomalies_ms": round(ms, 4), "torch_ms": round(ms_torch, 3),
                      "agree": float((flags == ref).all(1).float().mean()),
                      "flagged": flags.float().mean(0).tolist()}))


if __name__ == "__main__":
    main()
