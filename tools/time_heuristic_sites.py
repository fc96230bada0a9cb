"""Timing of heuristic_sites on a batch of pristine slabs: --slabs slabs, fcc(111) 3x3x4, fcc(111) 2x2x3 and
fcc(100) 2x2x3 in turn, hand-built triangle tables (no scipy needed).  Prints one JSON line:

  heuristic_sites_ms     one heuristic_sites call with the slabs' symmetry handed in - candidates, both reduction passes and
                         the compaction of the site list - the mean of --reps calls after a warm-up
  with_find_symmetry_ms  the same with symmetry="auto": slab_symmetry.find_symmetry included
  identity_only_ms       the same with symmetry=None
  sites / candidates     sites returned and raw candidates of the batch
  oracle_ms_per_slab / oracle_slabs
                         the float64 numpy oracle of the contract (tests/helpers_heuristic_sites.sites, the operations
                         given) on every --subsample-th slab, and how many slabs it did
  agree                  the device's kept candidates, rep and multiplicity equal the oracle's on those slabs

Every measurement runs in a child process of its own under its own time limit; a measurement that fails or runs out of
time is reported as null.  A record, not a gate.

    python tools/time_heuristic_sites.py [--slabs 1000] [--reps 5] [--subsample 100] [--limit 240]
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
MIX = ("111_3x3x4", "111_2x2x3", "100_2x2x3")


def names(n):
    return [MIX[k % len(MIX)] for k in range(n)]


def child_device(a):
    import torch

    from adsorbdiff_amd import placement as PL
    from adsorbdiff_amd import slab_symmetry as SY
    from tests import helpers_heuristic_sites as H

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    ns = names(a.slabs)
    sb, tri = H.slab_batch(ns, DEV), H.triangles(ns)
    sym = SY.find_symmetry(sb)
    st = PL.heuristic_sites(sb, tri, symmetry=sym)
    out = {"sites": int(st.pos.shape[0]), "candidates": int(st.candidates.shape[0]),
           "heuristic_sites_ms": round(timed(lambda: PL.heuristic_sites(sb, tri, symmetry=sym)), 3),
           "with_find_symmetry_ms": round(timed(lambda: PL.heuristic_sites(sb, tri)), 3),
           "identity_only_ms": round(timed(lambda: PL.heuristic_sites(sb, tri, symmetry=None)), 3)}
    print(json.dumps(out))


def child_oracle(a):
    import numpy as np

    from adsorbdiff_amd import placement as PL
    from tests import helpers_heuristic_sites as H

    ns = names(a.slabs)
    st = PL.heuristic_sites(H.slab_batch(ns, DEV), H.triangles(ns))
    off = st.seg_offset.cpu().numpy().astype(np.int64)
    rep, mult, cand_of, slab = (t.cpu().numpy() for t in (st.rep, st.multiplicity, st.candidate, st.slab))
    picks = list(range(0, a.slabs, max(1, a.subsample)))
    agree, spent = True, 0.0
    for b in picks:
        case = H.case(ns[b])
        t0 = time.perf_counter()
        want = H.sites(case)
        spent += time.perf_counter() - t0
        c0, c1 = off[3 * b], off[3 * b + 3]
        got_rep = np.where(rep[c0:c1] >= 0, rep[c0:c1] - c0, -1)
        agree = agree and (got_rep == want["rep"]).all() and (cand_of[slab == b] - c0).tolist() == want["kept"].tolist() \
            and mult[slab == b].tolist() == want["multiplicity"][want["kept"]].tolist()
    print(json.dumps({"oracle_ms_per_slab": round(spent * 1e3 / len(picks), 3), "oracle_slabs": len(picks), "agree": bool(agree)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slabs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--subsample", type=int, default=100)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per measurement")
    ap.add_argument("--child", choices=("device", "oracle"))
    a = ap.parse_args()
    if a.child:
        return {"device": child_device, "oracle": child_oracle}[a.child](a)
    out = {"slabs": a.slabs, "mix": list(MIX)}
    keys = {"device": ("sites", "candidates", "heuristic_sites_ms", "with_find_symmetry_ms", "identity_only_ms"),
            "oracle": ("oracle_ms_per_slab", "oracle_slabs", "agree")}
    for kind in ("device", "oracle"):
        got = {}
        try:
            res = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", kind, "--slabs", str(a.slabs), "--reps",
                                  str(a.reps), "--subsample", str(a.subsample)], capture_output=True, text=True, timeout=a.limit,
                                 cwd=str(ROOT))
            if res.returncode == 0:
                got = json.loads(res.stdout.strip().splitlines()[-1])
            else:
                print(res.stderr[-2000:], file=sys.stderr)
        except subprocess.TimeoutExpired:
            print(f"{kind}: no result within {a.limit} s", file=sys.stderr)
        out.update({k: got.get(k) for k in keys[kind]})
        if not got:
            break                       # a measurement that failed on the device: nothing more is started on it
    print(json.dumps(out))


if __name__ == "__main__":
    main()
