"""Timing of the surface tags on --slabs copies of the 35-atom vacancy slab of tests/helpers_voronoi.py
(fcc(111) 3x3x4 without one top atom).  Prints one JSON line:

  tag_ms          one tag_surface_atoms call with the fcc bulk table (9 atoms per slab get their Voronoi cell), device events,
                  the mean of --reps calls after one warm-up
  voronoi_ms      one voronoi_coordination call on all atoms of the same batch (17 of 35 cells per slab are open and run
                  through all of their candidates)
  tags_per_slab   atoms of tag 1 per slab (11), the same for every copy

The host figure to set beside it is ``python tools/make_golden_voronoi.py --time N`` (the qhull loop; needs scipy).  The
measurement runs in a child process under its own time limit.  A record, not a gate.

    python tools/time_surface_tags.py [--slabs 1000] [--reps 3] [--limit 240]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEV = "cuda:0"


def device_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def child(a):
    import torch

    from adsorbdiff_amd import surface_tags as ST
    from tests import helpers_voronoi as H

    sb = H.batch_of([H.case("111_3x3x4_vacancy")] * a.slabs, DEV)
    table = torch.from_numpy(H.fcc_bulk_row())[None].expand(a.slabs, 119).contiguous().to(DEV)
    m = H.synthetic_masses()
    out = ST.tag_surface_atoms(sb, bulk=table, masses=m)
    per = out.tags.view(a.slabs, 35).sum(1)
    assert int(per.min()) == int(per.max())
    print(json.dumps({"atoms": int(sb.pos.shape[0]), "tags_per_slab": int(per[0]),
                      "tag_ms": round(device_ms(lambda: ST.tag_surface_atoms(sb, bulk=table, masses=m), a.reps), 3),
                      "voronoi_ms": round(device_ms(lambda: ST.voronoi_coordination(sb), a.reps), 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slabs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds for the measurement")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"slabs": a.slabs, "atoms": None, "tags_per_slab": None, "tag_ms": None, "voronoi_ms": None}
    try:
        res = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--slabs", str(a.slabs), "--reps",
                              str(a.reps)], capture_output=True, text=True, timeout=a.limit, cwd=str(ROOT))
        if res.returncode == 0:
            out.update(json.loads(res.stdout.strip().splitlines()[-1]))
        else:
            print(res.stderr[-2000:], file=sys.stderr)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.limit} s", file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
