"""Timing of the surface triangulation: placement.surface_triangles - scipy.spatial.Delaunay in a Python loop
over the slabs, on the host - against placement.surface_triangles_device, on the same box.  Prints one JSON line:

  slabs / surface_atoms  --slabs slabs of 16 tag-1 atoms (a 4 x 4 square surface, 0.15 A in-plane jitter) over a lower layer
  host_ms                one surface_triangles call on the batch (host; the batch's arrays are read back inside it)
  device_ms              one surface_triangles_device call - five launches and the one host read - the mean of --reps calls
                         after a warm-up
  same_set / tied / tied_admissible
                         slabs whose device triangles are scipy's as a set of index triples (every slab is compared); the
                         others - random jitter leaves a few quadrilaterals co-circular within circle_tol, which the contract
                         splits by its fan rule and scipy by the sign of an exact determinant - and whether on each of those the
                         float64 oracle (tests/helpers_surface_triangles.py) finds ties and every device triangle admissible
  large_host_ms / large_device_ms / large_triangles
                         the same pair on the one 342-surface-atom slab of tests/helpers_slab_symmetry.LARGE_SLAB
  sites_host_ms / sites_device_ms
                         heuristic_sites end to end on the --slabs batch with triangles=None (scipy, re-packed and uploaded)
                         and with triangles="device", symmetry=None in both

Every measurement runs in a child process of its own under its own time limit; a measurement that fails or runs out of
time is reported as null and nothing more is started.  A record, not a gate.

    python tools/time_surface_triangles.py [--slabs 1000] [--reps 5] [--limit 240]
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


def jittered(n, seed=7):
    import numpy as np

    from tests import helpers_surface_triangles as H

    rng = np.random.default_rng(seed)
    grid = np.array([[i * 2.7, j * 2.7] for i in range(4) for j in range(4)]) + 0.4
    cell = [[10.8, 0.0, 0.0], [0.0, 10.8, 0.0], [0.0, 0.0, 22.0]]
    return [H._slab(grid + rng.uniform(-0.15, 0.15, size=(16, 2)), cell) for _ in range(n)]


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


def host_ms(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def same_sets(st, host, cases):
    import numpy as np

    from tests import helpers_surface_triangles as H

    off = st.tri_offset.cpu().numpy()
    index = st.index.cpu().numpy()
    same, tied, admissible = 0, 0, True
    for b, c in enumerate(cases):
        pts, n_top = H.tiled_points(c["pos"], c["tags"], c["cell"])
        look = {tuple(p): k for k, p in enumerate(pts)}
        want = {tuple(sorted(look[tuple(v)] for v in t)) for t in host[b]}
        got = {tuple(sorted(t)) for t in index[off[b]:off[b + 1]].tolist()}
        if got == want:
            same += 1
            continue
        tied += 1
        res = H.triples(pts[:, :2], n_top)
        ok = {tuple(sorted(t)) for t in res["index"][res["admissible"]].tolist()}
        admissible = admissible and bool(res["admissible"].sum() > res["strict"].sum()) and got <= ok and len(got) == len(want)
    return {"same_set": same, "tied": tied, "tied_admissible": admissible if tied else None}


def child_batch(a):
    from adsorbdiff_amd import placement as PL
    from tests import helpers_surface_triangles as H

    cases = jittered(a.slabs)
    sb = H.batch_of(cases, DEV)
    st = PL.surface_triangles_device(sb)
    t_host, host = host_ms(lambda: PL.surface_triangles(sb))
    print(json.dumps({"surface_atoms": 16, "triangles": int(st.tri.shape[0]), "host_ms": round(t_host, 3),
                      "device_ms": round(device_ms(lambda: PL.surface_triangles_device(sb), a.reps), 3),
                      **same_sets(st, host, cases)}))


def child_large(a):
    import numpy as np

    from adsorbdiff_amd import placement as PL
    from tests import helpers_heuristic_sites as HH
    from tests import helpers_slab_symmetry as HS
    from tests import helpers_surface_triangles as H

    c = H.lattice(HS.LARGE_SLAB[0])
    assert int((np.asarray(c["tags"]) == 1).sum()) == HS.LARGE_SLAB[2]
    sb = HH.slab_batch([HS.LARGE_SLAB[0]], DEV)
    st = PL.surface_triangles_device(sb)
    t_host, host = host_ms(lambda: PL.surface_triangles(sb))
    print(json.dumps({"large_triangles": int(st.tri.shape[0]), "large_host_ms": round(t_host, 3),
                      "large_device_ms": round(device_ms(lambda: PL.surface_triangles_device(sb), a.reps), 3),
                      "large_same_set": same_sets(st, host, [c])["same_set"] == 1}))


def child_sites(a):
    from adsorbdiff_amd import placement as PL
    from tests import helpers_surface_triangles as H

    sb = H.batch_of(jittered(a.slabs), DEV)
    PL.heuristic_sites(sb, "device", symmetry=None)                   # warm-up of both
    t_host, _ = host_ms(lambda: PL.heuristic_sites(sb, None, symmetry=None))
    print(json.dumps({"sites_host_ms": round(t_host, 3),
                      "sites_device_ms": round(device_ms(lambda: PL.heuristic_sites(sb, "device", symmetry=None), a.reps), 3)}))


CHILDREN = {"batch": (child_batch, ("surface_atoms", "triangles", "host_ms", "device_ms", "same_set", "tied", "tied_admissible")),
            "large": (child_large, ("large_triangles", "large_host_ms", "large_device_ms", "large_same_set")),
            "sites": (child_sites, ("sites_host_ms", "sites_device_ms"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slabs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per measurement")
    ap.add_argument("--child", choices=tuple(CHILDREN))
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child][0](a)
    out = {"slabs": a.slabs}
    for kind, (_, keys) in CHILDREN.items():
        got = {}
        try:
            res = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", kind, "--slabs", str(a.slabs), "--reps",
                                  str(a.reps)], capture_output=True, text=True, timeout=a.limit, cwd=str(ROOT))
            if res.returncode == 0:
                got = json.loads(res.stdout.strip().splitlines()[-1])
            else:
                print(res.stderr[-2000:], file=sys.stderr)
        except subprocess.TimeoutExpired:
            print(f"{kind}: no result within {a.limit} s", file=sys.stderr)
        out.update({k: got.get(k) for k in keys})
        if not got:
            break                       # a measurement that failed on the device: nothing more is started on it
    print(json.dumps(out))


if __name__ == "__main__":
    main()
