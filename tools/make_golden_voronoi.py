"""Writes tests/golden/voronoi_cn.npz: what ``scipy.spatial.Voronoi`` (qhull, which pymatgen's ``VoronoiNN`` calls) gives for
the cases of tests/helpers_voronoi.py, so that the tests of the surface tags need no scipy on the GPU machine.

Per case: the inputs (pos float32, Z, cell float32, select) and per selected atom ``cn``, ``omega_max``, ``nn`` and ``open``.  For atom i the
point set is the origin and the candidates of the contract (``helpers_voronoi.candidates``); a ridge of the origin with a
vertex at infinity makes the atom open (NaN, NaN, 0); otherwise every ridge's vertices are ordered around the ridge, its
solid angle is the fan of Van Oosterom and Strackee, and ``cn`` is ``get_cn(use_weights=True)`` with tol 0.1.  Before anything
is written the generator asserts the margins of every case and that the float64 oracle agrees to 1e-9.  Plain recorded
data, a few KB.  Needs scipy; no GPU.

    python tools/make_golden_voronoi.py [--check] [--time N]

``--time N``: the wall time of this qhull loop over N copies of the 35-atom vacancy slab, all atoms.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import helpers_voronoi as H  # noqa: E402


def qhull_atom(D, tol=H.WEIGHT_TOL):
    """(cn, omega_max, nn, open) of the origin among the candidates D [m,3]."""
    from scipy.spatial import Voronoi

    if len(D) < 4:
        return np.nan, np.nan, 0, True
    vor = Voronoi(np.vstack([np.zeros(3), D]))
    omega = np.zeros(len(D))
    for (p, q), verts in zip(vor.ridge_points, vor.ridge_vertices):
        if 0 not in (p, q):
            continue
        j = (q if p == 0 else p) - 1
        if -1 in verts:
            return np.nan, np.nan, 0, True
        V = vor.vertices[verts]
        n, c = D[j] / np.linalg.norm(D[j]), V.mean(0)
        u = np.cross(n, [1, 0, 0] if abs(n[0]) < 0.9 else [0, 1, 0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        V = V[np.argsort(np.arctan2((V - c) @ v, (V - c) @ u))]
        omega[j] = H._fan(V)
    w = omega / omega.max()
    return float(w[w > tol].sum()), float(omega.max()), int((w > tol).sum()), False


def qhull_case(c, atoms=None):
    rows = [qhull_atom(H.candidates(c["pos"], c["cell"], i)) for i in (range(len(c["Z"])) if atoms is None else atoms)]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], np.int64),
            np.array([r[3] for r in rows], bool))


def make():
    H.assert_margins()
    out, worst = {}, 0.0
    for name in H.CASES:
        c = H.case(name)
        cn, om, nn, op = qhull_case(c, H.selected(name))
        ocn, oom, onn, oop = H.oracle_arrays(name)
        assert (op == oop).all() and (nn == onn).all(), f"{name}: the oracle and qhull differ in nn or open"
        if (~op).any():
            worst = max(worst, np.abs(cn - ocn)[~op].max(), np.abs(om - oom)[~op].max())
        for field in ("pos", "Z", "cell"):
            out[f"{name}__{field}"] = np.asarray(c[field])
        out[f"{name}__select"] = H.select_mask(name)
        out[f"{name}__cn"], out[f"{name}__omega_max"], out[f"{name}__nn"], out[f"{name}__open"] = cn, om, nn, op
    assert worst < H.ATOL, worst
    print(f"oracle against qhull, cn and omega_max: {worst:.2e} at worst")
    thin = out["111_2x2x3_thin_gap__open"]
    assert not thin.any(), "the thin-gap slab has open cells: shrink the gap"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the file instead of writing it")
    ap.add_argument("--time", type=int, default=0, metavar="N")
    a = ap.parse_args()
    if a.time:
        c = H.case("111_3x3x4_vacancy")
        t0 = time.perf_counter()
        qhull_case(c)
        one = time.perf_counter() - t0
        print(f"qhull loop, one 35-atom slab: {one:.3f} s; {a.time} slabs: {one * a.time:.1f} s (one measured, scaled)")
        return
    out = make()
    if a.check:
        with np.load(H.GOLDEN) as z:
            assert sorted(z.files) == sorted(out), "the file holds other arrays"
            for k, v in out.items():
                assert z[k].dtype == v.dtype and z[k].shape == v.shape and np.array_equal(z[k], v, equal_nan=v.dtype.kind == "f"), k
        print("equal:", H.GOLDEN)
        return
    H.GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(H.GOLDEN, **out)
    print(H.GOLDEN, H.GOLDEN.stat().st_size, "bytes;", sum(len(v) for k, v in out.items() if k.endswith("__Z")), "atoms")


if __name__ == "__main__":
    main()
