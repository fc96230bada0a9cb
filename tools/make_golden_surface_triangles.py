"""Writes tests/golden/surface_triangles.npz: what scipy.spatial.Delaunay, through placement.surface_triangles, keeps for
the cases of tests/helpers_surface_triangles.py whose triangulation is unique - the three slabs of ``generic3`` and the
perfect fcc(111) 3x3x4 - so that the GPU tests of the device triangulation need no scipy.

Per case: the inputs (pos float32, Z, cell float32, tags), ``index`` [T,3] int64 - scipy's kept triangles as canonical rows
(the least tiled index first, counter-clockwise, ascending) - and ``vertices`` [T,3,3] float32: the rows of
``surface_triangles`` in that order, ``.astype(float32)``.  Before anything is written the generator asserts the margins
of every case (no point within a factor of ten of circle_tol off a circumcircle that decides) and that scipy's set equals
the float64 oracle's strict set.  Plain recorded data, a few KB.  Needs scipy; no GPU.

    python tools/make_golden_surface_triangles.py [--check]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import helpers_surface_triangles as H  # noqa: E402


def make():
    out = {}
    for key, which in H.FIXTURE_CASES:
        case = H.fixture_case(key, which)
        xy, n_top, res = H.oracle(key, which)
        H.assert_margins(res)
        strict = H.rows_of(res, "strict", xy)
        index, vertices = H.scipy_rows(case)
        assert index.shape == strict.shape and (index == strict).all(), f"{key} {which}: scipy's set is not the oracle's strict set"
        assert (H.rows_of(res, "admissible", xy) == strict).all(), f"{key} {which}: a tie"
        name = H.fixture_name(key, which)
        for field in ("pos", "Z", "cell", "tags"):
            out[f"{name}__{field}"] = np.asarray(case[field])
        out[f"{name}__index"], out[f"{name}__vertices"] = index, vertices
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the file instead of writing it")
    a = ap.parse_args()
    out = make()
    if a.check:
        with np.load(H.GOLDEN) as z:
            assert sorted(z.files) == sorted(out), "the file holds other arrays"
            for k, v in out.items():
                assert z[k].dtype == v.dtype and z[k].shape == v.shape and (z[k] == v).all(), k
        print("equal:", H.GOLDEN)
        return
    H.GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(H.GOLDEN, **out)
    print(H.GOLDEN, H.GOLDEN.stat().st_size, "bytes;", {k: v.shape for k, v in out.items() if k.endswith("__index")})


if __name__ == "__main__":
    main()
