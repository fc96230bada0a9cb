"""CPU tests of the placement contract: properties of the float64 oracle in tests/helpers_placement.py that
the device kernels are compared against, the closed-form height against the reference's fsolve formulation, the host
pieces of adsorbdiff_amd.placement (surface_triangles, argument checks) and its registration."""
import builtins
import math

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import placement as PL
from tests import helpers_placement as H

RADII, MASSES = H.synthetic_radii(), H.synthetic_masses()
SHAPES = [(1, 1), (30, 2), (63, 5), (200, 7), (17, 5), (90, 2)]   # (slab atoms, adsorbate atoms)
_CASES = {}


def cases(mode="random"):
    """Generated once per process: one slab per shape (the third is left-handed), 2 sites x 2 augmentations each."""
    if mode not in _CASES:
        rng = np.random.default_rng(21 if mode == "random" else 22)
        _CASES[mode] = [H.draw_case(rng, ns, na, RADII, MASSES, n_sites=2, n_aug=2, mode=mode, left_handed=(k == 2))
                        for k, (ns, na) in enumerate(SHAPES)]
    return _CASES[mode]


def test_registered_in_the_library():
    for name in ("adf_place_draws", "adf_place_adsorbates", "adf_place_site_candidates", "adf_interstitial_distances"):
        assert name in L.EXPORTS
    assert "placement.hip" in __import__("adsorbdiff_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("mode", ["random", "random_site_heuristic_placement"])
def test_placed_adsorbate_touches_at_exactly_the_gap(mode):
    """With a counted pair, the least dist - R_a - R_s over ALL pairs is the interstitial gap (to 1e-12); without one the
    adsorbate stays on the site."""
    seen = 0
    for c in cases(mode):
        for o in c["oracle"]:
            if o["n_combos"] > 0:
                got = H.min_gap_all_pairs(o, c["slab"]["Z"], c["ads"][0], RADII)
                assert abs(got - o["gap"]) <= 1e-12, (got, o["gap"])
                seen += 1
            else:
                assert o["scaled_normal"] == 0.0
    assert seen >= 12
    hole = H.hole_case(RADII, MASSES, np.random.default_rng(1))["oracle"][0]
    assert hole["n_combos"] == 0 and hole["scaled_normal"] == 0.0 and np.array_equal(hole["pos"][0], H.f32([7.0, 7.2, 5.0]))


def test_left_handed_cell_points_the_normal_down():
    c = cases()[2]
    assert H.normal(H.f32(c["slab"]["cell"]))[2] < 0 and all(o["n_combos"] > 0 for o in c["oracle"])
    assert all(o["n"][2] < 0 for o in c["oracle"])


def test_closed_form_height_against_the_reference_fsolve():
    """The reference solves fun(x) = 0 per counted pair with fsolve started at 3 d_min (restated in the helper).  fun is a
    parabola with its vertex at x = h: a start right of the vertex (h < 3 d_min) reaches the upper root, the contract's
    x_pair, and a start left of it the lower one - the deliberate reading stated in the header.  Pairs whose start is
    within 0.1 A of the vertex (zero slope) are left out; the bound on the others is 1e-9 A."""
    pytest.importorskip("scipy")
    upper = lower = 0
    worst = 0.0
    for mode in ("random", "random_site_heuristic_placement"):
        for c in cases(mode):
            for o in c["oracle"]:
                w = o["slab_c"][None] - o["ads_c"][:, None]
                h = w @ o["n"]
                q = np.linalg.norm(w - h[..., None] * o["n"], axis=-1)
                roots = H.fsolve_scaled_normal(o)
                best = -np.inf
                for a, s, x in roots:
                    rad = math.sqrt(o["D"][a, s] ** 2 - q[a, s] ** 2)
                    start = 3.0 * (o["D"][a, s] - o["gap"])
                    if start > h[a, s] + 0.1:
                        worst = max(worst, abs(x - (h[a, s] + rad)))
                        upper += 1
                    elif start < h[a, s] - 0.1:
                        assert abs(x - (h[a, s] - rad)) <= 1e-9
                        lower += 1
                    best = max(best, h[a, s] + rad)
                if roots:
                    assert best == o["scaled_normal"]
    print(f"closed form vs fsolve: {upper} upper-root pairs, worst {worst:.2e} A; {lower} lower-root pairs")
    assert upper > 100 and worst <= 1e-9, worst


def test_rotation_matrix_properties():
    rng = np.random.default_rng(3)
    for mode in ("random", "random_site_heuristic_placement"):
        for _ in range(200):
            u = rng.uniform(0, 1, 3)
            R, zrot, rv = H.rotation(*u, mode)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
            assert np.abs(R @ np.array([0.0, 0.0, 1.0]) - rv).max() < 1e-14
            assert abs(np.linalg.norm(rv) - 1.0) < 1e-14 and 0.0 <= zrot < 360.0
            if mode != "random":
                assert rv[2] >= math.cos(math.pi / 9)
    # both poles take the fallback axis x_hat x rotvec and stay proper rotations
    for u1, want in ((0.5 + 0.5 * (1 - 1e-16), 1.0), (0.0, -1.0)):
        R, _, rv = H.rotation(0.0, u1, 0.3, "random")
        assert rv[2] == want and np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
    # the z rotation is counter-clockwise about +z and comes first
    R, _, _ = H.rotation(0.25, 1.0 - 1e-17, 0.0, "random_site_heuristic_placement")
    assert np.abs(R @ np.array([1.0, 0.0, 0.0]) - np.array([0.0, 1.0, 0.0])).max() < 1e-7
    # a one-atom adsorbate is not rotated and reports zeros
    c = cases()[0]
    for o in c["oracle"]:
        assert np.array_equal(o["meta"], np.zeros(4)) and np.array_equal(o["rel"], np.zeros((1, 3)))


def test_candidate_counts_keep_rule_and_selection_order():
    for num_sites, T, want in ((1, 4, 1), (5, 4, 3), (100, 7, 29), (3, 50, 1), (8, 16, 1)):
        assert H.per_triangle(num_sites, T) == want
    cell = np.array([[8.0, 0.0, 0.0], [3.0, 7.0, 0.0], [0.2, 0.1, 24.0]])
    frac = np.array([[0.5, 0.5, 0.3], [0.0, 0.0, 0.3], [-2e-7, 0.5, 0.3], [0.5, 1.0 - 0.5e-7, 0.3], [0.5, 1.0 - 2e-7, 0.3],
                     [1.2, 0.5, 0.3], [0.5, -0.3, 0.3], [0.999, 0.001, 5.0], [0.5, 0.5, -4.0]])
    keep, _ = H.keep_rule(frac @ cell, cell)
    assert keep.tolist() == [True, True, False, False, True, False, False, True, True]   # c is not periodic for a site
    tri = H.lattice_triangles(cell, 2, 9.0)
    assert tri.shape == (2 * 4 * 4, 3, 3)
    per = H.per_triangle(5, len(tri))
    rows = H.candidate_rows(np.random.default_rng(5), tri, per, cell)
    cand, keep, margin = H.candidates_oracle(tri, per, cell, rows)
    assert cand.shape == (len(tri) * per, 3) and margin >= H.MIN_SEAM_MARGIN and 0 < keep.sum() < len(keep)
    # every candidate lies in its own triangle's plane patch: barycentric weights in [0, 1]
    sel = H.select_oracle(keep, rows[:, 2], 5)
    assert len(sel) == 5 and keep[sel].all() and np.all(np.diff(rows[sel, 2]) >= 0)
    assert rows[sel, 2].max() <= np.sort(rows[keep, 2])[4]
    assert len(H.select_oracle(keep, rows[:, 2], 10 ** 6)) == keep.sum()          # fewer kept than asked: a shorter result
    ties = H.select_oracle(np.array([True, True, False, True]), np.array([0.5, 0.5, 0.1, 0.2]), 3)
    assert ties.tolist() == [3, 0, 1]


def test_surface_triangles_on_a_rectangular_lattice():
    pytest.importorskip("scipy")
    a, b = 2.7, 3.1
    surf = np.array([[i * a, j * b, 9.0] for i in range(3) for j in range(2)])
    below = surf + np.array([0.5 * a, 0.5 * b, -2.0])
    cell = np.array([[3 * a, 0.0, 0.0], [0.0, 2 * b, 0.0], [0.0, 0.0, 25.0]])
    slab = dict(pos=np.concatenate([below, surf]), Z=np.full(12, 29), tags=np.array([0] * 6 + [1] * 6), fixed=np.array([1] * 6 + [0] * 6),
                cell=cell)
    (tri,) = PL.surface_triangles(H.slab_batch([slab]))
    assert tri.ndim == 3 and tri.shape[1:] == (3, 3) and len(tri) >= 12
    surf32 = H.f32(surf)
    tiled = {tuple(np.round(p + i * H.f32(cell[0]) + j * H.f32(cell[1]), 4)) for p in surf32 for i in (-1, 0, 1) for j in (-1, 0, 1)}
    central = {tuple(np.round(p, 4)) for p in surf32}
    for t in tri:
        vs = [tuple(np.round(v, 4)) for v in t]
        assert all(v in tiled for v in vs)
        assert any(v in central for v in vs)
    assert np.array_equal(PL.tiling_vectors(cell), cell[:2])
    # a slab without three surface atoms has no triangle
    slab["tags"] = np.array([0] * 12)
    with pytest.raises(ValueError, match="no surface triangle"):
        PL.surface_triangles(H.slab_batch([slab]))


def test_errors(monkeypatch):
    real = builtins.__import__

    def no_ase(name, *a, **kw):
        if name == "ase" or name.startswith("ase."):
            raise ImportError("No module named 'ase'")
        return real(name, *a, **kw)

    c = cases()[1]
    sb = H.slab_batch([c["slab"]])
    monkeypatch.setattr(builtins, "__import__", no_ase)
    with pytest.raises(ImportError, match="radii="):
        PL.AdsorbatePlacer()
    with pytest.raises(ImportError, match="masses="):
        PL.AdsorbatePlacer(radii=RADII)
    with pytest.raises(ImportError, match="radii="):           # before anything touches a device
        PL.interstitial_distances(sb)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.AdsorbatePlacer(RADII, MASSES, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.interstitial_distances(sb, RADII, MASSES)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.place_adsorbates(sb, c["ads"], 2, radii=RADII, masses=MASSES)
    for bad in (dict(mode="heuristic"), dict(mode="bogus"), dict(interstitial_gap=5.0), dict(interstitial_gap=-0.1)):
        with pytest.raises(ValueError):
            PL.place_adsorbates(sb, c["ads"], 2, radii=RADII, masses=MASSES, **bad)
    assert not any(isinstance(v, (list, tuple, np.ndarray)) and len(v) > 20 for v in vars(PL).values())   # no table lives here


def test_surface_triangles_without_scipy_says_what_to_pass(monkeypatch):
    real = builtins.__import__

    def no_scipy(name, *a, **kw):
        if name == "scipy" or name.startswith("scipy."):
            raise ImportError("No module named 'scipy'")
        return real(name, *a, **kw)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(ImportError, match="triangles="):
        PL.surface_triangles(H.slab_batch([cases()[1]["slab"]]))
