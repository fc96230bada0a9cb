"""CPU tests of the heuristic site finder: the float64 oracle of tests/helpers_heuristic_sites.py against the
crystallographic known answers, its decision margins, the argument checks of the Python entry points and the registration
of csrc/sites.hip."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import build as BUILD
from adsorbdiff_amd import lib as L
from adsorbdiff_amd import placement as PL
from adsorbdiff_amd.slab_symmetry import SlabSymmetry
from tests import helpers_heuristic_sites as H


@pytest.mark.parametrize("name", list(H.TABLE))
def test_oracle_gives_the_known_site_counts(name):
    n_ops, want, identity = H.TABLE[name]
    case = H.case(name)
    assert len(case["ops"]) == n_ops
    res = H.oracle(name)                                  # asserts the margins
    assert H.site_counts(res) == want
    if identity is not None:
        assert H.site_counts(res, both=False) == identity
        alone = H.oracle(name, symmetric=False)
        assert H.site_counts(alone) == identity and H.site_counts(alone, both=False) == identity
    # every first-pass survivor is counted once
    kept = res["kept"]
    assert int(res["multiplicity"][kept].sum()) == sum(H.site_counts(res, both=False))
    assert (res["multiplicity"][np.setdiff1d(np.arange(len(res["rep"])), kept)] == 0).all()
    assert ((res["rep"] == -1) == ~res["valid"]).all() and (res["rep"][kept] == kept).all()


def test_oracle_multiplicities_and_layout_of_111_3x3x4():
    res = H.oracle("111_3x3x4")
    assert res["multiplicity"][res["kept"]].tolist() == [9, 27, 9, 9]
    assert res["kind"][res["kept"]].tolist() == [0, 1, 2, 2]
    T = len(H.case("111_3x3x4")["tri"])
    assert T == 50 and res["segments"] == [(0, 9), (9, 9 + 3 * T), (9 + 3 * T, 9 + 4 * T)]
    assert res["valid"].all()


def test_oracle_right_triangles_have_no_hollow():
    res = H.oracle("100_2x2x3")
    s0, s1 = res["segments"][2]
    assert not res["valid"][s0:s1].any() and (res["rep"][s0:s1] == -1).all()
    assert np.abs(res["cos"]).min() < 1e-6               # the right angle: below the band, so the decision is safe


@pytest.mark.parametrize("name", H.VARIANTS)
def test_variants_meet_the_margins(name):
    res = H.oracle(name)
    if name == "rattled":
        assert len(H.case(name)["ops"]) == 1 and H.site_counts(res) == H.site_counts(res, both=False) == (9, 27, 18)
    if name in ("two_species", "left_handed"):
        assert H.site_counts(res) == (1, 1, 2)


def test_margin_assertion_fires():
    with pytest.raises(AssertionError, match="pair distance"):
        H.assert_margins(dict(distances=np.array([0.0, 0.2, 3.0])))
    with pytest.raises(AssertionError, match="cosine"):
        H.assert_margins(dict(distances=np.zeros(0), cos=np.array([[0.5, 0.5, 5e-5]])))


def test_bridge_order_lists_edges_by_opposite_corner():
    c = H.case("111_1x1x3")
    tri = c["tri"][:1].copy()
    tri[0] = [[1, 1, 9], [2, 1, 9], [1.5, 1.8, 9]]       # well inside the cell: no wrap
    x, valid, kind, _ = H.candidates(c["pos"], c["tags"], c["cell"], tri)
    v = tri[0]
    assert np.allclose(x[1:4], [(v[1] + v[2]) / 2, (v[0] + v[2]) / 2, (v[0] + v[1]) / 2], atol=1e-6)
    assert np.allclose(x[4], v.mean(0), atol=1e-6) and kind.tolist() == [0, 1, 1, 1, 2] and valid.all()


# ------------------------------------------------------------------------------------------------ the Python entry points
def test_argument_checks_and_no_cpu_fallback():
    names = ["111_1x1x3", "100_2x2x3"]
    sb, tri = H.slab_batch(names), H.triangles(names)
    for bad in ((), ("ontop", "ontop"), ("top",), ("ontop", "fourfold")):
        with pytest.raises(ValueError, match="positions"):
            PL.heuristic_sites(sb, tri, symmetry=None, positions=bad)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            PL.heuristic_sites(sb, tri, symmetry=None, tol=bad)
    with pytest.raises(ValueError, match="1 triangle tables for 2 slabs"):
        PL.heuristic_sites(sb, tri[:1], symmetry=None)
    with pytest.raises(ValueError, match="symmetry"):
        PL.heuristic_sites(sb, tri, symmetry="spglib")
    with pytest.raises(ValueError, match="symmetry of 3 slabs"):
        PL.heuristic_sites(sb, tri, symmetry=SlabSymmetry.identity([1, 1, 1], "cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.heuristic_sites(sb, tri, symmetry=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.place_adsorbates_heuristic(sb, (np.array([8]), np.zeros((1, 3))), [0], radii=np.ones(100), masses=np.ones(100),
                                      triangles=tri, symmetry=None)


def test_mode_string_is_still_refused_and_names_the_new_entry():
    with pytest.raises(ValueError, match="place_adsorbates_heuristic"):
        PL.AdsorbatePlacer.place(None, None, None, None, mode="heuristic")
    with pytest.raises(ValueError):
        PL.place_adsorbates(None, None, 1, mode="heuristic")
    assert PL.SITE_KINDS == ("ontop", "bridge", "hollow") and "heuristic" not in PL.MODES


def test_surface_sites_are_sites():
    fields = PL.SurfaceSites._fields
    assert fields[:4] == PL.Sites._fields[:4]
    for f in ("kind", "multiplicity", "candidate", "candidates", "valid", "rep"):
        assert f in fields
    st = PL.SurfaceSites(*([torch.zeros(0)] * len(fields)))
    assert PL.AdsorbatePlacer._as_sites(None, H.slab_batch(["111_1x1x3"]), st) is st


def test_sites_hip_is_registered():
    assert "sites.hip" in BUILD.SOURCES and (BUILD.CSRC / "sites.hip").exists()
    for name in ("adf_surface_site_candidates", "adf_reduce_sites"):
        assert name in L.EXPORTS
    lib = L.load()
    assert len(lib.adf_surface_site_candidates.argtypes) == 14 and len(lib.adf_reduce_sites.argtypes) == 18
    # a null pointer is refused on the host, before anything is launched: this needs no device
    assert lib.adf_reduce_sites(None, None, None, None, None, 1, 1, 1, None, None, None, 0, 0.05, None, None, None, None,
                                None) == L.ADF_EINVAL
    assert b"null argument" in lib.adf_last_error()
    assert lib.adf_surface_site_candidates(None, None, None, None, None, None, 1, 1, 1, 1, None, None, None, None) == L.ADF_EINVAL
    assert b"null argument" in lib.adf_last_error()


def test_scipy_triangulation_gives_the_hand_table_sites():
    """Where scipy imports: the Delaunay table of ``surface_triangles`` on fcc(111) 3x3 reduces to the same sites as the hand
    table (the same positions, modulo the lattice), under the identity pass and under the slab's operations."""
    pytest.importorskip("scipy.spatial")
    name = "111_3x3x4"
    c = H.case(name)
    tri = PL.surface_triangles(H.slab_batch([name]))[0]
    got = H.sites(dict(c, tri=tri))
    H.assert_margins(got)
    want = H.oracle(name)
    assert H.site_counts(got) == H.site_counts(want) == (1, 1, 2)
    assert H.site_counts(got, both=False) == H.site_counts(want, both=False)
    # the identity-pass survivors are the same point set
    from tests.helpers_slab_symmetry import frame, reduce_norm
    M, Mi = frame(c["cell"])
    for kind in range(3):
        a = got["candidates"][[i for i in np.nonzero(got["first"] == np.arange(len(got["first"])))[0] if got["kind"][i] == kind]]
        b = want["candidates"][[i for i in np.nonzero(want["first"] == np.arange(len(want["first"])))[0] if want["kind"][i] == kind]]
        d = reduce_norm(a[:, None, :].astype(np.float64) - b[None, :, :].astype(np.float64), M, Mi)
        assert d.shape[0] == d.shape[1] and (d.min(1) < 1e-4).all() and (d.min(0) < 1e-4).all()
