"""Host tests of the device triangulation (csrc/triangulate.hip, placement.surface_triangles_device): the
float64 oracle of tests/helpers_surface_triangles.py against the recorded scipy tables, the fixture against scipy where it
imports, the oracle's margins, the registration of the entry and the argument checks that need no device."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import build as BUILD
from adsorbdiff_amd import lib as L
from adsorbdiff_amd import placement as PL
from tests import helpers_surface_triangles as H


# ------------------------------------------------------------------------------------------------ oracle and fixture
@pytest.mark.parametrize("key,which", H.FIXTURE_CASES)
def test_oracle_equals_the_recorded_scipy_table(key, which):
    fx = H.load_fixture()[H.fixture_name(key, which)]
    case = H.fixture_case(key, which)
    for f in ("pos", "Z", "cell", "tags"):
        assert fx[f].dtype == np.asarray(case[f]).dtype and (fx[f] == case[f]).all(), f     # the builders give the recorded inputs
    xy, n_top, res = H.oracle(key, which)
    H.assert_margins(res)
    strict = H.rows_of(res, "strict", xy)
    assert strict.shape == fx["index"].shape and (strict == fx["index"]).all()
    assert (H.rows_of(res, "admissible", xy) == strict).all()          # no tie: the triangulation is unique
    assert (H.expected(xy, n_top, res=res) == strict).all()            # and the fan rule has nothing to split
    H.check_table(xy, n_top, fx["index"])
    pts, _ = H.tiled_points(case["pos"], case["tags"], case["cell"])
    assert fx["vertices"].dtype == np.float32 and (fx["vertices"] == pts[fx["index"]].astype(np.float32)).all()


def test_fixture_holds_the_counts_checked_for_this_kind_of_input():
    fx = H.load_fixture()
    assert [len(fx[n]["index"]) for n in ("generic3_0", "generic3_1", "generic3_2", "111_3x3x4")] == [6, 19, 30, 30]
    assert [int((fx[n]["tags"] == 1).sum()) for n in ("generic3_0", "generic3_1", "generic3_2")] == [1, 5, 9]
    # one cell is skewed, one has the row tiling_vectors skips in front
    assert fx["generic3_0"]["cell"][1, 0] != 0 and (fx["generic3_1"]["cell"][0, :2] == 0).all()
    assert (PL.tiling_vectors(fx["generic3_1"]["cell"]) == fx["generic3_1"]["cell"][1:]).all()


def test_fixture_regenerates_where_scipy_imports():
    pytest.importorskip("scipy.spatial")
    fx = H.load_fixture()
    for key, which in H.FIXTURE_CASES:
        index, vertices = H.scipy_rows(H.fixture_case(key, which))
        got = fx[H.fixture_name(key, which)]
        assert index.shape == got["index"].shape and (index == got["index"]).all()
        assert vertices.dtype == got["vertices"].dtype and (vertices == got["vertices"]).all()


@pytest.mark.parametrize("name", H.DEGENERATE)
def test_oracle_on_the_degenerate_lattices(name):
    """Perfect rectangles: no strict triangle, two admissible ones per diagonal, and the fan rule picks parallel diagonals."""
    xy, n_top, res = H.oracle(name)
    assert not res["strict"].any() and res["admissible"].any()
    want = H.expected(xy, n_top, res=res)
    H.check_table(xy, n_top, want)
    admissible = {tuple(t) for t in H.rows_of(res, "admissible", xy)}
    assert all(tuple(t) in admissible for t in want) and len(want) < len(admissible)
    d = H.longest_edge_directions(xy, want)
    assert np.abs(d - d[0]).max() < 1e-6


def test_margin_assertion_fires_on_a_doctored_input():
    case = dict(H.generic3()[2])
    pts, n_top = H.tiled_points(case["pos"], case["tags"], case["cell"])
    xy = pts[:, :2].copy()
    res = H.triples(xy, n_top)
    H.assert_margins(res)
    # move a point onto a neighbouring triangle's circle, 3 circle_tol outside it
    m = int(np.nonzero(res["strict"])[0][0])
    q = int(np.argmin(np.where(np.isfinite(res["signed"][m]), res["signed"][m], np.inf)))
    out = xy[q] - res["centre"][m]
    xy[q] = res["centre"][m] + out / np.linalg.norm(out) * (res["r"][m] + 3 * H.CIRCLE_TOL)
    with pytest.raises(AssertionError, match="factor of ten"):
        H.assert_margins(H.triples(xy, n_top))


def test_hex_count_is_the_brute_force_count():
    for name, p in (("111_2x2x3", 2), ("111_3x3x4", 3)):
        xy, n_top, res = H.oracle(name)
        assert int(res["strict"].sum()) == H.hex_count(p)
    assert H.hex_count(7) == 2 * 49 + 28


# ------------------------------------------------------------------------------------------------ registration
def test_triangulate_hip_is_registered():
    assert "triangulate.hip" in BUILD.SOURCES and (BUILD.CSRC / "triangulate.hip").exists()
    assert "adf_surface_triangles" in L.EXPORTS
    header = (BUILD.PKG.parent / "include" / "adsorbdiff_hip.h").read_text()
    assert "int32_t adf_surface_triangles(" in header and "circle_tol" in header
    lib = L.load()
    assert len(lib.adf_surface_triangles.argtypes) == 12
    # refused on the host, before anything is launched: this needs no device
    assert lib.adf_surface_triangles(None, None, None, None, 1, 1, 1e-4, 18, None, None, None, None) == L.ADF_EINVAL
    assert b"null argument" in lib.adf_last_error()


# ------------------------------------------------------------------------------------------------ the Python entry points
def test_argument_checks_and_no_cpu_fallback():
    sb = H.batch_of(H.generic3())
    placer = PL.AdsorbatePlacer.__new__(PL.AdsorbatePlacer)
    placer.dev = torch.device("cpu")
    for call in (lambda t: PL.heuristic_sites(sb, t, symmetry=None), lambda t: placer.sites(sb, 2, triangles=t),
                 lambda t: placer.heuristic_sites(sb, t, symmetry=None)):
        with pytest.raises(ValueError, match="triangles = 'scipy'"):
            call("scipy")
        other = PL.SurfaceTriangles(torch.zeros(4, 3, 3), torch.tensor([0, 2, 4], dtype=torch.int32),
                                    torch.zeros(4, 3, dtype=torch.int32), [2, 2])
        with pytest.raises(ValueError, match="SurfaceTriangles of 2 slabs for a batch of 3"):
            call(other)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call("device")
    for bad in (-1e-4, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="circle_tol"):
            PL.surface_triangles_device(sb, circle_tol=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.surface_triangles_device(sb)
    assert PL._one_slab_triangles("device") == "device" and PL._one_slab_triangles(None) is None
    one = np.zeros((2, 3, 3))
    assert PL._one_slab_triangles(one)[0] is one


def test_surface_triangles_to_list_is_the_host_form():
    tri = torch.arange(5 * 9, dtype=torch.float32).reshape(5, 3, 3)
    st = PL.SurfaceTriangles(tri, torch.tensor([0, 2, 5], dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int32), [2, 3])
    a, b = st.to_list()
    assert a.dtype == np.float64 and a.shape == (2, 3, 3) and b.shape == (3, 3, 3)
    assert (np.concatenate([a, b]) == tri.numpy()).all()
    assert PL.SurfaceTriangles._fields == ("tri", "tri_offset", "index", "counts")
