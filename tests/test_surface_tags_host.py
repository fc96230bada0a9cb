"""CPU tests of the surface tags: the float64 oracle of tests/helpers_voronoi.py against what qhull gave for
the same points (tests/golden/voronoi_cn.npz), the oracle's tags on the table of the tests, ``tile_atoms`` on CPU tensors,
the registration of csrc/voronoi.hip and the argument checks of adsorbdiff_amd/surface_tags.py."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import build as BUILD
from adsorbdiff_amd import lib as L
from adsorbdiff_amd import surface_tags as ST
from tests import helpers_voronoi as H


# ------------------------------------------------------------------------------------------------ the oracle
def test_margins_hold_for_every_input_of_the_tests():
    H.assert_margins()


@pytest.mark.parametrize("name", list(H.CASES))
def test_oracle_equals_qhull(name):
    fx = H.load_fixture()[name]
    c = H.case(name)
    assert all((fx[k] == c[k]).all() and fx[k].dtype == c[k].dtype for k in ("pos", "Z", "cell"))
    assert (fx["select"] == H.select_mask(name)).all()
    cn, om, nn, op = H.oracle_arrays(name)
    assert (op == fx["open"]).all() and (nn == fx["nn"]).all()
    assert np.isnan(fx["cn"][op]).all() and (fx["nn"][op] == 0).all()
    print(name, "cn", np.abs(cn - fx["cn"])[~op].max(initial=0.0), "omega_max", np.abs(om - fx["omega_max"])[~op].max(initial=0.0))
    assert np.abs(cn - fx["cn"])[~op].max(initial=0.0) < H.ATOL
    assert np.abs(om - fx["omega_max"])[~op].max(initial=0.0) < H.ATOL


def test_known_coordination_numbers():
    fx = H.load_fixture()
    assert abs(fx["fcc_primitive"]["cn"][0] - 12.0) < 1e-4 and fx["fcc_primitive"]["nn"][0] == 12
    assert abs(fx["bcc_primitive"]["cn"][0] - 10.16061) < 1e-5 and fx["bcc_primitive"]["nn"][0] == 14
    assert len(np.unique(np.round(fx["fcc4_rattled"]["cn"], 6))) == 4
    assert fx["alone"]["open"].all() and not fx["111_2x2x3_thin_gap"]["open"].any()
    vac = fx["111_3x3x4_vacancy"]
    assert int((np.abs(vac["cn"] - 9.6) < 1e-3).sum()) == 3


def test_float32_positions_put_full_coordination_on_the_knife_of_round_5():
    """Why the contract compares cn < minimum - cn_tol: the reference's round(cn, 5) < 12 would split these atoms."""
    cn = H.load_fixture()["111_3x3x4"]["cn"]
    full = cn[np.abs(cn - 12.0) < 1e-3]
    assert len(full) == 18 and (full < 12.0).any() and np.abs(full - 12.0).max() < 1e-4


@pytest.mark.parametrize("name,bulk,height,count", H.TAG_TABLE)
def test_oracle_tags_on_the_table(name, bulk, height, count):
    res = H.tags_of(name, H.fcc_bulk_row() if bulk else None, height)
    tags, layer = res["tags"], H.layer_of(name)
    assert int(tags.sum()) == count
    assert (tags[layer == layer.max()] == 0).all()                    # the bottom layer: open cells, below the centre of mass
    if name == "111_3x3x4_vacancy" and bulk:
        assert (layer[tags == 1] <= 1).all() and int((tags[layer == 1]).sum()) == 3
        cn = np.array([H.oracle(name)[i]["cn"] for i in np.nonzero((tags == 1) & (layer == 1))[0]])
        assert np.abs(cn - 9.6).max() < 1e-3
    elif name == "110_2x2x6" and (bulk or height == 2.0):
        assert (tags == (layer <= 1)).all()
    else:
        assert (tags == (layer == 0)).all()


# ------------------------------------------------------------------------------------------------ tile_atoms
def test_tile_atoms_counts_order_and_cell():
    cases = [H.case("111_2x2x3_thin_gap"), H.case("fcc4_rattled"), H.case("111_3x3x4")]
    sb = H.batch_of(cases)
    sb.tags = torch.arange(sb.pos.shape[0]) % 2
    sb.surface_cn = torch.arange(sb.pos.shape[0], dtype=torch.float64)
    before = sb.pos.clone()
    out = ST.tile_atoms(sb, min_ab=8.0)
    assert torch.equal(sb.pos, before) and sb.natoms.tolist() == [12, 4, 36]
    want = []
    for c in cases:
        cell = c["cell"].astype(np.float64)
        want.append((int(np.ceil(8.0 / np.linalg.norm(cell[0]))), int(np.ceil(8.0 / np.linalg.norm(cell[1])))))
    assert want == [(2, 2), (3, 3), (1, 1)]
    assert out.natoms.tolist() == [12 * 4, 4 * 9, 36] and out.pos.shape[0] == 48 + 36 + 36
    assert out.batch.tolist() == [0] * 48 + [1] * 36 + [2] * 36 and out.sid == sb.sid
    start = 0
    for b, (c, (na, nb)) in enumerate(zip(cases, want)):
        n = len(c["Z"])
        cell = torch.from_numpy(c["cell"])
        for i in range(na):
            for j in range(nb):
                rows = slice(start, start + n)                          # image-major, the a index outer
                shift = float(i) * cell[0] + float(j) * cell[1]
                assert torch.allclose(out.pos[rows], torch.from_numpy(c["pos"]) + shift, atol=1e-5)
                assert out.atomic_numbers[rows].tolist() == c["Z"].tolist()
                first = int(sb.natoms[:b].sum())
                assert out.tags[rows].tolist() == sb.tags[first:first + n].tolist()
                assert out.surface_cn[rows].tolist() == sb.surface_cn[first:first + n].tolist()
                start += n
        assert torch.equal(out.cell[b, 0], cell[0] * na) and torch.equal(out.cell[b, 1], cell[1] * nb)
        assert torch.equal(out.cell[b, 2], cell[2])
    with pytest.raises(ValueError, match="min_ab"):
        ST.tile_atoms(sb, min_ab=0.0)


# ------------------------------------------------------------------------------------------------ registration
def test_voronoi_hip_is_registered():
    assert "voronoi.hip" in BUILD.SOURCES and (BUILD.CSRC / "voronoi.hip").exists()
    header = (BUILD.PKG.parent / "include" / "adsorbdiff_hip.h").read_text()
    lib = L.load()
    for name, nargs in (("adf_voronoi_coordination", 15), ("adf_bulk_coordination_min", 8), ("adf_tag_surface_atoms", 18)):
        assert name in L.EXPORTS and f"int32_t {name}(" in header
        assert len(getattr(lib, name).argtypes) == nargs
    assert "weight_tol" in header and "cn_tol" in header and "Security radius" in header
    # refused on the host, before anything is launched: this needs no device
    assert lib.adf_voronoi_coordination(None, None, None, None, 1, 1, None, 13.0, 0.1, 100.0, None, None, None, None,
                                        None) == L.ADF_EINVAL
    assert b"null argument" in lib.adf_last_error()
    assert lib.adf_bulk_coordination_min(None, None, None, None, 1, 1, None, None) == L.ADF_EINVAL
    assert b"null argument" in lib.adf_last_error()
    assert lib.adf_tag_surface_atoms(None, None, None, None, None, 1, 1, None, None, 2.0, 13.0, 0.1, 100.0, 1e-3, None, None,
                                     None, None) == L.ADF_EINVAL
    assert b"null argument" in lib.adf_last_error()


# ------------------------------------------------------------------------------------------------ the Python entry points
def test_argument_checks_and_no_cpu_fallback():
    sb = H.batch_of([H.case("111_3x3x4"), H.case("fcc4_rattled")])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for kw in ("cutoff", "tol", "far"):
            with pytest.raises(ValueError, match=kw):
                ST.voronoi_coordination(sb, **{kw: bad})
            with pytest.raises(ValueError, match=kw):
                ST.tag_surface_atoms(sb, masses=H.synthetic_masses(), **{kw: bad})
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="height"):
            ST.tag_surface_atoms(sb, height=bad, masses=H.synthetic_masses())
        with pytest.raises(ValueError, match="cn_tol"):
            ST.tag_surface_atoms(sb, cn_tol=bad, masses=H.synthetic_masses())
    for call in (lambda: ST.voronoi_coordination(sb), lambda: ST.bulk_coordination(sb),
                 lambda: ST.tag_surface_atoms(sb, masses=H.synthetic_masses())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert ST.VoronoiCoordination._fields == ("cn", "omega_max", "num_neighbors", "open")
    assert ST._mass_table(np.arange(100.0), "cpu").shape == (119,) and float(ST._mass_table(np.arange(100.0), "cpu")[99]) == 99.0
    with pytest.raises(ValueError, match="empty mass table"):
        ST._mass_table([], "cpu")
