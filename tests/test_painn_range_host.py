"""CPU side of tests/test_gpu_painn_range.py: for every case of helpers_painn_range.CASES, on the oracle's own graph, the
float32 oracle stays inside every bound the device is held to by at least HOST_MARGIN (4) - the bounds are achievable in
single precision before a GPU is involved - and the measures mean what they say: at most FLOOR_SHARE (10 %) of the rows of
any compared reference tensor lie under the row floor (the exactly-zero vec rows of ``k1`` are compared exactly instead),
and every case has the structural property it exists for."""
import pytest
import torch

from tests import helpers_painn_range as PR

_BATCH = None


def _batch():
    global _BATCH
    if _BATCH is None:
        _BATCH = PR.make_batch()
    return _BATCH


def test_case_table_covers_the_accepted_range():
    c = PR.CASES
    assert {v["H"] for v in c.values()} >= {128, 192, 320, 384, 640, 1024}
    assert {v["R"] for v in c.values()} >= {2, 8, 24, 30, 40, 64, 96, 120, 126, 128}
    assert {v["p"] for v in c.values()} == {3, 5, 7} and {v["K"] for v in c.values()} >= {1, 20, 128}
    assert max(v["L"] for v in c.values()) == 16 and not c["one_head"]["so3"]
    assert c["direct128"]["direct"] and c["direct24"]["direct"] and c["direct24"]["R"] == 24
    assert all(v["H"] % 64 == 0 and v["R"] % 2 == 0 for v in c.values())
    assert set(PR.ENERGY_CASES) <= set(c)


@pytest.mark.parametrize("name", list(PR.CASES))
def test_float32_oracle_is_inside_every_bound_with_margin(name):
    b = _batch()
    m = PR.make_model(name)
    graph = PR.oracle_graph(name, b)
    PR.assert_structure(name, graph, b)
    bound = PR.REL_TOL / PR.HOST_MARGIN
    f1, f2, cap = PR.forward(name, m, b, graph, torch.float64)
    g1, g2, cap32 = PR.forward(name, m, b, graph, torch.float32)
    worst = {"rows": 0.0, "forced": 0.0, "heads": 0.0, "means": 0.0, "floor": 0.0}
    zero_rows = 0

    def rows(got, ref, what, key):
        nonlocal zero_rows
        e, share, zero = PR.row_figures(got, ref)
        worst[key] = max(worst[key], e)
        worst["floor"] = max(worst["floor"], share)
        assert e < bound, (name, what, e)
        assert share <= PR.FLOOR_SHARE, (name, what, share)
        assert PR.zero_rows_exact(got, zero), (name, what)
        zero_rows += int(zero.sum())

    for l, (lay, lay32) in enumerate(zip(cap["layers"], cap32["layers"])):   # chained: the forward as it runs
        rows(lay32["x"], lay["x"], "x after layer %d" % l, "rows")
        rows(lay32["vec"], lay["vec"], "vec after layer %d" % l, "rows")
    inputs = PR.block_inputs(m, b, cap)                                       # teacher-forced: what the device is handed
    ref = PR.forced_blocks(name, m, graph, inputs, torch.float64)
    got = PR.forced_blocks(name, m, graph, inputs, torch.float32)
    for l, (r4, g4) in enumerate(zip(ref, got)):
        for what, r, g in zip(("message x", "message vec", "update x", "update vec"), r4, g4):
            rows(g, r, "%s of layer %d" % (what, l), "forced")
    for what, g, r in (("f1", g1, f1), ("f2", g2, f2)):
        if r is None:
            assert name == "one_head"
            continue
        e, s = PR.head_figure(g, r, b.batch), PR.mean_figure(g, r, b)
        worst["heads"], worst["means"] = max(worst["heads"], e), max(worst["means"], s)
        assert e < bound and s < bound, (name, what, e, s)
    assert (zero_rows > 0) == (name == "k1"), (name, zero_rows)
    print("%s: float32 oracle rows %.1e, teacher-forced rows %.1e, heads %.1e, adsorbate means %.1e (bound %.1e); "
          "largest share of rows under the floor %.3f" % (name, worst["rows"], worst["forced"], worst["heads"], worst["means"],
                                                          bound, worst["floor"]))


@pytest.mark.parametrize("name", PR.ENERGY_CASES)
def test_float32_energy_and_gradient_forces_are_inside_their_bounds_with_margin(name):
    b = _batch()
    m = PR.make_model(name, energy=True)
    ei, _, dist, unit = PR.oracle_graph(name, b)
    es, ed, vec = ei[0], ei[1], unit * dist[:, None]
    e64, f64 = PR.energy_reference(name, m, b, es, ed, vec, torch.float64)
    e32, f32 = PR.energy_reference(name, m, b, es, ed, vec, torch.float32)
    e_err, f_err = PR.energy_figures(e32, f32, e64, f64)
    print("%s: float32 energy row-rel %.1e, forces max-rel %.1e (bound %.1e)" % (name, e_err, f_err, PR.REL_TOL / PR.HOST_MARGIN))
    assert e_err < PR.REL_TOL / PR.HOST_MARGIN and f_err < PR.REL_TOL / PR.HOST_MARGIN, (name, e_err, f_err)
