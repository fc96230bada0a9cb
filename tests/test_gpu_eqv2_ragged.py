"""The HIP EquiformerV2 path on ragged graphs, chunk seams and polar edge frames, against the FLOAT64 oracle.

The other EquiformerV2 GPU tests run saturated slabs (every atom has exactly K = 20 in-edges) in one node chunk and compare
with a float32 oracle at 1e-4.  Here: CSR segments of 0, 1, ..., K, K + 1, 63 / 64 / 65 and 128 edges (tests/
helpers_eqv2_ragged.py), the node-chunk loop of the driver with an empty chunk and a short last chunk, edges on and next to
the pole of `eq_wigner_kernel`'s frame, and two bounds on every output, every block and every degree:
  hard   1e-4, the project's budget;
  tight  10 x the float32 oracle's own distance from the float64 oracle on the same case, computed in the test.  A float32
         evaluation of this model sits 1e-6 to 6e-6 from the float64 one on these graphs; the HIP path measured about twice a
         float32 evaluation's error on the fixtures, so 10 x leaves a factor of five for another graph and still fails a
         kernel that is 1e-4-correct only.
Every figure is printed before it is asserted (pytest -rA shows them).
"""
import pytest
import torch

from tests import helpers_eqv2_ragged as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK_VAR = "ADF_EQV2_CHUNK_EDGES"

_MODELS = {}


def model(name, cutoff=12.0):
    if (name, cutoff) not in _MODELS:
        _MODELS[(name, cutoff)] = H.make(name, cutoff).to(DEV)
    return _MODELS[(name, cutoff)]


def fresh_engine(m, exact=False):
    """A new handle (it reads the environment's switches at creation) with the given arithmetic."""
    if m._engine is not None:
        m._engine.close()
    m._engine = None
    eng = m.engine()
    eng.set_arithmetic(exact)
    return eng


def ragged_case(name, which="ragged"):
    """(model, graph, batch, float32 oracle, float64 oracle), the oracles computed once per (model, graph)."""
    ei, vec, Z = H.ragged_graph() if which == "ragged" else H.rotated_ragged_graph()
    m = model(name)
    r32, r64 = H.oracle_pair((name, which), m, Z, graph=(ei, vec))
    return m, (ei, vec), H.one_system_batch(Z).to(DEV), r32, r64


def assert_isolated_rows_are_zero(f1, f2, rows):
    idx = torch.as_tensor(rows, device=f1.device)
    assert bool((f1[idx] == 0.0).all()) and bool((f2[idx] == 0.0).all()), (f1[idx], f2[idx])


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", ["small", "mfma"])
def test_ragged_graph_vs_fp64_oracle(name, exact):
    """Both heads and the node embeddings after the edge-degree embedding and after every block, per degree, on the 23-node
    ragged edge list, under both bounds; the targets without in-edges give exactly 0.0 in both heads; the engine counts
    the 443 edges."""
    m, (ei, vec), b, r32, r64 = ragged_case(name)
    eng = fresh_engine(m, exact)
    eng.set_edges(ei, vec)
    f1, f2, xb = eng.forward(b, return_blocks=True)
    assert int(eng.counters().num_edges) == ei.shape[1] == 443
    H.check_against_fp64(f"ragged {name} {'exact' if exact else 'f16x3'}", (f1, f2, xb), r32, r64, H.MODELS[name]["lmax"])
    assert_isolated_rows_are_zero(f1, f2, H.ISOLATED)


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_chunk_seams(monkeypatch, name):
    """The node-chunk loops of `eq_forward_impl`, `eq_attention` and `eq_block_nodes` with more than one chunk:
    ADF_EQV2_CHUNK_EDGES = 640 = 128 x 5 gives chunks of 5, 5, 5, 5, 3 nodes (the third one, nodes 10..14, has no edge at
    all; the last one is short), 1 gives one node per chunk.  Every product, softmax and sum of a row depends on that row's
    target alone, so both heads and all blocks equal the single-chunk forward bit for bit, and stay within the oracle's
    bounds."""
    m, (ei, vec), b, r32, r64 = ragged_case(name)
    monkeypatch.delenv(CHUNK_VAR, raising=False)
    eng = fresh_engine(m)
    eng.set_edges(ei, vec)
    eng.profile_enable(True)
    f1, f2, xb = eng.forward(b, return_blocks=True)
    # the profiler opens one "attn_weights" group per chunk of every attention (2 blocks + 2 force blocks)
    assert eng.profile_read()["attn_weights"][1] == 4
    H.check_against_fp64(f"chunks {name} one chunk", (f1, f2, xb), r32, r64, H.MODELS[name]["lmax"])
    for value, chunks in (("640", 5), ("1", 23)):
        monkeypatch.setenv(CHUNK_VAR, value)
        eng = fresh_engine(m)
        eng.set_edges(ei, vec)
        eng.profile_enable(True)
        g1, g2, yb = eng.forward(b, return_blocks=True)
        assert eng.profile_read()["attn_weights"][1] == 4 * chunks, "the chunk size did not reach the driver"
        print(f"chunks {name} {CHUNK_VAR}={value}: max |diff| to one chunk: f1 {float((g1 - f1).abs().max()):.2e} "
              f"f2 {float((g2 - f2).abs().max()):.2e} blocks {float((yb - xb).abs().max()):.2e}")
        H.check_against_fp64(f"chunks {name} {CHUNK_VAR}={value}", (g1, g2, yb), r32, r64, H.MODELS[name]["lmax"])
        assert torch.equal(g1, f1) and torch.equal(g2, f2) and torch.equal(yb, xb), value
        assert_isolated_rows_are_zero(g1, g2, H.ISOLATED)
    monkeypatch.delenv(CHUNK_VAR)
    fresh_engine(m)   # the next test's engine does not inherit the one-node chunks


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_subset_forward_on_ragged_targets(name):
    """`forward_prepared(out_idx=...)` on the first isolated node, the 40-edge target, the 128-edge hub, a one-edge target
    and the last (isolated) node: the listed rows equal the full forward's bit for bit, the others are not written."""
    m, (ei, vec), b, r32, r64 = ragged_case(name)
    eng = fresh_engine(m)
    eng.set_edges(ei, vec)
    f1, f2 = eng.forward(b)
    rows = [0, 9, 18, 21, 22]
    assert [H.DEGREES[i] for i in rows] == [0, 40, 128, 1, 0]
    prep = eng.prepare(b)
    idx = torch.tensor(rows, dtype=torch.int32, device=DEV)
    g1, g2 = torch.full_like(f1, 7.0), torch.full_like(f2, 7.0)
    eng.forward_prepared(prep, b.pos.float().contiguous(), g1, g2, out_idx=idx)
    eng.check_flags()
    li = idx.long()
    assert torch.equal(g1[li], f1[li]) and torch.equal(g2[li], f2[li])
    rest = torch.ones(prep.num_atoms, dtype=torch.bool, device=DEV)
    rest[li] = False
    assert bool((g1[rest] == 7.0).all()) and bool((g2[rest] == 7.0).all())
    assert_isolated_rows_are_zero(g1, g2, [0, 22])
    H.check_against_fp64(f"subset {name} full forward", (f1, f2), r32, r64, H.MODELS[name]["lmax"])


@pytest.mark.parametrize("exact", [False, True])
def test_own_graph_unsaturated_vs_fp64_oracle(exact):
    """The device's own graph builder below saturation (cutoff 6 A, in-degrees 0 .. 11 < K, one isolated atom, systems of
    2, 9 and 14 atoms): the same number of edges as the oracle's builder, outputs and blocks within the bounds, exactly
    zero rows for the isolated atom, no device flag raised."""
    from oracle import eqv2_oracle as Q

    b, deg = H.sparse_batch()
    m = model("small", H.SPARSE_CUTOFF)
    r32, r64 = H.oracle_pair(("small", "sparse"), m, b.atomic_numbers, batch=b)
    ei, _, _ = Q.radius_graph_pbc(b.pos, b.cell, b.natoms, H.SPARSE_CUTOFF, H.K)
    eng = fresh_engine(m, exact)
    eng.set_edges(None, None)
    f1, f2, xb = eng.forward(b.to(DEV), return_blocks=True)
    eng.check_flags()
    assert int(eng.counters().num_edges) == ei.shape[1] == int(deg.sum())
    H.check_against_fp64(f"own graph {'exact' if exact else 'f16x3'}", (f1, f2, xb), r32, r64, H.MODELS["small"]["lmax"])
    assert_isolated_rows_are_zero(f1, f2, torch.nonzero(deg == 0).reshape(-1).tolist())


def test_live_distance_basis_on_ragged_graph():
    """Radii divided by 100 and the basis part of every first radial layer times 3 (the setup of
    tests/test_gpu_eqv2.py::test_eqv2_distance_basis_path_vs_oracle): the per-edge radial path and its Gaussian window on
    empty and long segments, against the float64 oracle given the same radii."""
    from oracle import eqv2_oracle as Q
    from tests.test_gpu_eqv2 import oracle_hp

    ei, vec, Z = H.ragged_graph()
    m = H.make("small")
    with torch.no_grad():
        m.atom_radii.div_(100.0)
        for n, p in m.named_parameters():
            if n.endswith("rad_func.net.0.weight"):
                p[:, :600].mul_(3.0)
    radii = m.atom_radii.detach().clone()
    r32, r64 = H.oracle_pair(("small", "basis"), m, Z, graph=(ei, vec), atom_radii=radii)
    b = H.one_system_batch(Z)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        z1, _ = Q.eqv2_forward(sd, oracle_hp(m), b.pos, b.atomic_numbers, b.cell, b.natoms, graph=(ei, vec))
    assert H.frob(z1, r32[0]) > 1e-3, "the distance basis does not reach the outputs of this test model"
    m = m.to(DEV)
    eng = fresh_engine(m)
    eng.set_edges(ei, vec)
    f1, f2, xb = eng.forward(b.to(DEV), return_blocks=True)
    H.check_against_fp64("live basis small", (f1, f2, xb), r32, r64, H.MODELS["small"]["lmax"])
    assert_isolated_rows_are_zero(f1, f2, H.ISOLATED)
    m._engine.close()
    m._engine = None


def test_rotated_ragged_graph_vs_fp64_oracle():
    """The ragged graph's vectors under one fixed proper rotation that puts a generic edge of the 128-edge hub exactly on
    -y: a second, unrelated set of edge frames (more oracle cases; no equivariance is asserted)."""
    m, (ei, vec), b, r32, r64 = ragged_case("small", "rotated")
    eng = fresh_engine(m)
    eng.set_edges(ei, vec)
    f1, f2, xb = eng.forward(b, return_blocks=True)
    H.check_against_fp64("rotated small", (f1, f2, xb), r32, r64, H.MODELS["small"]["lmax"])
    assert_isolated_rows_are_zero(f1, f2, H.ISOLATED)
