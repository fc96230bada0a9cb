"""CPU side of the ragged EquiformerV2 tests: the generators' structural properties (tests/helpers_eqv2_ragged.py) and the
float64 mode of oracle/eqv2_oracle.py the GPU tests measure against.

Measured on the CPU (relative Frobenius distance of the float32 oracle from the float64 oracle, heads f1 / f2):
  ragged graph, small model (L=4, C=8, 2 blocks)                         1.5e-6 / 1.1e-6
  ragged graph, mfma model (L=6, C=32, hidden 64, 8 heads, alpha 64)     3.6e-6 / 5.8e-6
  sparse own-graph batch, small model, cutoff 6                          8.5e-7 / 5.8e-7
  rotated ragged graph, small model                                      1.9e-6 (larger head)
  ragged graph with the live distance basis, small model                 5.0e-6 (larger head)
The node embeddings of the float32 oracle are 1e-7 to 1e-6 from the float64 ones per block and degree.  The float64 forward
of the mfma model takes under a second.
"""
import pytest
import torch

from tests import helpers_eqv2_ragged as H
from tests.helpers import batch_from_fixture, load_npz, state_dict_from_fixture


def test_ragged_graph_structure():
    ei, vec, Z = H.ragged_graph()           # asserts degrees, counts, sources, self-loops and lengths itself
    assert ei.shape == (2, 443) and vec.shape == (443, 3) and Z.shape == (23,)
    assert ei.dtype == torch.int64 and vec.dtype == torch.float32
    # five isolated nodes in a row: one whole empty chunk at five nodes per chunk (chunk 2 = nodes 10..14)
    assert H.DEGREES[10:15] == [0] * 5 and sum(H.DEGREES[:10]) == int((ei[1] < 10).sum())
    assert torch.equal(vec[:7], torch.tensor(H.POLAR))
    rho = (vec[:, [0, 2]] / vec.norm(dim=1, keepdim=True)).norm(dim=1)
    assert int((rho == 0).sum()) == 2 and int(((rho > 0) & (rho < 1e-4)).sum()) == 3
    assert float(Z.min()) >= 1 and float(Z.max()) < 80 and not bool(((Z == 36) | (Z == 54)).any())
    again = H.ragged_graph()
    assert all(torch.equal(a, b) for a, b in zip((ei, vec, Z), again))


def test_rotated_ragged_graph_structure():
    ei, vec, Z = H.ragged_graph()
    ej, rot, _ = H.rotated_ragged_graph()
    assert torch.equal(ei, ej)
    assert float((rot.norm(dim=1) - vec.norm(dim=1)).abs().max()) < 1e-5
    e = int(torch.nonzero(ei[1] == 18)[0])
    assert float(rot[e, 0]) == 0.0 and float(rot[e, 2]) == 0.0 and float(rot[e, 1]) < 0.0
    assert float((rot - vec).norm(dim=1).median()) > 1.0       # another set of frames


def test_sparse_batch_structure():
    b, deg = H.sparse_batch()               # asserts the in-degree spread, the isolated atom and the absence of ties itself
    assert b.natoms.tolist() == [2, 9, 14] and int(deg.max()) < H.K
    print("sparse batch in-degrees", deg.tolist())


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_fp64_oracle_on_ragged_graph(name):
    """The float64 oracle is finite, returns exactly 0.0 for targets without in-edges (zero aggregate, and so3_linear has a
    bias on l = 0 only), every other row is above 1e-3 of the largest (the comparison is not vacuous), and the float32
    oracle is within 1e-5 of it."""
    ei, vec, Z = H.ragged_graph()
    m = H.make(name)
    r32, r64 = H.oracle_pair((name, "ragged"), m, Z, graph=(ei, vec))
    L = H.MODELS[name]["lmax"]
    assert r64[2].shape == (3, 23, (L + 1) ** 2, H.MODELS[name]["C"])
    iso = torch.tensor(H.ISOLATED)
    rest = torch.tensor([i for i in range(23) if i not in H.ISOLATED])
    for k in (0, 1):
        assert bool(torch.isfinite(r64[k]).all()) and bool(torch.isfinite(r32[k]).all())
        assert bool((r64[k][iso] == 0.0).all()) and bool((r32[k][iso] == 0.0).all())
        rn = r64[k].norm(dim=1)
        assert float(rn[rest].min()) > 1e-3 * float(rn.max()), (k, float(rn[rest].min()), float(rn.max()))
    assert bool(torch.isfinite(r64[2]).all())
    d1, d2 = H.frob(r32[0], r64[0]), H.frob(r32[1], r64[1])
    print(f"{name}: float32 oracle vs float64 oracle on the ragged graph: {d1:.2e} {d2:.2e}")
    assert 0.0 < d1 < 1e-5 and 0.0 < d2 < 1e-5


def test_fp64_oracle_on_sparse_own_graph():
    b, deg = H.sparse_batch()
    m = H.make("small", cutoff=H.SPARSE_CUTOFF)
    r32, r64 = H.oracle_pair(("small", "sparse"), m, b.atomic_numbers, batch=b)
    for k in (0, 1):
        assert bool(torch.isfinite(r64[k]).all())
        assert bool((r64[k][deg == 0] == 0.0).all())
        rn = r64[k].norm(dim=1)
        assert float(rn[deg > 0].min()) > 1e-3 * float(rn.max())
    d1, d2 = H.frob(r32[0], r64[0]), H.frob(r32[1], r64[1])
    print(f"small: float32 oracle vs float64 oracle on the sparse own-graph batch: {d1:.2e} {d2:.2e}")
    assert 0.0 < d1 < 1e-5 and 0.0 < d2 < 1e-5


def test_float32_default_of_the_oracle_is_unchanged():
    """`dtype` defaults to float32 and the default evaluates what it evaluated before the argument existed: the explicit
    float32 call, the default call and the call that also returns the blocks give the same bits, all in float32, on the
    l4m2 fixture case (tests/test_oracle_golden.py holds the same call against the reference's recordings, unchanged)."""
    from oracle import eqv2_oracle as Q
    from tests.test_gpu_eqv2 import parse_hp

    fx = load_npz("eqv2_l4m2.npz")
    hpf = parse_hp(fx)
    hp = dict(lmax=int(fx["lmax"]), mmax=int(fx["mmax"]), **{k: hpf[k] for k in (
        "num_layers", "sphere_channels", "attn_hidden_channels", "num_heads", "attn_alpha_channels", "attn_value_channels",
        "ffn_hidden_channels", "grid_resolution", "max_radius", "max_neighbors")})
    sd = state_dict_from_fixture(fx)
    b = batch_from_fixture(fx)
    graph = (torch.from_numpy(fx["edge_index"]), torch.from_numpy(fx["edge_vec"]))
    with torch.no_grad():
        a = Q.eqv2_forward(sd, hp, b.pos, b.atomic_numbers, b.cell, b.natoms, graph=graph)
        c = Q.eqv2_forward(sd, hp, b.pos, b.atomic_numbers, b.cell, b.natoms, graph=graph, dtype=torch.float32)
        e = Q.eqv2_forward(sd, hp, b.pos, b.atomic_numbers, b.cell, b.natoms, graph=graph, return_blocks=True)
        w = Q.eqv2_forward(sd, hp, b.pos, b.atomic_numbers, b.cell, b.natoms, graph=graph, dtype=torch.float64)
    assert len(a) == 2 and a[0].dtype == torch.float32 and e[2].dtype == torch.float32
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[0], e[0]) and torch.equal(a[1], e[1])
    # the recorded reference outputs: the float32 default is where it was (1e-5, tests/test_oracle_golden.py), and the
    # float64 mode is the same function
    assert H.frob(a[0], fx["f1"]) < 1e-5 and H.frob(a[1], fx["f2"]) < 1e-5
    assert w[0].dtype == torch.float64 and H.frob(a[0], w[0]) < 1e-5 and H.frob(a[1], w[1]) < 1e-5
    assert torch.get_default_dtype() == torch.float32            # the float64 tables do not leak a default dtype
    # the recorded node embeddings: the new `return_blocks` output is the quantity the fixtures call x_blocks
    for k in range(e[2].shape[0]):
        assert H.frob(e[2][k], fx["x_blocks"][k]) < 1e-5, k
