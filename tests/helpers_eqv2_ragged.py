"""Ragged inputs for the EquiformerV2 path (CPU only, seeded, deterministic) and the float64-oracle bounds the tests on
them share: tests/test_eqv2_ragged_host.py (oracle side) and tests/test_gpu_eqv2_ragged.py (device side).

`ragged_graph()`: one explicit 23-node edge list for `engine.set_edges` with empty, single-edge, K, K + 1, wave-sized and
128-edge CSR segments and edges on / next to the polar axis of `eq_wigner_kernel`'s frame.
`sparse_batch()`: three small systems whose own radius graph is far from saturated (degrees 0, 1, ... below K).
"""
import math

import torch

from adsorbdiff_amd.data import Batch

REL_TOL = 1e-4          # the project's budget (BASELINE.json north_star)
TIGHT_FACTOR = 10.0     # tight bound = 10 x the float32 oracle's own distance from the float64 oracle on the same case
K = 20
# in-degree of every node, in node order
DEGREES = [0, 1, 2, 3, 5, 0, 17, 20, 21, 40, 0, 0, 0, 0, 0, 63, 64, 65, 128, 4, 9, 1, 0]
ISOLATED = [i for i, d in enumerate(DEGREES) if d == 0]
# exact vectors written onto the first edges (targets 1, 2, 3, 4: the small segments): +-y is the pole of the kernel's frame
# (rho = |(n_x, n_z)| = 0: cg = 1, sg = 0), the last three lie just off it (rho = 1.1e-7, 5e-7, 5e-5: the kernel divides by rho)
POLAR = [(0.0, 2.5, 0.0), (0.0, -3.0, 0.0), (1e-7, 2.0, -2e-7), (0.0, -2.0, 1e-6), (3.0, 0.0, 0.0), (0.0, 0.0, -3.0),
         (1e-4, 2.0, 0.0)]

MODELS = {
    # generic logit kernel, scalar products
    "small": dict(lmax=4, mmax=2, C=8, hidden=8, heads=2, alpha=4, value=4, ffn=16, ec=8, layers=2),
    # alpha-64 four-heads kernel, f16x3 matrix-core products, two S2 waves per edge
    "mfma": dict(lmax=6, mmax=2, C=32, hidden=64, heads=8, alpha=64, value=16, ffn=32, ec=32, layers=2),
}


def make(name, cutoff=12.0):
    from tests.test_gpu_eqv2 import make_model

    return make_model(cutoff=cutoff, **MODELS[name])


def ragged_graph():
    """(edge_index [2, E] (source, target) sorted by target, edge_vec [E, 3], Z [23])."""
    N = len(DEGREES)
    g = torch.Generator().manual_seed(3)
    E = sum(DEGREES)
    dst = torch.repeat_interleave(torch.arange(N), torch.tensor(DEGREES))
    src = torch.randint(0, N, (E,), generator=g)               # isolated nodes are sources too; some self-loops
    vec = torch.randn(E, 3, generator=g) * 3.0
    length = vec.norm(dim=1, keepdim=True)
    vec = vec / length * length.clamp(0.5, 11.9)
    vec[:len(POLAR)] = torch.tensor(POLAR)
    Z = torch.randint(1, 80, (N,), generator=g).float()
    Z[(Z == 36) | (Z == 54)] = 47.0                            # no tabulated radius (tests/test_gpu_eqv2.py::safe_batch)
    ei = torch.stack([src, dst])
    # the properties the tests rely on
    deg = torch.bincount(dst, minlength=N).tolist()
    assert deg == DEGREES and N == 23 and E == 443 and E % 4 == 3
    assert DEGREES[0] == 0 and DEGREES[-1] == 0 and ISOLATED == [0, 5, 10, 11, 12, 13, 14, 22]
    assert {K, K + 1, 63, 64, 65, 128} <= set(DEGREES) and max(DEGREES) == 128
    assert bool((dst[1:] >= dst[:-1]).all())
    assert len(set(src.tolist()) & set(ISOLATED)) > 0, "no isolated node is a source"
    loops = src == dst
    assert bool(loops.any()) and float(vec[loops].norm(dim=1).min()) > 0.0
    d = vec.norm(dim=1)
    assert float(d.min()) >= 0.5 - 1e-6 and float(d.max()) <= 11.9 + 1e-5
    assert int(dst[len(POLAR) - 1]) <= 4                       # the exact vectors sit on the small-degree targets
    return ei, vec, Z


def one_system_batch(Z, box=30.0, seed=1):
    """A batch that carries Z for an explicit edge list: the positions are not read when `set_edges` is in force."""
    n = int(Z.shape[0])
    b = Batch()
    b.pos = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 10.0 + 10.0
    b.atomic_numbers = Z.float().clone()
    b.tags = torch.ones(n, dtype=torch.long)
    b.fixed = torch.zeros(n, dtype=torch.long)
    b.cell = torch.eye(3)[None] * box
    b.natoms = torch.tensor([n])
    b.batch = torch.zeros(n, dtype=torch.long)
    b.sid = ["0"]
    return b


def rotation_onto_minus_y(v):
    """The proper rotation (float64 [3, 3]) about v x (-y) that takes v / |v| onto -y (Rodrigues)."""
    a = v.double() / v.double().norm()
    t = torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64)
    ax = torch.linalg.cross(a, t)
    s, c = float(ax.norm()), float(a @ t)
    ax = ax / s
    Kx = torch.tensor([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + s * Kx + (1.0 - c) * (Kx @ Kx)
    assert float((R @ a - t).abs().max()) < 1e-14 and abs(float(torch.linalg.det(R)) - 1.0) < 1e-12
    return R


def rotated_ragged_graph():
    """The ragged graph with every vector turned by one fixed proper rotation that takes a generic edge (the first one of
    the 128-edge hub) onto -y: another, unrelated set of edge frames.  No equivariance is claimed."""
    ei, vec, Z = ragged_graph()
    e = int(torch.nonzero(ei[1] == 18)[0])
    R = rotation_onto_minus_y(vec[e])
    out = (vec.double() @ R.T).float()
    out[e] = torch.tensor([0.0, -float(vec[e].double().norm()), 0.0])   # exactly on the pole, not one rounding off it
    return ei, out, Z


SPARSE_NATOMS = (2, 9, 14)
SPARSE_CUTOFF = 6.0


def sparse_batch():
    """Three systems (2, 9, 14 atoms) spread over a ~9 A box inside triclinic ~30 A cells (wider than twice the 6 A cutoff:
    no self-images, no ties); the last atom sits more than 7 A from every other one.  Returns (batch, in-degrees)."""
    from oracle import eqv2_oracle as Q

    g = torch.Generator().manual_seed(3)   # (seed 5 leaves the two-atom system without an edge)
    pos = [torch.rand(n, 3, generator=g) * 9.0 + 8.0 for n in SPARSE_NATOMS]
    pos[2][-1] = torch.tensor([25.0, 25.0, 2.0])
    pos = torch.cat(pos)
    n = int(pos.shape[0])
    b = Batch()
    b.pos = pos
    Z = torch.randint(1, 80, (n,), generator=g).float()
    Z[(Z == 36) | (Z == 54)] = 47.0
    b.atomic_numbers = Z
    b.tags = torch.ones(n, dtype=torch.long)
    b.fixed = torch.zeros(n, dtype=torch.long)
    b.cell = torch.tensor([[30.0, 0.0, 0.0], [3.0, 29.0, 0.0], [0.0, 2.0, 31.0]])[None].repeat(3, 1, 1)
    b.natoms = torch.tensor(SPARSE_NATOMS)
    b.batch = torch.repeat_interleave(torch.arange(3), b.natoms)
    b.sid = ["0", "1", "2"]
    ei, sh, nb = Q.radius_graph_pbc(b.pos, b.cell, b.natoms, SPARSE_CUTOFF, K)
    ei, d, v, _ = Q.pbc_distances(b.pos, ei, b.cell, sh, nb)
    deg = torch.bincount(ei[1], minlength=n)
    low = set(deg[deg < K].tolist())
    assert len(low) >= 4 and {0, 1} <= low, sorted(low)
    assert int(nb.min()) > 0, "a system without edges is the empty-image error, not this test"
    assert int(deg[-1]) == 0 and float((pos[:-1] - pos[-1]).norm(dim=1).min()) > 7.0
    assert bool((sh == 0).all())                               # no periodic image is a neighbour
    # no near-tie at the cutoff: float32 and float64 arithmetic choose the same edges
    pair = torch.cat([torch.pdist(p.double()) for p in torch.split(pos, list(SPARSE_NATOMS))])
    assert float((pair - SPARSE_CUTOFF).abs().min()) > 1e-3
    return b, deg


# ------------------------------------------------------------------------------------------------ oracle + bounds
_ORACLE = {}


def oracle_pair(key, model, Z, graph=None, batch=None, atom_radii=None):
    """((f1, f2) float32 oracle, (f1, f2, x_blocks) float64 oracle) of `model` on an explicit edge list (`graph`) or on the
    oracle's own radius graph of `batch`; computed once per `key` and left unchanged."""
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import eqv2_oracle as Q
    from tests.test_gpu_eqv2 import oracle_hp

    sd = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    b = batch if batch is not None else one_system_batch(Z)
    kw = dict(graph=graph, atom_radii=atom_radii)
    with torch.no_grad():
        r32 = Q.eqv2_forward(sd, oracle_hp(model), b.pos, b.atomic_numbers, b.cell, b.natoms, **kw)
        r64 = Q.eqv2_forward(sd, oracle_hp(model), b.pos, b.atomic_numbers, b.cell, b.natoms, dtype=torch.float64,
                             return_blocks=True, **kw)
    assert r32[0].dtype == torch.float32 and r64[0].dtype == torch.float64 and r64[2].dtype == torch.float64
    _ORACLE[key] = (r32, r64)
    return _ORACLE[key]


def frob(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def row_err(a, b):
    """Largest row of a - b against the largest row of b."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    return float((a - b).norm(dim=1).max() / b.norm(dim=1).max().clamp(min=1e-300))


def oracle_distance(r32, r64):
    """The float32 oracle's distance from the float64 one: the larger Frobenius ratio of the two heads."""
    return max(frob(r32[0], r64[0]), frob(r32[1], r64[1]))


def check_against_fp64(label, got, r32, r64, lmax, tight=True):
    """Both heads and (when given) every block and degree of `got` = (f1, f2[, x_blocks]) against the float64 oracle: Frobenius
    ratio and largest row against the largest reference row, each under the hard bound (1e-4) and, with `tight`, under
    10 x the float32 oracle's own distance on this case.  Prints every figure before asserting."""
    dist = oracle_distance(r32, r64)
    bound = TIGHT_FACTOR * dist
    print(f"{label}: float32-oracle distance {dist:.2e}  tight bound {bound:.2e}{'' if tight else ' (not asserted)'}  hard bound {REL_TOL:.0e}")
    figures = []
    for name, g, r in (("f1", got[0], r64[0]), ("f2", got[1], r64[1])):
        figures.append((name, frob(g, r), row_err(g, r)))
    if len(got) > 2 and got[2] is not None:
        xb, rb = got[2], r64[2]
        assert tuple(xb.shape) == tuple(rb.shape), (tuple(xb.shape), tuple(rb.shape))
        for k in range(rb.shape[0]):
            for l in range(lmax + 1):
                sl = slice(l * l, (l + 1) ** 2)
                figures.append((f"x_blocks[{k}] l={l}", frob(xb[k, :, sl], rb[k, :, sl]), row_err(xb[k, :, sl], rb[k, :, sl])))
    worst = max(max(f, r) for _, f, r in figures)
    for name, f, r in figures:
        print(f"{label}:   {name:<18s} frobenius {f:.2e}  row {r:.2e}")
    print(f"{label}: worst {worst:.2e}")
    for name, f, r in figures:
        assert math.isfinite(f) and math.isfinite(r), (label, name, f, r)
        assert f < REL_TOL and r < REL_TOL, (label, name, f, r)
        if tight:
            assert f < bound and r < bound, (label, name, f, r, bound)
    return worst
