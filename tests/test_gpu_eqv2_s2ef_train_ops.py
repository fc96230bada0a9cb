"""``adf_op_eq_edge_dist`` / ``adf_op_eq_radial_gauss_fwd`` / ``adf_op_eq_radial_gauss_bwd`` and the whole first-layer Function
``RadialMLPLive`` against float64 torch: edge_channels under a wave, one per lane and two per lane; 0, 1, 5, 257 and 1000
edges with the hard rows of tests/test_gpu_eqv2_s2ef.py::test_radial_first_layer_vs_torch (d = rc, the 0.01 floor, just
inside each end of the basis, the table's last element pair), a d > rc row, a block of edges of one identical distance
(ties in the order, the longest single-column sum) and weight-gradient columns that no edge's window reaches.  The float64
basis uses the fp32 ``torch.linspace`` centres and the ``coeff`` derived from them.  Bounds: REL_TOL hard, and TIGHT_FACTOR
times float32 torch's own distance from float64 on the same rows; every figure is printed before it is asserted."""
import ctypes as C
import types

import pytest
import torch

from adsorbdiff_amd import lib as _lib
from oracle import eqv2_oracle as Q
from tests import helpers_eqv2_s2ef_train as S
from tests.helpers_eqv2_ragged import row_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB = S.NB
_ENG = {}


def engine(EC):
    """(model on the device, its engine, EqOps) per edge_channels, built once."""
    from adsorbdiff_amd.eqv2_train_step import EqOps

    if EC not in _ENG:
        m = S.small_train_model(edge_channels=EC).to(DEV)
        eng = m.engine(DEV)
        _ENG[EC] = (m, eng, EqOps(eng))
    return _ENG[EC]


def distances(E, rc, seed):
    """E distances: the hard rows, a block of ties, random ones below 0.8 rc (so that columns between 0.8 rc and rc stay
    out of every window), in a seeded shuffle that keeps the hard rows first."""
    g = torch.Generator().manual_seed(seed)
    hard = torch.tensor([rc, 0.01, 0.0101, rc - 1e-4, 0.5 * rc, rc * 0.999, rc * 1.02])
    ties = min(300, max(0, E - len(hard)) // 2)
    d = torch.cat([hard, torch.full((ties,), 0.3171 * rc), torch.rand(max(0, E - len(hard) - ties), generator=g) * 0.8 * rc])[:E]
    if E > len(hard):   # the ties are not contiguous in the list
        tail = d[len(hard):]
        d = torch.cat([d[:len(hard)], tail[torch.randperm(tail.numel(), generator=g)]])
    return d


def vectors(d, seed):
    g = torch.Generator().manual_seed(seed + 100)
    dirs = torch.nn.functional.normalize(torch.randn(d.numel(), 3, generator=g), dim=1)
    return (dirs * d[:, None]).float()


def device_dist(lib, vec):
    E = vec.shape[0]
    dist = torch.empty(E, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.adf_op_eq_edge_dist(vec.data_ptr() if E else None, E, dist.data_ptr() if E else None, s))
    return dist


def bounds(label, got, r64, r32, rows=True):
    """Frobenius (and largest row) of got against float64, next to float32 torch's; asserts REL_TOL and the tight bound."""
    f, f32 = S.frob(got, r64), S.frob(r32, r64)
    r, r32_ = (row_err(got, r64), row_err(r32, r64)) if rows else (0.0, 0.0)
    print(f"{label}: frobenius {f:.2e} (float32 torch {f32:.2e})" + (f"  row {r:.2e} (float32 torch {r32_:.2e})" if rows else ""))
    assert f < S.REL_TOL and r < S.REL_TOL, (label, f, r)
    assert f < S.TIGHT_FACTOR * f32 and (not rows or r < S.TIGHT_FACTOR * r32_), (label, f, f32, r, r32_)


@pytest.mark.parametrize("E", [0, 1, 5, 257, 1000])
@pytest.mark.parametrize("EC", [8, 32, 128])
def test_gauss_window_forward_and_weight_gradient_vs_float64(EC, E):
    m, eng, ops = engine(EC)
    lib, rc = eng.lib, float(m.max_radius)
    IN = NB + 2 * EC
    g = torch.Generator().manual_seed(11 * EC + E)
    d = distances(E, rc, EC + E)
    vec = vectors(d, EC + E).to(DEV)
    dist = device_dist(lib, vec)
    want_d = vec.double().norm(dim=1)
    if E:
        e = float(((dist.double() - want_d).abs() / want_d).max())
        print(f"EC {EC} E {E}: |vec| worst relative error {e:.2e}")
        assert e < 3e-7
    dc = dist.cpu()
    W0 = ((torch.rand(EC, IN, generator=g) - 0.5) * 0.3).to(DEV)
    h_pre = torch.randn(E, EC, generator=g)
    dh0 = torch.randn(E, EC, generator=g)
    dW_pre = torch.randn(EC, IN, generator=g)
    s = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t.numel() else None

    def fwd():
        h0 = h_pre.clone().to(DEV)
        sc = torch.empty(NB * EC, device=DEV)
        _lib.check(lib.adf_op_eq_radial_gauss_fwd(eng.handle, ptr(dist), W0.data_ptr(), IN, E, ptr(h0), sc.data_ptr(), sc.numel(), s()))
        return h0

    def bwd():
        dW0 = dW_pre.clone().to(DEV)
        perm = torch.sort(dist, stable=True).indices.to(torch.int32).contiguous()
        sc = torch.empty(max(4 * E, 1), device=DEV)
        gd = dh0.to(DEV)
        _lib.check(lib.adf_op_eq_radial_gauss_bwd(eng.handle, ptr(dist), ptr(perm), ptr(gd), E, dW0.data_ptr(), IN, sc.data_ptr(),
                                                  4 * E, s()))
        return dW0

    h0, h0_again, dW0, dW0_again = fwd(), fwd(), bwd(), bwd()
    assert torch.equal(h0, h0_again) and torch.equal(dW0, dW0_again), "two calls differ"
    if E == 0:
        assert torch.equal(dW0.cpu(), dW_pre)
        return
    b64, b32 = S.live_basis(dc, rc, torch.float64), S.live_basis(dc, rc, torch.float32)
    Wg = W0.cpu()[:, :NB]
    bounds(f"EC {EC} E {E} forward", h0, h_pre.double() + b64 @ Wg.double().t(), h_pre + b32 @ Wg.t())
    # columns: the embedding columns are never touched; a column no window reaches (every |d - mu_k| beyond 1.05 tmax, in
    # float64) comes back bit-identical; the others are pre-fill + sum
    offs, coeff = S.centres(rc)
    tmax = (104.0 / -coeff) ** 0.5
    gap = (dc.double()[:, None] - offs.double()[None, :]).abs().min(dim=0).values
    unreached, reached = gap > 1.05 * tmax, gap < 0.95 * tmax
    assert int(unreached.sum()) > 20 and int(reached.sum()) > 20
    out = dW0.cpu()
    assert torch.equal(out[:, NB:], dW_pre[:, NB:])
    assert torch.equal(out[:, :NB][:, unreached], dW_pre[:, :NB][:, unreached]), "a column outside every window was written"
    assert not torch.equal(out[:, :NB][:, reached], dW_pre[:, :NB][:, reached])
    want64 = dW_pre[:, :NB].double() + dh0.double().t() @ b64
    want32 = dW_pre[:, :NB] + dh0.t() @ b32
    keep = ~unreached
    bounds(f"EC {EC} E {E} weight gradient", out[:, :NB][:, keep], want64[:, keep], want32[:, keep], rows=False)
    # a scratch that is too small is refused
    sc = torch.empty(8, device=DEV)
    assert lib.adf_op_eq_radial_gauss_bwd(eng.handle, dist.data_ptr(), dist.data_ptr(), dist.data_ptr(), E, dW0.data_ptr(), IN,
                                          sc.data_ptr(), 4 * E - 1, s()) == _lib.ADF_EINVAL
    assert lib.adf_op_eq_radial_gauss_fwd(eng.handle, dist.data_ptr(), W0.data_ptr(), IN, E, h0.data_ptr(), sc.data_ptr(),
                                          NB * EC - 1, s()) == _lib.ADF_EINVAL
    assert lib.adf_op_eq_radial_gauss_fwd(eng.handle, dist.data_ptr(), W0.data_ptr(), NB - 1, E, h0.data_ptr(), sc.data_ptr(),
                                          NB * EC, s()) == _lib.ADF_EINVAL


CASES = [(8, 257), (32, 257), (128, 257), (32, 1), (32, 5), (32, 1000)]


@pytest.mark.parametrize("EC,E", CASES)
def test_first_layer_function_vs_float64(EC, E):
    """``RadialMLPLive`` (the edge-degree embedding's radial function) as a whole: its output and the gradient of every
    input against float64 autograd through ``Q.radial_mlp`` on [basis | semb[Z_src] | temb[Z_dst]]."""
    from adsorbdiff_amd.eqv2_train_step import RadialMLPLive

    m, eng, ops = engine(EC)
    rc, NE = float(m.max_radius), int(m.max_num_elements)
    gen = torch.Generator().manual_seed(5 * EC + E)
    d = distances(E, rc, 3 * EC + E)
    vec = vectors(d, 3 * EC + E).to(DEV)
    zs, zt = torch.randint(0, NE // 2, (E,), generator=gen), torch.randint(0, NE // 2, (E,), generator=gen)
    zs[:1], zt[:1] = NE - 1, NE - 1          # the table's last element pair
    graph = types.SimpleNamespace(E=E, vec=vec, zs1=(zs + 1).to(DEV, torch.int32), zt1=(zt + 1).to(DEV, torch.int32), dist=None,
                                  dperm=None)
    mod = m.edge_degree_embedding
    names = ["semb", "temb"] + [f"net.{i}.{k}" for i in (0, 1, 3, 4, 6) for k in ("weight", "bias")]
    params = [mod.source_embedding.weight, mod.target_embedding.weight] + [dict(mod.rad_func.named_parameters())[n] for n in names[2:]]
    params = [p.detach().clone() for p in params]
    params[2][:, :NB].mul_(3.0)   # let the basis part of the layer matter
    leaves = [p.detach().clone().requires_grad_(True) for p in params]
    out = RadialMLPLive.apply(ops, graph, 0, *leaves)
    R = torch.randn(out.shape, generator=gen)
    out.backward(R.to(DEV))
    again = [p.detach().clone().requires_grad_(True) for p in params]
    out2 = RadialMLPLive.apply(ops, graph, 0, *again)
    out2.backward(R.to(DEV))
    assert torch.equal(out, out2) and all(torch.equal(a.grad, b.grad) for a, b in zip(leaves, again)), "two calls differ"
    dist = graph.dist.cpu()
    assert float(((dist.double() - vec.cpu().double().norm(dim=1)).abs() / vec.cpu().double().norm(dim=1)).max()) < 3e-7

    def reference(dtype):
        lv = [p.detach().cpu().to(dtype).requires_grad_(True) for p in params]
        sd = {"r." + n: t for n, t in zip(names[2:], lv[2:])}
        scal = torch.cat([S.live_basis(dist, rc, dtype), lv[0][zs], lv[1][zt]], dim=1)
        o = Q.radial_mlp(sd, "r.", scal)
        (o * R.to(dtype)).sum().backward()
        return o.detach(), [t.grad for t in lv]

    o64, g64 = reference(torch.float64)
    o32, g32 = reference(torch.float32)
    label = f"function EC {EC} E {E}"
    bounds(label + " output", out.detach(), o64, o32)
    for n, lf, r, r32 in zip(names, leaves, g64, g32):
        if n == "net.0.weight":
            bounds(label + " d net.0.weight (Gaussian columns)", lf.grad[:, :NB], r[:, :NB], r32[:, :NB], rows=False)
        e, e32 = S.frob(lf.grad, r), S.frob(r32, r)
        print(f"{label} d {n}: {e:.2e} (float32 torch {e32:.2e})")
        assert e < S.REL_TOL, (label, n, e)
    # rows of the embedding tables for elements no edge holds: exactly zero
    for lf, z in ((leaves[0], zs), (leaves[1], zt)):
        absent = torch.ones(NE, dtype=torch.bool)
        absent[z] = False
        assert bool(absent.any()) and float(lf.grad.cpu()[absent].abs().max()) == 0.0
