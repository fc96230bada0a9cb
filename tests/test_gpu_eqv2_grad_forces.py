"""Energy-gradient forces of the EquiformerV2 S2EF force field (``force_mode = "energy_gradient"``): the five
entries of csrc/eqv2_geo.h one by one against float64 torch, then the whole forces against the float64 autograd of the
yardstick (tests/helpers_eqv2_grad_forces.py) on the device's own exported graph, the pole of the device's frame, the
reported energy, reproducibility, the net force, the untouched direct mode and training steps, ``ml_relax`` and ``validate``.

Bounds.  Whole forces: max|dF| / max|F| against float64 under 4 x the float32 yardstick's own distance from float64 on the
same case (it sums in other orders, but also in exact f32), recorded here from the CPU run of the yardstick; the device's
measured value stands beside it:

    case                    float32 yardstick   bound (4 x)   device
    fixture (2 systems)     9.2e-06             3.7e-05       8.9e-06
    ragged                  5.6e-06             2.2e-05       7.6e-06
    cluster (+-y, lone)     3.3e-06             1.3e-05       4.1e-06
    cell4 (+-y images)      6.3e-06             2.5e-05       6.3e-06
    no force block          9.7e-06             3.9e-05       5.6e-06
    energy_lin_ref          9.2e-06             3.7e-05       8.9e-06

Single entries: max|d| / max|ref| under 4 x float32 torch's own distance from float64 on the same inputs, the largest over
the parametrised set E = 1, 63, 257 of an entry and width (on one edge float32 torch can happen to be exact).  Measured:
rotate_in up to 3.8e-07 (float32 torch up to 1.9e-07), rotate_out up to 3.0e-07 (up to 1.8e-07), radial_gauss_dgrad up to 1.3e-07 (4.2e-07), edge_grad_to_atoms up to 1.5e-07
(3.7e-07), wigner_bwd on exact rows up to 1.7e-07 (up to 1.1e-07), on the device's own rows up to 1.5e-06 (up to 1.5e-06: the entry's formula in float32 torch
on the same fp32 rows).  Every figure is printed before it is asserted."""
import ctypes as C

import pytest
import torch

from adsorbdiff_amd import lib as _lib
from oracle import eqv2_oracle as Q
from tests import helpers_eqv2_grad_forces as G
from tests import helpers_eqv2_s2ef_train as S
from tests import helpers_eqv2_train as T
from tests.helpers_eqv2_ragged import one_system_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORCE_TOL = {"fixture": 3.7e-5, "ragged": 2.2e-5, "cluster": 1.3e-5, "cell4": 2.5e-5, "noforce": 3.9e-5, "linref": 3.7e-5}
_OPS, _CASES = {}, {}


# ------------------------------------------------------------------------------------------------ single entries
ES = (1, 63, 257)
WIDTHS = [(6, False), (4, False), (4, True)]     # (lmax, wide)
_RES = {}


def ops_for(L, wide=False):
    """(model, engine, EqOps) at lmax = L, mmax = 2, built once: C = 8 (2C = 16, NH V = 8, edge_channels = 8), or ``wide``:
    C = 40 and V = 36, so that 2C = 80 and NH V = 72 take the 64-channel panels of the two Wigner-term kernels into a second,
    partly filled trip, with the switch from x[src] to x[dst] inside the first."""
    from adsorbdiff_amd.eqv2_train_step import EqOps

    if (L, wide) not in _OPS:
        kw = dict(sphere_channels=40, attn_value_channels=36) if wide else {}
        m = S.ragged_model(lmax_list=[L], **kw).eval().to(DEV)
        eng = m.engine(DEV)
        _OPS[(L, wide)] = (m, eng, EqOps(eng))
    return _OPS[(L, wide)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def op_check(label, key, one, E):
    """``one(E) -> (device result, float64 reference, float32 reference)`` is run once for every E of the parametrised set;
    the bound of each case is 4 x the float32 reference's largest distance from float64 over that set (on one edge float32
    torch can happen to be exact; the set as a whole says what exact f32 arithmetic gives on these inputs)."""
    if key not in _RES:
        _RES[key] = {n: one(n) for n in ES}
    calib = max(G.rel_force_error(r32, r64) for _, r64, r32 in _RES[key].values())
    got, r64, r32 = _RES[key][E]
    e, bound = G.rel_force_error(got, r64), 4.0 * calib
    print(f"{label}[E={E}]: {e:.2e}  (float32 torch {G.rel_force_error(r32, r64):.2e}, over the set {calib:.2e}, bound {bound:.2e})")
    assert bool(torch.isfinite(got).all()), label
    assert e < bound, (label, E, e, bound)


def degree_major(t, L, M):
    """order-major rows [E, S_r, W] -> degree-major (the order of ``lm_list``)."""
    return t[:, torch.argsort(Q.order_major_perm(L, M))]


def wig_contraction(A_dm, Bfull, L, M):
    """[E, DR]: per degree the kept rows of A [E, S_r (degree-major), W] times the rows of B [E, S, W], summed over W."""
    out, r0 = [], 0
    for l in range(L + 1):
        nr = 2 * min(l, M) + 1
        out.append(torch.einsum("eic,ejc->eij", A_dm[:, r0:r0 + nr], Bfull[:, l * l:(l + 1) ** 2]).reshape(A_dm.shape[0], -1))
        r0 += nr
    return torch.cat(out, 1)


def wig_len(L, M):
    return sum((2 * min(l, M) + 1) * (2 * l + 1) for l in range(L + 1))


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("L, wide", WIDTHS)
def test_rotate_in_wigner_term_vs_einsum(L, wide, E):
    m, eng, ops = ops_for(L, wide)
    M, Cc, N = ops.M, ops.C, 7
    DR = wig_len(L, M)
    assert DR > 64 and (2 * Cc > 64 and (2 * Cc) % 64 != 0) == wide

    def one(E):
        g = torch.Generator().manual_seed(E + L)
        src, dst = torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)
        x, radial, dout = rnd(1, N, ops.S, Cc), rnd(2, E, ops.RW, 2 * Cc), rnd(3, E, ops.Sr, 2 * Cc)
        init = rnd(4, E, DR).float()

        def ref(dt):
            gw = dout.to(dt) * radial.to(dt)[:, T.radial_rows(L, M)]
            xcat = torch.cat([x.to(dt)[src], x.to(dt)[dst]], dim=2)
            return init.to(dt) + wig_contraction(degree_major(gw, L, M), xcat, L, M)

        outs = []
        for _ in range(2):
            dwig = init.clone().to(DEV)
            xd, rd, dd = x.float().to(DEV), radial.float().reshape(E, -1).contiguous().to(DEV), dout.float().to(DEV)
            sd, td = src.to(DEV, torch.int32), dst.to(DEV, torch.int32)
            _lib.check(eng.lib.adf_op_eq_rotate_in_bwd_wig(ops.h, xd.data_ptr(), sd.data_ptr(), td.data_ptr(), rd.data_ptr(),
                                                           dd.data_ptr(), E, dwig.data_ptr(), stream()))
            outs.append(dwig.cpu())
        assert torch.equal(outs[0], outs[1])
        return outs[0], ref(torch.float64), ref(torch.float32)

    op_check(f"rotate_in_bwd_wig[L={L}, 2C={2 * Cc}]", ("rotate_in", L, wide), one, E)


@pytest.mark.parametrize("only_l", [-1, 1])
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("L, wide", WIDTHS)
def test_rotate_out_wigner_term_vs_einsum(L, wide, E, only_l):
    m, eng, ops = ops_for(L, wide)
    M, NH, V, N = ops.M, ops.NH, ops.V, 7
    HV = NH * V
    DR = wig_len(L, M)
    assert (HV > 64 and HV % 64 != 0) == wide
    resc = Q.truncation_rescale(L, M, torch.float64)            # degree-major reduced

    def one(E):
        g = torch.Generator().manual_seed(E + L + 50)
        dst = torch.sort(torch.randint(0, N, (E,), generator=g)).values
        z, alpha, dagg = rnd(5, E, ops.Sr, HV), rnd(6, E, NH), rnd(7, N, ops.S, HV)
        init = rnd(8, E, DR).float()

        def ref(dt):
            a = z.to(dt) * alpha.to(dt).repeat_interleave(V, dim=1)[:, None, :]
            a_dm = degree_major(a, L, M) * resc.to(dt)[None, :, None]
            full = wig_contraction(a_dm, dagg.to(dt)[dst], L, M)
            if only_l >= 0:
                keep = torch.zeros(DR, dtype=torch.bool)
                off = wig_len(only_l - 1, M)
                keep[off:off + (2 * min(only_l, M) + 1) * (2 * only_l + 1)] = True
                full = full * keep.to(dt)[None]
            return init.to(dt) + full

        outs = []
        for _ in range(2):
            dwig = init.clone().to(DEV)
            zd, ad, gd, td = z.float().to(DEV), alpha.float().to(DEV), dagg.float().to(DEV), dst.to(DEV, torch.int32)
            _lib.check(eng.lib.adf_op_eq_rotate_out_bwd_wig(ops.h, zd.data_ptr(), ad.data_ptr(), NH, V, td.data_ptr(),
                                                            gd.data_ptr(), only_l, E, dwig.data_ptr(), stream()))
            outs.append(dwig.cpu())
        assert torch.equal(outs[0], outs[1])
        r64 = ref(torch.float64)
        if only_l >= 0:     # the other degrees are left alone, bit for bit
            untouched = r64 == init.double()
            assert bool(untouched.any()) and torch.equal(outs[0][untouched], init[untouched])
        return outs[0], r64, ref(torch.float32)

    op_check(f"rotate_out_bwd_wig[L={L}, NH V={HV}, only_l={only_l}]", ("rotate_out", L, wide, only_l), one, E)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("L", [6, 4])
def test_gauss_distance_gradient_vs_autograd(L, E):
    m, eng, ops = ops_for(L)
    rc, EC, NB = float(m.max_radius), ops.EC, ops.NB

    def one(E):
        vec = G.hard_vectors(E, rc, seed=E).to(DEV)
        dist = torch.empty(E, device=DEV)
        _lib.check(eng.lib.adf_op_eq_edge_dist(vec.data_ptr(), E, dist.data_ptr(), stream()))
        W0, dh0 = rnd(9, EC, NB + 2 * EC, scale=0.2), rnd(10, E, EC)
        init = rnd(11, E).float()

        def ref(dt):
            d = dist.cpu().to(dt).requires_grad_(True)
            h0 = S.live_basis(d, rc, dt) @ W0.to(dt)[:, :NB].t()
            (gd,) = torch.autograd.grad((h0 * dh0.to(dt)).sum(), d)
            return init.to(dt) + gd

        outs = []
        for _ in range(2):
            dd = init.clone().to(DEV)
            Wd, hd = W0.float().to(DEV), dh0.float().to(DEV)
            sc = torch.empty(NB * EC, device=DEV)
            _lib.check(eng.lib.adf_op_eq_radial_gauss_dgrad(ops.h, dist.data_ptr(), Wd.data_ptr(), Wd.stride(0), hd.data_ptr(), E,
                                                            dd.data_ptr(), sc.data_ptr(), sc.numel(), stream()))
            outs.append(dd.cpu())
        assert torch.equal(outs[0], outs[1])
        return outs[0], ref(torch.float64), ref(torch.float32)

    op_check(f"radial_gauss_dgrad[L={L}]", ("gauss", L), one, E)


@pytest.mark.parametrize("E", ES)
def test_edge_gradient_to_atoms_vs_index_add(E):
    lib = _lib.load()
    N = 9                                                # atom 8 has no edge

    def one(E):
        g = torch.Generator().manual_seed(E)
        dst = torch.sort(torch.randint(0, N - 1, (E,), generator=g)).values
        src = torch.randint(0, N - 1, (E,), generator=g)
        dvec = rnd(12, E, 3)
        eptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(dst, minlength=N).cumsum(0)]).to(DEV, torch.int32)
        sperm = torch.sort(src, stable=True).indices.to(DEV, torch.int32)
        sptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(src, minlength=N).cumsum(0)]).to(DEV, torch.int32)

        def ref(dt):
            return -torch.zeros(N, 3, dtype=dt).index_add_(0, src, dvec.to(dt)).index_add_(0, dst, -dvec.to(dt))

        outs = []
        for _ in range(2):
            f = torch.full((N, 3), 7.0, device=DEV)
            dv = dvec.float().to(DEV)
            _lib.check(lib.adf_op_eq_edge_grad_to_atoms(dv.data_ptr(), eptr.data_ptr(), sptr.data_ptr(), sperm.data_ptr(), N, E,
                                                        f.data_ptr(), stream()))
            outs.append(f.cpu())
        assert torch.equal(outs[0], outs[1])
        assert torch.equal(outs[0][8], torch.zeros(3))       # exactly zero
        return outs[0], ref(torch.float64), ref(torch.float32)

    op_check("edge_grad_to_atoms", ("to_atoms",), one, E)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("L", [6, 4])
def test_wigner_backward_vs_autograd(L, E):
    """(a) <G, wigner_from_rotation(frame(vec))[kept rows]> for a random G, on the rows of ``edge_frames(vec)``.  A random G
    is not invariant under the roll of the frame about the edge, so its gradient depends on how the frame rolls as the edge
    turns; the entry's answer is the one of a frame that does not roll, which ``transported_frames`` is at the point of
    evaluation (there it equals ``edge_frames``).  (b) a roll-invariant function of the rows, as the energy is, on the
    DEVICE's rows of the same vectors against the float64 autograd through the plain ``edge_frames`` of the yardstick: no
    transport, two different frames, the pole of the device's included.  The device's rows are fp32 rows of a frame whose
    angles were formed in fp32 - an input error float32 torch on exact rows does not have - so the calibration of (b) is the
    entry's own formula (``helpers_eqv2_grad_forces.wigner_bwd_torch``) in float32 torch on those same rows."""
    m, eng, ops = ops_for(L)
    M, rc = ops.M, float(m.max_radius)
    DR = wig_len(L, M)
    a, c = rnd(15, (L + 1) ** 2), rnd(16, (L + 1) ** 2)
    bw = rnd(17, L + 1, M + 1)

    def invariant(W, dt):
        """sum_l a_l^T W_l^T B_l W_l c_l with B_l diagonal and equal on +m and -m: invariant under the roll"""
        tot, off = 0.0, 0
        for l in range(L + 1):
            ml, n = min(l, M), 2 * l + 1
            Wl = W[:, off:off + (2 * ml + 1) * n].reshape(-1, 2 * ml + 1, n)
            Bl = torch.stack([bw[l, abs(mm)] for mm in range(-ml, ml + 1)]).to(dt)
            tot = tot + ((Wl @ a[l * l:(l + 1) ** 2].to(dt)) * Bl * (Wl @ c[l * l:(l + 1) ** 2].to(dt))).sum()
            off += (2 * ml + 1) * n
        return tot

    def run_device(vec0, wig, dwig, dd):
        E = vec0.shape[0]
        outs = []
        for _ in range(2):
            dvec = torch.empty(E, 3, device=DEV)
            v, w, gw, gd = vec0.to(DEV), wig.float().contiguous().to(DEV), dwig.float().contiguous().to(DEV), dd.float().to(DEV)
            _lib.check(eng.lib.adf_op_eq_wigner_bwd(ops.h, v.data_ptr(), w.data_ptr(), gw.data_ptr(), gd.data_ptr(), E,
                                                    dvec.data_ptr(), stream()))
            outs.append(dvec.cpu())
        assert torch.equal(outs[0], outs[1])
        return outs[0]

    def one_a(E):
        vec0 = G.hard_vectors(E, rc, seed=E + 7)
        Gm, dd = rnd(13, E, DR), rnd(14, E)

        def ref(dt):
            v = vec0.to(dt).clone().requires_grad_(True)
            W = G.kept_rows(Q.wigner_from_rotation(L, G.transported_frames(vec0.to(dt), v)), L, M)
            (gv,) = torch.autograd.grad((W * Gm.to(dt)).sum() + (v.norm(dim=1) * dd.to(dt)).sum(), v)
            return gv

        wig_o = G.kept_rows(Q.wigner_from_rotation(L, Q.edge_frames(vec0.double())), L, M)
        return run_device(vec0, wig_o, Gm, dd), ref(torch.float64), ref(torch.float32)

    def one_b(E):
        vec0 = G.hard_vectors(E, rc, seed=E + 7)
        dd = rnd(14, E)
        gen = torch.Generator().manual_seed(E)
        ei = torch.stack([torch.randint(0, 7, (E,), generator=gen), torch.sort(torch.randint(0, 7, (E,), generator=gen)).values])
        eng.set_edges(ei, vec0)
        try:
            wig_d = eng.export_graph(one_system_batch(torch.full((7,), 29.0)).to(DEV))[4].cpu()
        finally:
            eng.set_edges(None, None)
        assert wig_d.shape == (E, DR)
        Wleaf = wig_d.double().requires_grad_(True)
        (dwig,) = torch.autograd.grad(invariant(Wleaf, torch.float64), Wleaf)
        v = vec0.double().clone().requires_grad_(True)
        W = G.kept_rows(Q.wigner_from_rotation(L, Q.edge_frames(v)), L, M)
        (r64,) = torch.autograd.grad(invariant(W, torch.float64) + (v.norm(dim=1) * dd).sum(), v)
        r32 = G.wigner_bwd_torch(L, M, vec0, wig_d, dwig.float(), dd.float(), torch.float32)
        # the formula itself, in float64 on exact rows, is the autograd's derivative
        exact = G.kept_rows(Q.wigner_from_rotation(L, Q.edge_frames(vec0.double())), L, M).requires_grad_(True)
        (dex,) = torch.autograd.grad(invariant(exact, torch.float64), exact)
        assert G.rel_force_error(G.wigner_bwd_torch(L, M, vec0, exact.detach(), dex, dd, torch.float64), r64) < 1e-12
        return run_device(vec0, wig_d, dwig, dd), r64, r32

    op_check(f"wigner_bwd random G [L={L}]", ("wigner_a", L), one_a, E)
    op_check(f"wigner_bwd invariant, device rows [L={L}]", ("wigner_b", L), one_b, E)


# ------------------------------------------------------------------------------------------------ whole forces
def case(name):
    """name -> dict(model on the device, batch (cpu), batch on the device, graph exported by the device, float64 and float32
    yardstick (energy, forces), device (energy, forces)); built once."""
    if name in _CASES:
        return _CASES[name]
    edges = None
    if name == "ragged":
        m = S.ragged_model().eval()
        b, ei, vec = S.ragged_case()
        edges = (ei, vec)
    elif name == "cluster":
        m = S.small_train_model().eval()
        b, ei, vec = G.cluster_batch()
        edges = (ei, vec)
    elif name == "cell4":
        m = S.small_train_model().eval()
        b = G.cell4_batch()
    else:
        kw = {"fixture": {}, "noforce": dict(regress_forces=False), "linref": dict(use_energy_lin_ref=True)}[name]
        m = S.small_train_model(**kw).eval()
        b = S.fixture_case()[0]
    m = m.to(DEV)
    bd = b.clone().to(DEV)
    eng = m.engine(DEV)
    if edges is not None:
        eng.set_edges(*edges)
    graph = tuple(t.cpu() for t in eng.export_graph(bd))
    m.force_mode = "energy_gradient"
    out = m(bd)
    out2 = m(bd)
    r64 = G.reference_on_graph(m, b, graph)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)        # the float32 calibration in one fixed summation order: its net force is a bound below
    try:
        r32 = G.reference_on_graph(m, b, graph, torch.float32)
    finally:
        torch.set_num_threads(threads)
    _CASES[name] = dict(model=m, batch=b, dev_batch=bd, graph=graph, r64=r64, r32=r32, out=out, out2=out2)
    return _CASES[name]


@pytest.mark.parametrize("name", ["fixture", "ragged", "cluster", "cell4", "noforce", "linref"])
def test_forces_against_the_float64_yardstick(name):
    c = case(name)
    e64, f64 = c["r64"]
    f = c["out"]["forces"]
    assert set(c["out"]) == {"energy", "forces"} and f.shape == f64.shape and f.dtype == torch.float32
    err, calib = G.rel_force_error(f, f64), G.rel_force_error(c["r32"][1], f64)
    de = float((c["out"]["energy"].double().cpu() - e64).abs().max() / e64.abs().max())
    print(f"{name}: forces {err:.2e} (float32 yardstick {calib:.2e}, bound {FORCE_TOL[name]:.1e}); max|F| {float(f64.abs().max()):.3e}; "
          f"energy {de:.2e}; E = {c['graph'][1].numel()}")
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(c["out"]["energy"]).all())
    assert err < FORCE_TOL[name], (name, err)
    assert de < 1e-5
    src, dst = c["graph"][1].long(), c["graph"][2].long()
    lone = [i for i in range(f.shape[0]) if i not in set(src.tolist()) | set(dst.tolist())]
    assert (name == "cluster") == bool(lone)
    for i in lone:
        assert torch.equal(f[i].cpu(), torch.zeros(3)), (name, i)      # exactly 0.0
    if name in ("cluster", "cell4"):                                  # edges on the pole of the device's frame are there
        v = c["graph"][3]
        assert int(((v[:, 0] == 0) & (v[:, 2] == 0)).sum()) >= 2
    if name == "noforce":
        assert not hasattr(c["model"], "force_block")
    if name == "linref":
        # the frozen table shifts the energy and leaves the forces alone, bit for bit
        assert torch.equal(f, case("fixture")["out"]["forces"])
        assert not torch.equal(c["out"]["energy"], case("fixture")["out"]["energy"])


def test_forces_are_continuous_across_the_pole():
    """The cluster's two edges between atoms 0 and 1 exactly on the pole (rho = 0) and tilted off it by rho = 1e-6, every
    other edge as it was.  (Moving atom 1 itself by 1.5e-6 changes the float64 forces by 2.3e-5 of max|F| through the other
    edges' distances - the basis is 0.02 wide - which says nothing about the pole; the tilt alone changes them by 2.9e-7.)"""
    c = case("cluster")
    m = c["model"]
    _, ei, vec = G.cluster_batch()
    polar = (vec[:, 0] == 0) & (vec[:, 2] == 0)
    assert int(polar.sum()) == 2 and torch.equal(vec, c["graph"][3])
    tilted = vec.clone()
    tilted[polar, 0] = 1.5e-6 * torch.sign(vec[polar, 1])
    rho = tilted[polar][:, [0, 2]].norm(dim=1) / tilted[polar].norm(dim=1)
    assert bool(((rho > 0.9e-6) & (rho < 1.1e-6)).all())
    eng = m.engine(DEV, refresh=False)
    eng.set_edges(ei, tilted)
    try:
        off = m(c["dev_batch"])
    finally:
        eng.set_edges(ei, vec)
    on = c["out"]
    d = float((off["forces"] - on["forces"]).abs().max() / on["forces"].abs().max())
    print(f"pole continuity: rho = 0 against rho = {float(rho[0]):.2e}: {d:.2e} of max|F| (bound {FORCE_TOL['cluster']:.1e})")
    assert bool(torch.isfinite(off["forces"]).all()) and bool(torch.isfinite(on["forces"]).all())
    assert bool(torch.isfinite(off["energy"]).all())
    assert d < FORCE_TOL["cluster"]


def test_reported_energy():
    """Bit for bit the energy of ``EqV2S2EFTrainStep.forward`` in eval(), and within the README's 1.3e-6 of max|E| of the
    direct mode's ``model(batch)["energy"]``."""
    from adsorbdiff_amd.eqv2_train_step import EqV2S2EFTrainStep

    c = case("fixture")
    m, bd = c["model"], c["dev_batch"]
    m.force_mode = "direct"
    try:
        assert not m.training
        with torch.no_grad():
            e_train = EqV2S2EFTrainStep(m, DEV).forward(bd)[0]
        direct = m(bd)
    finally:
        m.force_mode = "energy_gradient"
    assert torch.equal(e_train, c["out"]["energy"])
    d = float((direct["energy"] - c["out"]["energy"]).abs().max() / direct["energy"].abs().max())
    print(f"energy of the gradient mode against the direct mode: {d:.2e} of max|E| (bound 1.3e-6)")
    assert d <= 1.3e-6


def test_bit_reproducible_and_independent_of_batch_mates():
    from adsorbdiff_amd.data import data_list_collater
    from adsorbdiff_amd.engine import image_repeats

    for name in ("fixture", "ragged", "cell4"):
        c = case(name)
        assert torch.equal(c["out"]["forces"], c["out2"]["forces"]) and torch.equal(c["out"]["energy"], c["out2"]["energy"])
    c = case("fixture")
    m, b = c["model"], c["batch"]
    alone = data_list_collater(b.to_data_list()[1:])
    assert image_repeats(alone, m.cutoff) == image_repeats(b, m.cutoff)       # both runs search the same images
    out = m(alone.to(DEV))
    n0 = int(b.natoms[0])
    assert torch.equal(out["forces"], c["out"]["forces"][n0:]) and torch.equal(out["energy"], c["out"]["energy"][1:])


@pytest.mark.parametrize("name", ["fixture", "ragged", "cluster", "cell4"])
def test_net_force_per_system(name):
    """With a fixed edge set the exact sum is zero; the device's is no larger than 4 x the float32 yardstick's own."""
    c = case(name)
    idx = c["batch"].batch.long()
    B = int(c["batch"].natoms.numel())
    net = lambda f: torch.zeros(B, 3, dtype=torch.float64).index_add_(0, idx, f.double().cpu()).norm(dim=1)
    dev, y32 = net(c["out"]["forces"]), net(c["r32"][1])
    print(f"{name}: net force per system: device {dev.tolist()}  float32 yardstick {y32.tolist()}")
    assert bool((dev <= 4.0 * y32).all()), (name, dev, y32)


def test_nothing_else_moved():
    """The direct mode before and after switching the mode back and forth, and one step of each training step before and
    after an energy-gradient call in the same process: the same bits."""
    from adsorbdiff_amd.eqv2_train_step import EqV2S2EFTrainStep, EqV2TrainStep

    m = S.small_train_model().to(DEV)
    b = S.fixture_case()[0]
    bd = b.clone().to(DEV)
    m.eval()
    before = {k: v.clone() for k, v in m(bd).items()}
    m.force_mode = "energy_gradient"
    grad_out = m(bd)
    m.force_mode = "direct"
    after = m(bd)
    assert set(before) == set(after) == {"energy", "forces"}
    assert torch.equal(before["energy"], after["energy"]) and torch.equal(before["forces"], after["forces"])
    assert not torch.equal(grad_out["forces"], after["forces"])

    def s2ef_step():
        m.train()
        step = EqV2S2EFTrainStep(m, DEV, normalizers=S.NORMALIZERS, **S.COEFFICIENTS)
        step.zero_grad()
        loss = step.loss_and_grad(bd)
        return loss.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    den = T.train_model("small").to(DEV)
    db, dei, dvec = T.ragged_case()
    dbd = db.clone().to(DEV)
    den.engine(DEV).set_edges(dei, dvec)
    targets = T.make_targets(int(db.natoms.numel()))

    def den_step():
        step = EqV2TrainStep(den, DEV, igso3=T.igso3_tables()[0])
        step.zero_grad()
        loss = step.loss_and_grad(dbd, targets)
        return loss.clone(), {k: p.grad.clone() for k, p in den.named_parameters() if p.grad is not None}

    l1, g1 = s2ef_step()
    d1, h1 = den_step()
    m.eval()
    m.force_mode = "energy_gradient"
    again = m(bd)
    m.force_mode = "direct"
    assert torch.equal(again["forces"], grad_out["forces"]) and torch.equal(again["energy"], grad_out["energy"])
    l2, g2 = s2ef_step()
    d2, h2 = den_step()
    assert torch.equal(l1, l2) and g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert torch.equal(d1, d2) and h1.keys() == h2.keys() and all(torch.equal(h1[k], h2[k]) for k in h1)
    assert len(g1) > 50 and len(h1) > 50


# ------------------------------------------------------------------------------------------------ ml_relax, validate
def relax_batch():
    """2 systems x 12 atoms: a jittered 2 x 2 x 3 grid in a 5.2 x 5.2 x 14 cell, the bottom layer fixed."""
    from adsorbdiff_amd.data import Batch, data_list_collater

    systems = []
    for s in range(2):
        g = torch.Generator().manual_seed(40 + s)
        grid = torch.tensor([[i, j, k] for k in range(3) for i in range(2) for j in range(2)], dtype=torch.float32) * 2.6
        d = Batch()
        d.pos = grid + 0.5 + 0.3 * (torch.rand(12, 3, generator=g) - 0.5)
        d.atomic_numbers = torch.tensor([29.0] * 8 + [8.0, 6.0, 1.0, 1.0])
        d.tags = torch.tensor([0] * 4 + [1] * 4 + [2] * 4)
        d.fixed = torch.tensor([1] * 4 + [0] * 8)
        d.cell = torch.tensor([[[5.2, 0.0, 0.0], [0.0, 5.2, 0.0], [0.0, 0.0, 14.0]]])
        d.natoms = torch.tensor([12])
        d.batch = torch.zeros(12, dtype=torch.long)
        d.sid = [str(s)]
        systems.append(d)
    return data_list_collater(systems)


@pytest.mark.parametrize("regress_forces", [True, False])
def test_ml_relax_and_validate(regress_forces):
    from adsorbdiff_amd.ml_relaxation import ml_relax
    from adsorbdiff_amd.trainer import ForcesTrainer
    from tests.helpers_s2ef import RELAX_KW, small_model

    m = small_model(RELAX_KW, regress_forces=regress_forces).to(DEV)
    tr = ForcesTrainer(m, device=DEV)
    b = S.with_targets(relax_batch(), seed=5)
    if not regress_forces:      # the parent's answer for an energy-only model
        with pytest.raises(NotImplementedError, match="the s2ef metrics need forces"):
            tr.validate([b.clone()])
    m.force_mode = "energy_gradient"
    start = b.pos.clone()
    out = ml_relax(b.clone().to(DEV), tr, steps=3, fmax=1e-4, relax_opt={"memory": 5}, save_full_traj=False, device=DEV)
    fixed = out.fixed.cpu() == 1
    assert bool(torch.isfinite(out.pos).all()) and bool(torch.isfinite(out.force).all()) and bool(torch.isfinite(out.y).all())
    assert torch.equal(out.pos.cpu()[fixed], start[fixed]) and not torch.equal(out.pos.cpu()[~fixed], start[~fixed])
    final = m(out.clone())
    assert torch.equal(final["forces"], out.force) and torch.equal(final["energy"].reshape(-1), out.y.reshape(-1))
    res = tr.validate([b.clone()])
    names = set(res) - {"loss"}
    print("validate:", {k: f"{v['metric']:.3e}" for k, v in sorted(res.items())})
    assert len(names) == 8 and "forces_mae" in names and all(torch.isfinite(torch.tensor(v["metric"])) for v in res.values())
