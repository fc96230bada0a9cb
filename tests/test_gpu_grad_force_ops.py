"""Every dual operator of the training step on energy-gradient forces (csrc/dual_ops.hip, csrc/message_dual.hip) on its own.

Reference: the operator's primal lines in torch, ``torch.func.jvp`` for (y, y_dot), and float64 autograd of
sum(y * y_bar) + sum(y_dot * y_dot_bar) over the inputs AND their tangents - which is the dual backward rule
x_bar = J^T y_bar + (d/dx [J x_dot])^T y_dot_bar, x_dot_bar = J^T y_dot_bar.  The entries are called the way
adsorbdiff_amd/train_step.py calls them: dual operands stacked (primal block, then tangent block), nrm in the right half of a
[x | nrm] buffer.

Bound: an output is within 1e-5 of its largest entry (the operator tests' budget); where the same expression evaluated with
torch in float32 is itself further away, 4 x that deviation.  Each case prints both."""
import ctypes as C
import math

import pytest
import torch

from oracle import painn_oracle as O
from tests import helpers_grad_force_train as HG
from tests import helpers_train as HT
from tests.test_gpu_train_ops import dev, gen, ok, ops, s

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional
ROWS, WIDTHS = (1, 63, 257), (128, 192)
GRID = [(n, h) for n in ROWS for h in WIDTHS]


def dual_refs(fn, inputs, tangents, upstream, upstream_t, dtype):
    """(outputs, output tangents, input gradients, input-tangent gradients) of ``fn`` in ``dtype`` on the CPU."""
    xs = [x.detach().cpu().to(dtype).requires_grad_(True) for x in inputs]
    ts = [t.detach().cpu().to(dtype).requires_grad_(True) for t in tangents]
    ys, yds = torch.func.jvp(fn, tuple(xs), tuple(ts))
    ys, yds = (list(v) if isinstance(v, (tuple, list)) else [v] for v in (ys, yds))
    total = sum((y * u.to(dtype)).sum() for y, u in zip(ys, upstream)) + sum((y * u.to(dtype)).sum() for y, u in zip(yds, upstream_t))
    grads = torch.autograd.grad(total, xs + ts, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, xs + ts)]
    return [y.detach() for y in ys], [y.detach() for y in yds], grads[:len(xs)], grads[len(xs):]


def both(fn, inputs, tangents, upstream, upstream_t):
    return dual_refs(fn, inputs, tangents, upstream, upstream_t, torch.float64), \
        dual_refs(fn, inputs, tangents, upstream, upstream_t, torch.float32)


def check(op, shape, got, ref64, ref32):
    got, ref64, ref32 = (t.detach().double().cpu().reshape(-1) for t in (got, ref64, ref32))
    assert got.shape == ref64.shape, (op, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), (op, shape, "non-finite output")
    scale = float(ref64.abs().max())
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, (op, shape)
        return
    err, e32 = float((got - ref64).abs().max()) / scale, float((ref32 - ref64).abs().max()) / scale
    print(f"{op} {shape}: error {err:.2e} float32 torch {e32:.2e}")
    assert err <= max(1e-5, 4.0 * e32), (op, shape, err, e32)


def stack(a, b):
    return dev(torch.stack([a, b]))


def out2(*shape):
    return torch.full((2, *shape), float("nan"), dtype=torch.float32, device=DEV)


def halves(t):
    torch.cuda.synchronize()
    t = t.cpu()
    return t[0], t[1]


# ------------------------------------------------------------------------------------------------ elementwise operators
@pytest.mark.parametrize("N,H", GRID)
def test_ssilu_dual(N, H):
    g = gen(71, N, H)
    h, hd, dy, dyd = (torch.randn(N, H, generator=g) * sc for sc in (3.0, 1.0, 1.0, 1.0))
    h2, dy2, y2, dh2 = stack(h, hd), stack(dy, dyd), out2(N, H), out2(N, H)
    lib = ops().lib
    ok(lib.adf_op_ssilu_dual_fwd(h2.data_ptr(), y2.data_ptr(), N * H, s()))
    ok(lib.adf_op_ssilu_dual_bwd(h2.data_ptr(), dy2.data_ptr(), dh2.data_ptr(), N * H, s()))
    r64, r32 = both(O.ssilu, [h], [hd], [dy], [dyd])
    (y, yd), (gh, ghd) = halves(y2), halves(dh2)
    for name, got, k, i in (("y", y, 0, 0), ("y_dot", yd, 1, 0), ("dh", gh, 2, 0), ("dh_dot", ghd, 3, 0)):
        check("ssilu_dual " + name, (N, H), got, r64[k][i], r32[k][i])


@pytest.mark.parametrize("N,H", GRID)
def test_layernorm_dual(N, H):
    g = gen(72, N, H)
    x, xd = torch.randn(N, H, generator=g) * 2.0 + 0.5, torch.randn(N, H, generator=g)
    w, b = 1.0 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    dy, dyd = torch.randn(N, H, generator=g), torch.randn(N, H, generator=g)
    dx0 = torch.randn(2, N, H, generator=g)
    x2, dy2, y2, dx2 = stack(x, xd), stack(dy, dyd), out2(N, H), dev(dx0)
    wd, bd = dev(w), dev(b)
    stats, dw, db = torch.empty(N, 2, device=DEV), out2(H)[0], out2(H)[0]
    lib = ops().lib
    ok(lib.adf_op_layernorm_dual_fwd(x2.data_ptr(), wd.data_ptr(), bd.data_ptr(), y2.data_ptr(), stats.data_ptr(), N, H, s()))
    ok(lib.adf_op_layernorm_dual_bwd(x2.data_ptr(), wd.data_ptr(), stats.data_ptr(), dy2.data_ptr(), dx2.data_ptr(), dw.data_ptr(),
                                     db.data_ptr(), N, H, ops().scratch(512 * 2 * H + 16).data_ptr(), s()))

    def fn(x_, w_, b_):
        # F.layer_norm spelled out: reverse mode through the fused operator's forward-mode rule does not reach x
        # (measured on the CPU: its x gradient misses the tangent's dependence on the moments)
        mu = x_.mean(1, keepdim=True)
        var = ((x_ - mu) ** 2).mean(1, keepdim=True)
        return (x_ - mu) / torch.sqrt(var + 1e-5) * w_ + b_

    z = torch.zeros
    r64, r32 = both(fn, [x, w, b], [xd, z(H), z(H)], [dy], [dyd])
    (y, yd), (gx, gxd) = halves(y2), halves(dx2 - dev(dx0))
    check("layernorm_dual y", (N, H), y, r64[0][0], r32[0][0])
    check("layernorm_dual y_dot", (N, H), yd, r64[1][0], r32[1][0])
    check("layernorm_dual dx (accumulated)", (N, H), gx, r64[2][0], r32[2][0])
    check("layernorm_dual dx_dot (accumulated)", (N, H), gxd, r64[3][0], r32[3][0])
    check("layernorm_dual dw", (N, H), dw.cpu(), r64[2][1], r32[2][1])
    check("layernorm_dual db", (N, H), db.cpu(), r64[2][2], r32[2][2])


@pytest.mark.parametrize("N,H", GRID)
def test_vdot_dual(N, H):
    g = gen(73, N, H)
    vv, vvd = torch.randn(N, 3, 2 * H, generator=g), torch.randn(N, 3, 2 * H, generator=g)
    ddot, ddotd, dn, dnd = (torch.randn(N, H, generator=g) for _ in range(4))
    dv1, dv1d = torch.randn(N, 3, H, generator=g), torch.randn(N, 3, H, generator=g)
    vv2, ddot2, dv1_2 = stack(vv, vvd), stack(ddot, ddotd), stack(dv1, dv1d)
    cat2, dcat2 = out2(N, 2 * H), out2(N, 2 * H)          # nrm / dnrm live in the right halves
    dcat2[:, :, H:] = torch.stack([dn, dnd]).to(DEV)
    dot2, dvv2 = out2(N, H), out2(N, 3, 2 * H)
    lib = ops().lib
    ok(lib.adf_op_vdot_dual_fwd(vv2.data_ptr(), dot2.data_ptr(), cat2.data_ptr() + 4 * H, 2 * H, N, H, C.c_float(1e-8), s()))
    ok(lib.adf_op_vdot_dual_bwd(vv2.data_ptr(), cat2.data_ptr() + 4 * H, 2 * H, ddot2.data_ptr(), dcat2.data_ptr() + 4 * H, 2 * H,
                                dv1_2.data_ptr(), dvv2.data_ptr(), N, H, s()))

    def fn(v):
        v1, v2 = v[..., :H], v[..., H:]
        return (v1 * v2).sum(1) / math.sqrt(H), torch.sqrt((v2 * v2).sum(1) + 1e-8), v1

    r64, r32 = both(fn, [vv], [vvd], [ddot, dn, dv1], [ddotd, dnd, dv1d])
    torch.cuda.synchronize()
    assert bool(torch.isnan(cat2[:, :, :H]).all()), "the kernel wrote outside the right half of [x | nrm]"
    (d, dd_), (n_, nd) = halves(dot2), halves(cat2[:, :, H:].contiguous())
    (gv, gvd) = halves(dvv2)
    for name, got, k, i in (("dot", d, 0, 0), ("dot_dot", dd_, 1, 0), ("nrm", n_, 0, 1), ("nrm_dot", nd, 1, 1),
                            ("dvv", gv, 2, 0), ("dvv_dot", gvd, 3, 0)):
        check("vdot_dual " + name, (N, H), got, r64[k][i], r32[k][i])


@pytest.mark.parametrize("N,H", GRID)
def test_update_out_dual(N, H):
    g = gen(74, N, H)
    rn = lambda *sh: torch.randn(*sh, generator=g)   # noqa: E731
    x1, x1d, vec1, vec1d = rn(N, H), rn(N, H), rn(N, 3, H), rn(N, 3, H)
    a, ad, dot, dotd, vv, vvd = rn(N, 3 * H), rn(N, 3 * H), rn(N, H), rn(N, H), rn(N, 3, 2 * H), rn(N, 3, 2 * H)
    gx, gxd, gv, gvd = rn(N, H), rn(N, H), rn(N, 3, H), rn(N, 3, H)
    scale = 1.07
    x1_2, vec1_2, a2, dot2, vv2 = stack(x1, x1d), stack(vec1, vec1d), stack(a, ad), stack(dot, dotd), stack(vv, vvd)
    gx2, gv2 = stack(gx, gxd), stack(gv, gvd)
    xo, vo = out2(N, H), out2(N, 3, H)
    da, ddot, dv1, dx1, dvec1 = out2(N, 3 * H), out2(N, H), out2(N, 3, H), out2(N, H), out2(N, 3, H)
    lib = ops().lib
    ok(lib.adf_op_update_out_dual_fwd(x1_2.data_ptr(), vec1_2.data_ptr(), a2.data_ptr(), dot2.data_ptr(), vv2.data_ptr(),
                                      C.c_float(scale), xo.data_ptr(), vo.data_ptr(), N, H, s()))
    ok(lib.adf_op_update_out_dual_bwd(a2.data_ptr(), dot2.data_ptr(), vv2.data_ptr(), C.c_float(scale), gx2.data_ptr(),
                                      gv2.data_ptr(), da.data_ptr(), ddot.data_ptr(), dv1.data_ptr(), dx1.data_ptr(),
                                      dvec1.data_ptr(), N, H, s()))

    def fn(x1_, vec1_, a_, dot_, v1_):
        a1, a2_, a3 = a_[:, :H], a_[:, H:2 * H], a_[:, 2 * H:]
        return (x1_ + (a1 + a2_ * dot_) / math.sqrt(2.0)) * scale, vec1_ + a3[:, None, :] * v1_

    r64, r32 = both(fn, [x1, vec1, a, dot, vv[..., :H]], [x1d, vec1d, ad, dotd, vvd[..., :H]], [gx, gv], [gxd, gvd])
    got = {"x2": halves(xo), "vec2": halves(vo), "dx1": halves(dx1), "dvec1": halves(dvec1), "da": halves(da),
           "ddot": halves(ddot), "dv1": halves(dv1)}
    for name, k in (("x2", 0), ("vec2", 1)):
        check(f"update_out_dual {name}", (N, H), got[name][0], r64[0][k], r32[0][k])
        check(f"update_out_dual {name}_dot", (N, H), got[name][1], r64[1][k], r32[1][k])
    for name, k in (("dx1", 0), ("dvec1", 1), ("da", 2), ("ddot", 3), ("dv1", 4)):
        check(f"update_out_dual {name}", (N, H), got[name][0], r64[2][k], r32[2][k])
        check(f"update_out_dual {name}_dot", (N, H), got[name][1], r64[3][k], r32[3][k])


# ------------------------------------------------------------------------------------------------ edge tangents and the basis
def _graph(name):
    m = HG.make_config_model(name).to(DEV)
    bd = HG.make_config_batch(name).to(DEV)
    eng = m.engine(DEV)
    E = eng.build_graph(bd)
    _, _, _, es, ed, dist, unit = eng.export_graph()
    return m, bd, eng, E, es.cpu().long(), ed.cpu().long(), dist.cpu(), unit.cpu()


def _reverse_rows(es, ed, dist, unit):
    """rev[e]: the row of the same pair in the partner's segment (same distance bits, negated unit vector)."""
    key = {}
    rows = zip(es.tolist(), ed.tolist(), dist.view(torch.int32).tolist(), [tuple(r) for r in unit.tolist()])
    for e, (a, b, d, u) in enumerate(rows):
        key[(a, b, d, u)] = e
    rev = torch.empty(es.numel(), dtype=torch.long)
    rows = zip(es.tolist(), ed.tolist(), dist.view(torch.int32).tolist(), [tuple(-c for c in r) for r in unit.tolist()])
    for e, (a, b, d, u) in enumerate(rows):
        rev[e] = key[(b, a, d, tuple(c + 0.0 for c in u))]
    return rev


@pytest.mark.parametrize("name", ["single", "ragged", "isolated", "hub"])
def test_message_dual_kernels_on_the_engine_graph(name):
    """adf_op_edge_tangent, adf_op_rbf_dual and the two message kernels on the engine's exported graph: ``single`` runs the
    vec == 0 variant (its only layer), ``ragged`` a 1-atom adsorbate and self-image edges, ``isolated`` an empty CSR segment,
    ``hub`` in-degrees above 256.  rbfh is a function of the distance (as the model's is), so that the two rows of a pair
    carry the same values: the backward kernel reads them through the reverse rows and writes d(rbfh) at the segment's own
    rows, which the reference's rows are mapped to."""
    m, bd, eng, E, es, ed, dist, unit = _graph(name)
    N, H, R = int(bd.pos.shape[0]), m.hidden_channels, m.num_rbf
    H3 = 3 * H
    g = gen(75, N, H)
    rn = lambda *sh: torch.randn(*sh, generator=g)   # noqa: E731
    lib, h = ops().lib, eng.handle
    # ---- edge tangents and the dual basis
    v = rn(N, 3)
    e_tan = torch.full((E, 4), float("nan"), device=DEV)
    rbf2 = torch.full((2 * E, R), float("nan"), device=DEV)
    ok(lib.adf_op_edge_tangent(h, dev(v).data_ptr(), e_tan.data_ptr(), E, s()))
    ok(lib.adf_op_rbf_dual(h, e_tan.data_ptr(), rbf2.data_ptr(), E, s()))
    torch.cuda.synchronize()
    mu = m.radial_basis.rbf.offset.detach().cpu()
    res = []
    for dt in (torch.float64, torch.float32):
        u_, d_, dl = unit.to(dt), dist.to(dt), (v[es] - v[ed]).to(dt)
        dd = (u_ * dl).sum(1)
        ud = (dl - u_ * dd[:, None]) / d_[:, None]
        rb, rbd = torch.func.jvp(lambda t: HG.GF.radial_basis(t, float(m.cutoff), mu.to(dt)), (d_,), (dd,))
        res.append((torch.cat([ud, dd[:, None]], 1), rb, rbd))
    check("edge_tangent", (name, E), e_tan.cpu(), res[0][0], res[1][0])
    check("rbf_dual rbf", (name, E, R), rbf2[:E].cpu(), res[0][1], res[1][1])
    check("rbf_dual rbf_dot", (name, E, R), rbf2[E:].cpu(), res[0][2], res[1][2])
    rev = _reverse_rows(es, ed, dist, unit)
    tan = e_tan.cpu()
    assert torch.equal(tan[rev, 3], tan[:, 3]) and torch.equal(tan[rev, :3], -tan[:, :3]), "a pair's tangents must mirror"
    # ---- the message kernels
    vec_is_zero = name == "single"
    freq, phase = 0.5 + rn(H3).abs(), rn(H3)
    dd = tan[:, 3]
    arg = dist[:, None] * freq[None, :] + phase[None, :]
    rbfh, rbfhd = torch.sin(arg), torch.cos(arg) * freq[None, :] * dd[:, None]
    xh, xhd, x, xd = rn(N, H3), rn(N, H3), rn(N, H), rn(N, H)
    vec, vecd = (torch.zeros(N, 3, H), torch.zeros(N, 3, H)) if vec_is_zero else (rn(N, 3, H), rn(N, 3, H))
    gx, gxd, gv, gvd = rn(N, H), rn(N, H), rn(N, 3, H), rn(N, 3, H)
    xh2, x2, vec2 = stack(xh, xhd), stack(x, xd), None if vec_is_zero else stack(vec, vecd)
    rbfh2 = dev(torch.cat([rbfh, rbfhd]))
    gx2, gv2 = stack(gx, gxd), stack(gv, gvd)
    x1_2, vec1_2 = out2(N, H), out2(N, 3, H)
    dxh2, drbfh2, dvec2, dx2 = out2(N, H3), torch.full((2 * E, H3), float("nan"), device=DEV), out2(N, 3, H), out2(N, H)
    ok(lib.adf_op_message_dual_fwd(h, e_tan.data_ptr(), xh2.data_ptr(), vec2.data_ptr() if vec2 is not None else None,
                                   rbfh2.data_ptr(), x2.data_ptr(), x1_2.data_ptr(), vec1_2.data_ptr(), 1 if vec_is_zero else 0,
                                   E, s()))
    ok(lib.adf_op_message_dual_bwd(h, e_tan.data_ptr(), xh2.data_ptr(), vec2.data_ptr() if vec2 is not None else None,
                                   rbfh2.data_ptr(), gx2.data_ptr(), gv2.data_ptr(), dxh2.data_ptr(), drbfh2.data_ptr(),
                                   dvec2.data_ptr() if vec2 is not None else None, dx2.data_ptr(), 1 if vec_is_zero else 0, E, s()))

    def fn(xh_, vec_, rbfh_, u_, x_):
        xa, xb, xc = xh_[:, :H], xh_[:, H:2 * H], xh_[:, 2 * H:]
        ra, rb, rc = rbfh_[:, :H], rbfh_[:, H:2 * H], rbfh_[:, 2 * H:]
        sx = torch.zeros_like(x_).index_add_(0, ed, xa[es] * ra)
        msg = vec_[es] * (xb[es] * rb)[:, None, :] / math.sqrt(3.0) + (xc[es] * rc)[:, None, :] * u_[:, :, None]
        dv = torch.zeros_like(vec_).index_add_(0, ed, msg) / math.sqrt(H)
        return (x_ + sx) / math.sqrt(2.0), vec_ + dv

    ud = tan[:, :3]
    r64, r32 = both(fn, [xh, vec, rbfh, unit, x], [xhd, vecd, rbfhd, ud, xd], [gx, gv], [gxd, gvd])
    shape = (name, N, E, H)
    for nm, buf, k in (("x1", x1_2, 0), ("vec1", vec1_2, 1)):
        a, b = halves(buf)
        check(f"message_dual_fwd {nm}", shape, a, r64[0][k], r32[0][k])
        check(f"message_dual_fwd {nm}_dot", shape, b, r64[1][k], r32[1][k])
    outs = [("dxh", dxh2, 0), ("dx", dx2, 4)] + ([] if vec_is_zero else [("dvec", dvec2, 1)])
    for nm, buf, k in outs:
        a, b = halves(buf)
        check(f"message_dual_bwd {nm}", shape, a, r64[2][k], r32[2][k])
        check(f"message_dual_bwd {nm}_dot", shape, b, r64[3][k], r32[3][k])
    torch.cuda.synchronize()
    dr = drbfh2.cpu()
    check("message_dual_bwd drbfh", shape, dr[:E], r64[2][2][rev], r32[2][2][rev])
    check("message_dual_bwd drbfh_dot", shape, dr[E:], r64[3][2][rev], r32[3][2][rev])
    if name == "isolated":
        deg = torch.bincount(ed, minlength=N)
        assert int((deg == 0).sum()) > 0
    if name == "hub":
        assert int(torch.bincount(ed, minlength=N).max()) > 256
