"""The edge-side training operators of the EquiformerV2 denoiser (adf_op_eq_*, csrc/eqv2_train.hip), one by one, forward and
backward, against float64 autograd of the matching piece of oracle/eqv2_oracle.py - on the ragged graph (in-degrees 0, 1,
K, K + 1, 63, 64, 65, 128; self-loops; polar edges), with the DEVICE's own edge list and Wigner rows, for the generic
(`small`) and the wide (`mfma`) model.

Bounds: forward 1e-5 (Frobenius ratio); every returned gradient under max(1e-4, 10 x the float32 oracle piece's own
distance from the float64 one), printed.  Two calls give the same bits."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_eqv2_train as T
from oracle import eqv2_oracle as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CASES = {}


def case(name):
    """(ops, graph, context of CPU index tensors) of a model on the ragged graph; built once per model."""
    if name in _CASES:
        return _CASES[name]
    from adsorbdiff_amd.eqv2_train_step import EqGraph, EqOps

    m = T.train_model(name).to(DEV)
    b, ei, vec = T.ragged_case()
    b = b.to(DEV)
    eng = m.engine(DEV)
    eng.set_edges(ei, vec)
    g = EqGraph(eng, b, eng.prepare(b))
    ops = EqOps(eng)
    # the hand-off returns the list it was given, CSR pointers included
    assert g.E == 443 and g.N == 23
    assert torch.equal(g.src.cpu().long(), ei[0]) and torch.equal(g.dst.cpu().long(), ei[1])
    assert torch.equal(g.vec.cpu(), vec)
    assert torch.equal(g.eptr.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(ei[1], minlength=23).cumsum(0)]))
    L, M = ops.L, ops.M
    perm = Q.order_major_perm(L, M)
    ctx = dict(L=L, M=M, perm=perm, inv=torch.argsort(perm), src=ei[0], dst=ei[1], Z=b.atomic_numbers.cpu().long(),
               D=T.wigner_rows_to_D(g.wig.cpu(), L, M), rrows=T.radial_rows(L, M), res=int(m.grid_resolution), model=m)
    # the exported Wigner rows are rows of rotations: D D^T = 1 on the kept rows
    D = ctx["D"]
    gram = torch.bmm(D, D.transpose(1, 2))
    assert float((gram - torch.eye(D.shape[1], dtype=D.dtype)).abs().max()) < 1e-5
    _CASES[name] = (ops, g, ctx)
    return _CASES[name]


def compare(label, dev_fn, ref_fn, inputs, seed=0):
    """dev_fn / ref_fn: {name: tensor} -> tensor or tuple of tensors.  Forward and the gradient of every input under a fixed
    random cotangent, device vs float64 reference, with the float32 reference's own distance as calibration."""
    def run(fn, leaves, cot=None):
        out = fn(**leaves)
        out = list(out) if isinstance(out, (tuple, list)) else [out]
        if cot is None:
            gen = torch.Generator().manual_seed(100 + seed)
            cot = [torch.randn(o.shape, generator=gen) for o in out]
        tot = sum((o * c.to(o.device, o.dtype)).sum() for o, c in zip(out, cot))
        grads = torch.autograd.grad(tot, list(leaves.values()), allow_unused=True)
        return [o.detach() for o in out], dict(zip(leaves, grads)), cot

    o64, g64, cot = run(ref_fn, {k: v.detach().double().requires_grad_(True) for k, v in inputs.items()})
    o32, g32, _ = run(ref_fn, {k: v.detach().clone().float().requires_grad_(True) for k, v in inputs.items()}, cot)
    od, gd, _ = run(dev_fn, {k: v.detach().float().to(DEV).requires_grad_(True) for k, v in inputs.items()}, cot)
    od2, gd2, _ = run(dev_fn, {k: v.detach().float().to(DEV).requires_grad_(True) for k, v in inputs.items()}, cot)
    for i, (a, r) in enumerate(zip(od, o64)):
        e = T.frob(a, r)
        print(f"{label}: forward[{i}] {e:.2e}  (float32 oracle {T.frob(o32[i], r):.2e})")
        assert e < 1e-5, (label, "forward", i, e)
        assert torch.equal(a, od2[i]), (label, "forward not reproducible", i)
    for k in inputs:
        if g64[k] is None:
            continue
        assert gd[k] is not None, (label, k)
        d32 = T.frob(g32[k], g64[k])
        bound = max(T.REL_TOL, T.TIGHT_FACTOR * d32)
        e = T.frob(gd[k], g64[k])
        print(f"{label}: d {k:<10s} {e:.2e}  float32 oracle {d32:.2e}  bound {bound:.2e}")
        assert e < bound, (label, k, e, bound)
        assert torch.equal(gd[k], gd2[k]), (label, "gradient not reproducible", k)


def rnd(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_rotate_in(name):
    from adsorbdiff_amd.eqv2_train_step import RotateIn

    ops, g, c = case(name)
    E, C2 = g.E, 2 * ops.C

    def ref(x, radial):
        msg = torch.bmm(c["D"].to(x.dtype), torch.cat([x[c["src"]], x[c["dst"]]], dim=2))[:, c["perm"]]
        return msg * radial.reshape(E, ops.RW, C2)[:, c["rrows"]]          # the oracle's `x0 * radial`, `blk * radial`

    compare(f"rotate_in[{name}]", lambda x, radial: RotateIn.apply(ops, g, x, radial), ref,
            dict(x=rnd(1, g.N, ops.S, ops.C), radial=rnd(2, E, ops.RW * C2)))


@pytest.mark.parametrize("name", ["small", "mfma"])
@pytest.mark.parametrize("which", [1, 2])
def test_so2_convolution(name, which):
    from adsorbdiff_amd.eqv2_train_step import SO2Conv

    ops, g, c = case(name)
    L, M = c["L"], c["M"]
    cin, cout, extra = (2 * ops.C, ops.Hd, ops.NH * ops.A + ops.Hd) if which == 1 else (ops.Hd, ops.NH * ops.V, 0)
    inputs = dict(x=rnd(3, g.E, ops.Sr, cin), W0=rnd(4, (L + 1) * cout + extra, (L + 1) * cin, scale=0.1),
                  b0=rnd(5, (L + 1) * cout + extra, scale=0.1))
    for m_ in range(1, M + 1):
        nm = L - m_ + 1
        inputs[f"W{m_}"] = rnd(5 + m_, 2 * nm * cout, nm * cin, scale=0.1)

    def dev(x, W0, b0, **Wm):
        out, ex = SO2Conv.apply(ops, x, extra, cout, W0, b0, *[Wm[f"W{k}"] for k in range(1, M + 1)])
        return (out, ex) if extra else out

    def ref(x, W0, b0, **Wm):
        sd = {"p.fc_m0.weight": W0, "p.fc_m0.bias": b0}
        sd.update({f"p.so2_m_conv.{k - 1}.fc.weight": Wm[f"W{k}"] for k in range(1, M + 1)})
        r = Q.so2_conv(sd, "p.", x[:, c["inv"]], L, M, cout, None, extra)
        return (r[0][:, c["perm"]], r[1]) if extra else r[:, c["perm"]]

    compare(f"so2_conv_{which}[{name}]", dev, ref, inputs)


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_separable_s2_activation(name):
    from adsorbdiff_amd.eqv2_train_step import S2Act

    ops, g, c = case(name)
    HA = ops.NH * ops.A

    def ref(y, ex):
        grids = Q.Grids(c["L"], c["M"], c["res"], y.dtype)
        y_dm = y[:, c["inv"]]
        gr = torch.einsum("bai,zic->zbac", grids.to_red, y_dm)
        act = torch.einsum("bai,zbac->zic", grids.from_red, F.silu(gr))
        return torch.cat([F.silu(ex[:, HA:])[:, None, :], act[:, 1:]], dim=1)[:, c["perm"]]

    compare(f"s2act[{name}]", lambda y, ex: S2Act.apply(ops, y, ex, HA), ref,
            dict(y=rnd(7, g.E, ops.Sr, ops.Hd), ex=rnd(8, g.E, HA + ops.Hd)))


@pytest.mark.parametrize("name", ["small", "mfma"])
@pytest.mark.parametrize("masked", [False, True])
def test_attention_weights(name, masked):
    from adsorbdiff_amd.eqv2_train_step import AttnWeights

    ops, g, c = case(name)
    H, A = ops.NH, ops.A
    mask = None
    if masked:
        mask = (torch.rand(g.E, H, generator=torch.Generator().manual_seed(9)) >= 0.1).float() / 0.9

    def ref(ex, w, b, adot):
        a = Q.layer_norm(ex[:, :H * A].reshape(-1, H, A), w, b)
        a = torch.einsum("ehk,hk->eh", Q.smooth_leaky_relu(a), adot)
        a = Q.segment_softmax(a, c["dst"], g.N)
        return a if mask is None else a * mask.to(a.dtype)

    md = None if mask is None else mask.to(DEV)
    compare(f"alpha[{name},{'masked' if masked else 'plain'}]", lambda ex, w, b, adot: AttnWeights.apply(ops, g, ex, w, b, adot, md),
            ref, dict(ex=rnd(10, g.E, H * A + ops.Hd), w=1.0 + rnd(11, A, scale=0.1), b=rnd(12, A, scale=0.1),
                      adot=rnd(13, H, A, scale=0.3)))


@pytest.mark.parametrize("name", ["small", "mfma"])
@pytest.mark.parametrize("only_l", [-1, 1])
def test_rotate_out_and_aggregate(name, only_l):
    from adsorbdiff_amd.eqv2_train_step import RotateOut

    ops, g, c = case(name)
    H, V, L, M = ops.NH, ops.V, c["L"], c["M"]

    def ref(z, alpha):
        msg = (z[:, c["inv"]].reshape(g.E, -1, H, V) * alpha[:, None, :, None]).reshape(g.E, -1, H * V)
        back = c["D"].to(z.dtype).transpose(1, 2) * Q.truncation_rescale(L, M, z.dtype)[None, None, :]
        agg = torch.zeros(g.N, ops.S, H * V, dtype=z.dtype).index_add_(0, c["dst"], torch.bmm(back, msg))
        if only_l >= 0:
            keep = torch.zeros(ops.S, dtype=z.dtype)
            keep[only_l * only_l:(only_l + 1) ** 2] = 1.0
            agg = agg * keep[None, :, None]
        return agg

    compare(f"rotate_out[{name},{only_l}]", lambda z, alpha: RotateOut.apply(ops, g, z, alpha, H, V, only_l), ref,
            dict(z=rnd(14, g.E, ops.Sr, H * V), alpha=torch.rand(g.E, H, generator=torch.Generator().manual_seed(15))))


def _radial_inputs(ops, out, seed):
    EC, IN = ops.EC, ops.NB + 2 * ops.EC
    return dict(semb=rnd(seed, ops.NE, EC, scale=0.3), temb=rnd(seed + 1, ops.NE, EC, scale=0.3),
                W0=rnd(seed + 2, EC, IN, scale=IN ** -0.5), b0=rnd(seed + 3, EC, scale=0.1), w1=1.0 + rnd(seed + 4, EC, scale=0.1),
                b1=rnd(seed + 5, EC, scale=0.1), W3=rnd(seed + 6, EC, EC, scale=EC ** -0.5), b3=rnd(seed + 7, EC, scale=0.1),
                w4=1.0 + rnd(seed + 8, EC, scale=0.1), b4=rnd(seed + 9, EC, scale=0.1), W6=rnd(seed + 10, out, EC, scale=EC ** -0.5),
                b6=rnd(seed + 11, out, scale=0.1))


def _radial_ref(c, E, NB, p):
    sd = {"r.net.0.weight": p["W0"], "r.net.0.bias": p["b0"], "r.net.1.weight": p["w1"], "r.net.1.bias": p["b1"],
          "r.net.3.weight": p["W3"], "r.net.3.bias": p["b3"], "r.net.4.weight": p["w4"], "r.net.4.bias": p["b4"],
          "r.net.6.weight": p["W6"], "r.net.6.bias": p["b6"]}
    scal = torch.cat([torch.zeros(E, NB, dtype=p["W0"].dtype), p["semb"][c["Z"][c["src"]]], p["temb"][c["Z"][c["dst"]]]], dim=1)
    return Q.radial_mlp(sd, "r.", scal)


ORDER = ("semb", "temb", "W0", "b0", "w1", "b1", "W3", "b3", "w4", "b4", "W6", "b6")


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_radial_mlp_and_absent_elements(name):
    from adsorbdiff_amd.eqv2_train_step import RadialMLP

    ops, g, c = case(name)
    out = ops.RW * 2 * ops.C
    inputs = _radial_inputs(ops, out, 20)
    compare(f"radial[{name}]", lambda **p: RadialMLP.apply(ops, g, 0, *[p[k] for k in ORDER]),
            lambda **p: _radial_ref(c, g.E, ops.NB, p), inputs)
    # rows of elements that are no edge's source / target: exactly zero
    leaves = {k: v.detach().to(DEV).requires_grad_(True) for k, v in inputs.items()}
    RadialMLP.apply(ops, g, 0, *[leaves[k] for k in ORDER]).square().sum().backward()
    for key, idx in (("semb", c["src"]), ("temb", c["dst"])):
        absent = torch.ones(ops.NE, dtype=torch.bool)
        absent[c["Z"][idx]] = False
        assert int(absent.sum()) > 0
        assert float(leaves[key].grad.cpu()[absent].abs().max()) == 0.0, key
        assert float(leaves[key].grad.cpu()[~absent].abs().min(dim=1).values.max()) > 0.0


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_edge_degree_embedding(name):
    from adsorbdiff_amd.eqv2_train_step import RadialMLP, RotateOut

    ops, g, c = case(name)
    L, M, C_ = c["L"], c["M"], ops.C
    inputs = _radial_inputs(ops, (L + 1) * C_, 40)
    ones = torch.ones(g.E, 1, device=DEV)

    def dev(**p):
        m0 = RadialMLP.apply(ops, g, ops.Sr * C_, *[p[k] for k in ORDER])
        return RotateOut.apply(ops, g, m0.reshape(g.E, ops.Sr, C_), ones, 1, C_, -1) / Q.AVG_DEGREE

    def ref(**p):
        m0 = _radial_ref(c, g.E, ops.NB, p).reshape(-1, L + 1, C_)
        red = Q.lm_list(L, M)
        cols = torch.tensor([red.index((l, 0)) for l in range(L + 1)])
        back = (c["D"].to(m0.dtype).transpose(1, 2) * Q.truncation_rescale(L, M, m0.dtype)[None, None, :])[:, :, cols]
        return torch.zeros(g.N, ops.S, C_, dtype=m0.dtype).index_add_(0, c["dst"], torch.bmm(back, m0)) / Q.AVG_DEGREE

    compare(f"edge_degree[{name}]", dev, ref, inputs)
