"""Every adf_op_* entry of the training step (csrc/train.hip, message_bwd.hip, rbf_wgrad.hip) on its own against float64
torch: the forward is the matching lines of oracle/painn_oracle.py in float64, the backward torch.autograd.grad through those
lines with a random upstream gradient.  The entries are called with raw tensors the way adsorbdiff_amd/train_step.py calls them,
its strided forms included (nrm written into the right half of a [x | nrm] buffer, dnrm read from the right half of dcat).

Bounds.  Products (linear_fwd, linear_bwd): the project's own, 5e-6 / 1e-5 relative.  Fused message kernels and
rbf_wgrad_fused: 2e-5 relative (the bound of the fused-against-plain test).  Everything elementwise or reducing in float32: no
fixed number - the same expression is evaluated with torch in float32 on the CPU, its row-wise error against float64 is e32, and
the kernel's error in the same norm must be at most 4 * e32 (device expf / sqrtf / division are within 1-2 ulp where libm gives
<= 1, and the summation order differs; a wrong index, stride or missing term shows as 1e-2 or more).  Where e32 is exactly 0 the
kernel must be exact.  Every output is surrounded by a sentinel (rows before and after, the columns next to a strided block) that
must stay untouched; it is pre-filled with NaN (a skipped element fails the comparison) or, for accumulating outputs, with random
content.  Each case prints `op shape: e32 error`."""
import ctypes as C
import json
import math

import pytest
import torch

from adsorbdiff_amd import lib as _lib
from adsorbdiff_amd.train_step import _Ops
from oracle import painn_oracle as O
from oracle import train_oracle as TO
from tests import helpers_train as HT
from tests.helpers import rel_err, row_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional
PAD = 3
SENT = -7.25e9

# rows x channels: every N of {1, 3, 63, 64, 65, 257, 4099} and every C of {1, 96, 128, 192, 512} (C = 1 and C = H / 2 are the
# head blocks); single-element rows (C = 1) only where the maximum runs over many rows
GRID = [(1, 128), (3, 96), (63, 1), (64, 192), (65, 512), (257, 96), (257, 1), (4099, 128), (4099, 1), (4099, 192)]

_OPS = None


def ops():
    global _OPS
    if _OPS is None:
        _OPS = _Ops(DEV)
    return _OPS


def gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2**31))


def dev(t, dtype=torch.float32):
    return t.detach().to(DEV, dtype).contiguous()


class Guarded:
    """An output block [rows, cols] inside a sentinel frame: PAD rows before and after, row stride ld >= cols, first
    column col0.  ``init``: the block's content before the call (accumulating outputs); NaN otherwise."""

    def __init__(self, rows, cols, ld=None, col0=0, init=None):
        self.rows, self.cols, self.ld, self.col0 = rows, cols, ld or cols, col0
        assert col0 + cols <= self.ld
        self.buf = torch.full((rows + 2 * PAD, self.ld), SENT, dtype=torch.float32, device=DEV)
        if init is not None:
            self.view.copy_(init.reshape(rows, cols).to(DEV))
        else:
            self.view.fill_(float("nan"))

    @property
    def view(self):
        return self.buf[PAD:PAD + self.rows, self.col0:self.col0 + self.cols]

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * (PAD * self.ld + self.col0)

    def result(self):
        torch.cuda.synchronize()
        out = self.view.clone().cpu()
        frame = self.buf.clone()
        frame[PAD:PAD + self.rows, self.col0:self.col0 + self.cols] = SENT
        assert bool((frame == SENT).all()), "the kernel wrote outside its output block"
        return out


class Strided:
    """An input block [rows, cols] with row stride ld inside a NaN frame (a read outside the block poisons the output)."""

    def __init__(self, t, ld=None, col0=0):
        rows, cols = t.shape[0], t.reshape(t.shape[0], -1).shape[1]
        self.ld = ld or cols
        self.buf = torch.full((rows + 2 * PAD, self.ld), float("nan"), dtype=torch.float32, device=DEV)
        self.buf[PAD:PAD + rows, col0:col0 + cols] = t.reshape(rows, cols).to(DEV)
        self.ptr = self.buf.data_ptr() + 4 * (PAD * self.ld + col0)


def refs(fn, inputs, upstream=None):
    """fn over CPU copies of ``inputs`` in float64 and in float32: [(outputs, gradients of sum(out * upstream))] x 2."""
    res = []
    for dt in (torch.float64, torch.float32):
        xs = [x.detach().cpu().to(dt).requires_grad_(upstream is not None) for x in inputs]
        outs = fn(*xs)
        outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
        grads = None
        if upstream is not None:
            pairs = [(o, u.detach().cpu().to(dt)) for o, u in zip(outs, upstream) if u is not None]
            grads = torch.autograd.grad([o for o, _ in pairs], xs, [u for _, u in pairs], allow_unused=True)
            grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, xs)]
        res.append(([o.detach() for o in outs], grads))
    return res


def check(op, shape, got, ref64, ref32, vector=False, terms=1, floor=1e-7, single=False):
    """The 4 * e32 rule in the row-wise norm (``vector``: a reduced [C] result is one row; ``floor``: rows are measured
    against max(their norm, floor)).

    Rows of ONE element: the maximum over a few stored float32 values is no statistic of the arithmetic - both results may be
    correctly rounded and still differ by any factor - so e32 is then at least what the format gives a float32 reduction of
    ``terms`` terms in an order that is not torch's pairwise one: 2^-24 sqrt(terms) (random-walk model of the rounding
    errors; terms = 1 for an elementwise result: the rounding unit)."""
    got, ref64, ref32 = got.detach().cpu(), ref64.detach().cpu(), ref32.detach().cpu()
    if vector:
        got, ref64, ref32 = got.reshape(1, -1), ref64.reshape(1, -1), ref32.reshape(1, -1)
    else:
        got, ref64, ref32 = (t.reshape(ref64.shape[0], -1) for t in (got, ref64, ref32))
    assert got.shape == ref64.shape, (op, got.shape, ref64.shape)
    e32, err = row_rel_err(ref32, ref64, floor), row_rel_err(got, ref64, floor)
    if (got.shape[1] == 1 or single) and e32 > 0.0:   # (single: one computed element per row next to exact ones)
        e32 = max(e32, 2.0**-24 * math.sqrt(terms))
    print(f"{op} {shape}: e32 {e32:.2e} error {err:.2e}")
    if e32 == 0.0:
        assert torch.equal(got.double(), ref64.double()), (op, shape, "must be exact")
    else:
        assert err <= 4.0 * e32, (op, shape, err, e32)


def s():
    return ops().s()


def ok(status):
    _lib.check(status)


# ------------------------------------------------------------------------------------------------ elementwise operators
@pytest.mark.parametrize("N,Cc", GRID)
def test_ssilu_forward_and_backward(N, Cc):
    g = gen(1, N, Cc)
    h, dy = torch.randn(N, Cc, generator=g) * 3.0, torch.randn(N, Cc, generator=g)
    hd, dyd = dev(h), dev(dy)
    y, dh = Guarded(N, Cc), Guarded(N, Cc)
    ok(ops().lib.adf_op_ssilu_fwd(hd.data_ptr(), y.ptr, N * Cc, s()))
    ok(ops().lib.adf_op_ssilu_bwd(hd.data_ptr(), dyd.data_ptr(), dh.ptr, N * Cc, s()))
    (o64, g64), (o32, g32) = refs(O.ssilu, [h], [dy])
    check("ssilu_fwd", (N, Cc), y.result(), o64[0], o32[0])
    check("ssilu_bwd", (N, Cc), dh.result(), g64[0], g32[0])


def test_ssilu_stays_finite_up_to_100():
    h = torch.cat([torch.linspace(-100.0, 100.0, 4001), torch.tensor([-100.0, -88.8, -87.3, 87.3, 88.8, 100.0, 0.0, -0.0]),
                   torch.zeros(23)]).sort().values.reshape(-1, 64)          # rows of 64 neighbouring arguments
    n = h.numel()
    dy = torch.randn(h.shape, generator=gen(2))
    hd, dyd = dev(h), dev(dy)
    y, dh = Guarded(h.shape[0], 64), Guarded(h.shape[0], 64)
    ok(ops().lib.adf_op_ssilu_fwd(hd.data_ptr(), y.ptr, n, s()))
    ok(ops().lib.adf_op_ssilu_bwd(hd.data_ptr(), dyd.data_ptr(), dh.ptr, n, s()))
    (o64, g64), (o32, g32) = refs(O.ssilu, [h], [dy])
    yr, dhr = y.result(), dh.result()
    assert bool(torch.isfinite(yr).all()) and bool(torch.isfinite(dhr).all())
    check("ssilu_fwd |x| <= 100", h.shape, yr, o64[0], o32[0])
    check("ssilu_bwd |x| <= 100", h.shape, dhr, g64[0], g32[0])


def _layernorm_inputs(N, H, g):
    x = torch.randn(N, H, generator=g) * (0.5 + torch.rand(N, 1, generator=g) * 3.0) + torch.randn(N, 1, generator=g)
    if N >= 3:
        x[N - 1] = 0.75                                      # a constant row (its sums are exact in binary)
        x[N // 2] = 1.0e4 + torch.randn(H, generator=g)      # mean 1e4, unit spread
    w, b = 1.0 + 0.3 * torch.randn(H, generator=g), 0.2 * torch.randn(H, generator=g)
    return x, w, b


@pytest.mark.parametrize("N,H", [(n, c) for n, c in GRID if c > 1])
def test_layernorm_forward_and_backward(N, H):
    g = gen(3, N, H)
    x, w, b = _layernorm_inputs(N, H, g)
    dy, dx0 = torch.randn(N, H, generator=g), torch.randn(N, H, generator=g)
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    y, stats = Guarded(N, H), Guarded(N, 2)
    ok(ops().lib.adf_op_layernorm_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr, stats.ptr, N, H, s()))

    def fwd(x_, w_, b_):
        return F.layer_norm(x_, (H,), w_, b_)

    def st(x_):
        return torch.stack([x_.mean(1), 1.0 / torch.sqrt(x_.var(1, unbiased=False) + 1e-5)], dim=1)

    (o64, g64), (o32, g32) = refs(fwd, [x, w, b], [dy])
    (s64, _), (s32, _) = refs(st, [x])
    check("layernorm_fwd", (N, H), y.result(), o64[0], o32[0])
    stats_got = stats.result()
    # the mean against the row's own scale (its rms, the same exact column in all three): relative to a mean that cancels to
    # 1e-3 of the spread a float32 sum of H terms is noise
    rms = x.double().pow(2).mean(1, keepdim=True).sqrt()
    check("layernorm_stats_mean", (N, H), torch.cat([stats_got[:, :1].double(), rms], 1), torch.cat([s64[0][:, :1], rms], 1),
          torch.cat([s32[0][:, :1].double(), rms], 1), terms=H, single=True)
    check("layernorm_stats_rstd", (N, H), stats_got[:, 1:], s64[0][:, 1:], s32[0][:, 1:], terms=H)
    # backward from the kernel's own statistics, as in the step; dx ADDS to random content
    stats_d = dev(stats_got)
    dx, dw, db = Guarded(N, H, init=dx0), Guarded(1, H), Guarded(1, H)
    sc = ops().scratch(512 * 2 * H + 16)
    ok(ops().lib.adf_op_layernorm_bwd(xd.data_ptr(), wd.data_ptr(), stats_d.data_ptr(), dyd.data_ptr(), dx.ptr, dw.ptr, db.ptr,
                                      N, H, sc.data_ptr(), s()))
    check("layernorm_bwd_dx", (N, H), dx.result(), dx0.double() + g64[0], dx0 + g32[0])
    check("layernorm_bwd_dw", (N, H), dw.result(), g64[1], g32[1], vector=True)
    check("layernorm_bwd_db", (N, H), db.result(), g64[2], g32[2], vector=True)


def _vdot_ref(Cc, eps=1e-8):
    def fn(vv):   # update_layer: v1, v2 = split(vec_proj(vec)); dot; vn
        v1, v2 = vv[..., :Cc], vv[..., Cc:]
        return (v1 * v2).sum(dim=1) * (1 / math.sqrt(Cc)), torch.sqrt(torch.sum(v2**2, dim=-2) + eps), v1
    return fn


@pytest.mark.parametrize("with_ddot,with_dv1", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("N,Cc", GRID)
def test_vdot_forward_and_backward(N, Cc, with_ddot, with_dv1):
    g = gen(4, N, Cc)
    vv = torch.randn(N, 3, 2 * Cc, generator=g)
    vv[0, :, Cc:] = 0.0                          # v2 = 0: the eps path, nrm = 1e-4
    xleft = torch.randn(N, Cc, generator=g)
    ddot, dnrm, dv1 = (torch.randn(N, Cc, generator=g), torch.randn(N, Cc, generator=g), torch.randn(N, 3, Cc, generator=g))
    vvd = dev(vv)
    dot = Guarded(N, Cc)
    cat = Guarded(N, 2 * Cc, init=torch.cat([xleft, torch.full((N, Cc), float("nan"))], 1))   # [x | nrm], ldn = 2C
    ok(ops().lib.adf_op_vdot_fwd(vvd.data_ptr(), dot.ptr, cat.ptr + 4 * Cc, 2 * Cc, N, Cc, C.c_float(1e-8), s()))
    up = [ddot if with_ddot else None, dnrm, dv1 if with_dv1 else None]
    (o64, g64), (o32, g32) = refs(_vdot_ref(Cc), [vv], up)
    if with_ddot and with_dv1:
        check("vdot_fwd_dot", (N, Cc), dot.result(), o64[0], o32[0])
        catr = cat.result()
        assert torch.equal(catr[:, :Cc], xleft), "vdot_fwd touched the left half of [x | nrm]"
        check("vdot_fwd_nrm", (N, Cc), catr[:, Cc:], o64[1], o32[1])
    # backward: nrm from its strided place (float32 torch values), dnrm from the right half of dcat with ANOTHER stride
    nrm_in = Strided(o32[1], ld=2 * Cc, col0=Cc)
    dcat = Strided(dnrm, ld=2 * Cc + 8, col0=Cc)
    ddotd, dv1d = dev(ddot), dev(dv1)
    dvv = Guarded(3 * N, 2 * Cc)
    ok(ops().lib.adf_op_vdot_bwd(vvd.data_ptr(), nrm_in.ptr, 2 * Cc, ddotd.data_ptr() if with_ddot else None, dcat.ptr,
                                 2 * Cc + 8, dv1d.data_ptr() if with_dv1 else None, dvv.ptr, N, Cc, s()))
    check(f"vdot_bwd ddot={int(with_ddot)} dv1={int(with_dv1)}", (N, Cc), dvv.result().reshape(N, -1), g64[0].reshape(N, -1),
          g32[0].reshape(N, -1))


@pytest.mark.parametrize("N,H", GRID)
def test_update_out_forward_and_backward(N, H):
    g = gen(5, N, H)
    x1, vec1, a = torch.randn(N, H, generator=g), torch.randn(N, 3, H, generator=g), torch.randn(N, 3 * H, generator=g)
    dot, vv = torch.randn(N, H, generator=g), torch.randn(N, 3, 2 * H, generator=g)
    dx2, dvec2 = torch.randn(N, H, generator=g), torch.randn(N, 3, H, generator=g)
    scale = 0.9

    def fn(x1_, vec1_, a_, dot_, vv_):   # update_layer's tail + the residuals and the scale factor of painn_forward
        h1, h2, h3 = a_[:, :H], a_[:, H:2 * H], a_[:, 2 * H:]
        dx = (h1 + h2 * dot_) * (1 / math.sqrt(2.0))
        dvec = h3[:, None, :] * vv_[..., :H]
        return (x1_ + dx) * scale, vec1_ + dvec

    dv = [dev(t) for t in (x1, vec1, a, dot, vv, dx2, dvec2)]
    x2, vec2 = Guarded(N, H), Guarded(3 * N, H)
    ok(ops().lib.adf_op_update_out_fwd(dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(),
                                       C.c_float(scale), x2.ptr, vec2.ptr, N, H, s()))
    da, ddot, dv1, dx1, dvec1 = Guarded(N, 3 * H), Guarded(N, H), Guarded(3 * N, H), Guarded(N, H), Guarded(3 * N, H)
    ok(ops().lib.adf_op_update_out_bwd(dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), C.c_float(scale), dv[5].data_ptr(),
                                       dv[6].data_ptr(), da.ptr, ddot.ptr, dv1.ptr, dx1.ptr, dvec1.ptr, N, H, s()))
    (o64, g64), (o32, g32) = refs(fn, [x1, vec1, a, dot, vv], [dx2, dvec2])
    check("update_out_fwd_x2", (N, H), x2.result(), o64[0], o32[0])
    check("update_out_fwd_vec2", (N, H), vec2.result().reshape(N, -1), o64[1].reshape(N, -1), o32[1].reshape(N, -1))
    check("update_out_bwd_dx1", (N, H), dx1.result(), g64[0], g32[0])
    check("update_out_bwd_dvec1", (N, H), dvec1.result().reshape(N, -1), g64[1].reshape(N, -1), g32[1].reshape(N, -1))
    check("update_out_bwd_da", (N, H), da.result(), g64[2], g32[2])
    check("update_out_bwd_ddot", (N, H), ddot.result(), g64[3], g32[3])
    # the direct gradient of v1 (the left half of d vv); nothing reaches v2 here
    assert float(g64[4][..., H:].abs().max()) == 0.0
    check("update_out_bwd_dv1", (N, H), dv1.result().reshape(N, -1), g64[4][..., :H].reshape(N, -1),
          g32[4][..., :H].reshape(N, -1))


@pytest.mark.parametrize("N,Cc", GRID)
def test_vnorm_forward_and_backward(N, Cc):
    g = gen(6, N, Cc)
    t1 = torch.randn(N, 3, Cc, generator=g)
    t1[N - 1, :, 0] = 0.0                        # an exactly zero vector: torch's subgradient is 0
    xleft, dnrm = torch.randn(N, Cc, generator=g), torch.randn(N, Cc, generator=g)
    t1d = dev(t1)
    cat = Guarded(N, 2 * Cc, init=torch.cat([xleft, torch.full((N, Cc), float("nan"))], 1))
    ok(ops().lib.adf_op_vnorm_fwd(t1d.data_ptr(), cat.ptr + 4 * Cc, 2 * Cc, N, Cc, s()))

    def fn(t):   # gated_block: torch.norm(vec1_proj(v), dim=-2)
        return torch.norm(t, dim=-2)

    (o64, g64), (o32, g32) = refs(fn, [t1], [dnrm])
    catr = cat.result()
    assert torch.equal(catr[:, :Cc], xleft), "vnorm_fwd touched the left half of [x | nrm]"
    check("vnorm_fwd", (N, Cc), catr[:, Cc:], o64[0], o32[0])
    assert float(catr[N - 1, Cc]) == 0.0
    nrm_in = Strided(o32[0], ld=2 * Cc, col0=Cc)          # ldn = 2C ...
    dcat = Strided(dnrm, ld=2 * Cc + 8, col0=Cc)          # ... and lddn different from it
    dt1 = Guarded(3 * N, Cc)
    ok(ops().lib.adf_op_vnorm_bwd(t1d.data_ptr(), nrm_in.ptr, 2 * Cc, dcat.ptr, 2 * Cc + 8, dt1.ptr, N, Cc, s()))
    got = dt1.result().reshape(N, 3, Cc)
    assert float(got[N - 1, :, 0].abs().max()) == 0.0 and float(g64[0][N - 1, :, 0].abs().max()) == 0.0
    check("vnorm_bwd", (N, Cc), got.reshape(N, -1), g64[0].reshape(N, -1), g32[0].reshape(N, -1))


@pytest.mark.parametrize("with_xs", [True, False])
@pytest.mark.parametrize("N,Cc", GRID)
def test_gate_forward_and_backward(N, Cc, with_xs):
    g = gen(7, N, Cc)
    o, t2 = torch.randn(N, 2 * Cc, generator=g) * 2.0, torch.randn(N, 3, Cc, generator=g)
    dxs, dvout = torch.randn(N, Cc, generator=g), torch.randn(N, 3, Cc, generator=g)

    def fn(o_, t2_):   # gated_block: ssilu(xo), gate * vec2
        return O.ssilu(o_[:, :Cc]), o_[:, Cc:][:, None, :] * t2_

    od, t2d, dvd = dev(o), dev(t2), dev(dvout)
    xs, vout = Guarded(N, Cc, ld=Cc + 5, col0=2), Guarded(3 * N, Cc)
    ok(ops().lib.adf_op_gate_fwd(od.data_ptr(), t2d.data_ptr(), xs.ptr if with_xs else None, Cc + 5, vout.ptr, N, Cc, s()))
    (o64, g64), (o32, g32) = refs(fn, [o, t2], [dxs if with_xs else None, dvout])
    if with_xs:
        check("gate_fwd_xs", (N, Cc), xs.result(), o64[0], o32[0])
    check("gate_fwd_vout", (N, Cc), vout.result().reshape(N, -1), o64[1].reshape(N, -1), o32[1].reshape(N, -1))
    dxs_in = Strided(dxs, ld=Cc + 3, col0=1)
    d_o, dt2 = Guarded(N, 2 * Cc), Guarded(3 * N, Cc)
    ok(ops().lib.adf_op_gate_bwd(od.data_ptr(), t2d.data_ptr(), dxs_in.ptr if with_xs else None, Cc + 3, dvd.data_ptr(), d_o.ptr,
                                 dt2.ptr, N, Cc, s()))
    got = d_o.result()
    if with_xs:
        check("gate_bwd_do_x", (N, Cc), got[:, :Cc], g64[0][:, :Cc], g32[0][:, :Cc])
    else:
        assert float(got[:, :Cc].abs().max()) == 0.0
    check(f"gate_bwd_do_gate xs={int(with_xs)}", (N, Cc), got[:, Cc:], g64[0][:, Cc:], g32[0][:, Cc:])
    check(f"gate_bwd_dt2 xs={int(with_xs)}", (N, Cc), dt2.result().reshape(N, -1), g64[1].reshape(N, -1), g32[1].reshape(N, -1))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("N,Cc", GRID)
def test_copy_rows(N, Cc, accumulate):
    g = gen(8, N, Cc)
    src, dst0 = torch.randn(N, Cc, generator=g), torch.randn(N, Cc, generator=g)
    sin = Strided(src, ld=2 * Cc + 1, col0=1)
    dst = Guarded(N, Cc, ld=Cc + 7, col0=3, init=dst0 if accumulate else None)
    ok(ops().lib.adf_op_copy_rows(sin.ptr, 2 * Cc + 1, dst.ptr, Cc + 7, N, Cc, accumulate, s()))
    if accumulate:
        check("copy_rows accumulate", (N, Cc), dst.result(), dst0.double() + src.double(), dst0 + src)
    else:
        check("copy_rows", (N, Cc), dst.result(), src.double(), src)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2047, 2049, 4099 * 128, 3 * 512 * 512 + 5])
def test_sqnorm_accumulate(n):
    gsrc = torch.randn(n, generator=gen(9, n)) * 1e-3
    gsrc[0], gsrc[-1] = 0.4, -0.3          # a dropped first or last element is a quarter of the sum
    gd = dev(gsrc)
    out = Guarded(1, 1, init=torch.tensor([[0.37]]))   # ADDS to what is there
    ok(ops().lib.adf_op_sqnorm_accumulate(gd.data_ptr(), n, out.ptr, s()))
    check("sqnorm_accumulate", (n,), out.result(), 0.37 + (gsrc.double() ** 2).sum().reshape(1, 1),
          (torch.tensor(0.37) + (gsrc**2).sum()).reshape(1, 1), terms=n)


# ------------------------------------------------------------------------------------------------ embedding
def _small_model(H=128, R=128):
    return HT.make_config_model(dict(HT.CONFIGS["ragged"], H=H, R=R)).to(DEV)


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 257, 4099])
def test_embed_forward_and_backward(N):
    H = 128
    m = _small_model()
    eng = m.engine(DEV)
    g = gen(10, N)
    present = torch.tensor([1, 6, 8, 29, 78, 83])                 # many atoms per element; every other element is absent
    Z = present[torch.randint(0, len(present), (N,), generator=g)]
    Zd = dev(Z, torch.int32)
    x = Guarded(N, H)
    ok(ops().lib.adf_op_embed_fwd(eng.handle, Zd.data_ptr(), N, x.ptr, s()))
    table = m.atom_emb.embeddings.weight.detach().cpu()
    check("embed_fwd", (N, H), x.result(), table[Z - 1].double(), table[Z - 1])
    dx, demb0 = torch.randn(N, H, generator=g), torch.randn(table.shape[0], H, generator=g)
    dxd = dev(dx)
    demb = Guarded(table.shape[0], H, init=demb0)
    ok(ops().lib.adf_op_embed_bwd(dxd.data_ptr(), Zd.data_ptr(), demb.ptr, N, H, s()))
    got = demb.result()
    r64 = demb0.double().index_add(0, Z - 1, dx.double())
    r32 = demb0.clone().index_add(0, Z - 1, dx)
    absent = torch.ones(table.shape[0], dtype=torch.bool)
    absent[Z - 1] = False
    assert int(absent.sum()) >= table.shape[0] - len(present)
    assert torch.equal(got[absent], demb0[absent]), "embed_bwd touched the row of an element that does not occur"
    check("embed_bwd", (N, H), got[~absent], r64[~absent], r32[~absent])


# ------------------------------------------------------------------------------------------------ loss
class _FixedNorm:
    def __init__(self, norm):
        self.norm = norm

    def score_norm(self, eps):
        return self.norm


@pytest.mark.parametrize("B,ads", [(1, (1,)), (1, (70,)), (5, (1, 4, 70, 4, 1)), (70, (4, 1, 70, 4, 1, 4, 4))])
def test_score_loss(B, ads):
    g = gen(11, B, len(ads))
    tags, batch = [], []
    for b in range(B):
        n_ads = ads[b % len(ads)]
        n_slab = int(torch.randint(3, 90, (1,), generator=g))
        t = torch.cat([torch.randint(0, 2, (n_slab,), generator=g), torch.full((n_ads,), 2)])
        t = t[torch.randperm(t.numel(), generator=g)]            # adsorbate atoms interleaved with the slab's
        tags.append(t)
        batch.append(torch.full((t.numel(),), b))
    tags, batch = torch.cat(tags).long(), torch.cat(batch).long()
    N = tags.numel()
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.bincount(batch, minlength=B), 0).to(torch.int32)
    f1, f2 = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    tg = HT.make_targets(B, seed=12)
    rot_norm = 0.5 + torch.rand(B, 1, generator=g) * 3.0
    names = ("tr_sigma", "rot_sigma", "tr_score", "rot_score")
    f1d, f2d, tagd, offd, nd = dev(f1), dev(f2), dev(tags, torch.int32), dev(off, torch.int32), dev(rot_norm)
    td = [dev(tg[k]) for k in names]
    loss, df1, df2 = Guarded(1, 3), Guarded(N, 3), Guarded(N, 3)
    ok(ops().lib.adf_op_score_loss(f1d.data_ptr(), f2d.data_ptr(), tagd.data_ptr(), offd.data_ptr(), td[0].data_ptr(),
                                   td[1].data_ptr(), td[2].data_ptr(), td[3].data_ptr(), nd.data_ptr(), loss.ptr, df1.ptr,
                                   df2.ptr, B, ops().scratch(2 * B + 16).data_ptr(), s()))
    out = []
    for dt in (torch.float64, torch.float32):
        a1, a2 = f1.to(dt).requires_grad_(True), f2.to(dt).requires_grad_(True)
        l, terms = TO.score_matching_loss(a1, a2, tags, batch, {k: tg[k].to(dt) for k in names}, _FixedNorm(rot_norm.to(dt)))
        g1, g2 = torch.autograd.grad(l, [a1, a2])
        out.append((torch.stack([l.detach(), terms[0].detach(), terms[1].detach()]).reshape(3, 1), g1, g2))
    shape = (B, N, max(ads))
    check("score_loss", shape, loss.result().reshape(3, 1), out[0][0], out[1][0], terms=3 * B + max(ads))
    got1, got2 = df1.result(), df2.result()
    assert float(got1[tags != 2].abs().max()) == 0.0 and float(got2[tags != 2].abs().max()) == 0.0
    check("score_loss_df1", shape, got1, out[0][1], out[1][1])
    check("score_loss_df2", shape, got2, out[0][2], out[1][2])


# ------------------------------------------------------------------------------------------------ products
LINEAR_NK = [(128, 128), (384, 128), (576, 192), (96, 96), (2, 64), (1, 64), (192, 64)]
LINEAR_BWD_M = [1, 31, 33, 1023, 1025, 8197, 9217, 66563]


@pytest.mark.parametrize("N,K", LINEAR_NK + [(384, 32), (64, 256)])
def test_linear_forward(N, K):
    """y = A W^T + b through the f16x3 split at the step's shapes: 5e-6 relative (test_linear_f16x3_activation_range), every
    row against its own norm, with and without bias, contiguous and with lda / ldc larger than the width."""
    for M in (1, 3, 63, 64, 65, 257, 4099):
        for strided in (False, True):
            g = gen(13, M, N, K, strided)
            A = torch.randn(M, K, generator=g) * (10.0 ** torch.randint(-3, 3, (M, 1), generator=g).float())
            W, b = torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
            lda, ldc = (K + 4, N + 4) if strided else (K, N)
            Ain = Strided(A, ld=lda)
            Wd, bd = dev(W), dev(b)
            out = Guarded(M, N, ld=ldc)
            use_bias = not strided
            ok(ops().lib.adf_op_linear_fwd(Ain.ptr, lda, Wd.data_ptr(), bd.data_ptr() if use_bias else None, out.ptr, ldc, M, N,
                                           K, s()))
            ref = A.double() @ W.double().T + (b.double() if use_bias else 0.0)
            got = out.result()
            # every row against its own scale |a_m| max_n |w_n| (the normwise measure of a dot product: a row of one or two
            # outputs may cancel to nothing), and for a full-width output also against its own norm as in the existing test
            scale = A.double().norm(dim=1) * W.double().norm(dim=1).max() + (b.double().abs().max() if use_bias else 0.0)
            err = rel_err(got, ref)
            berr = float(((got.double() - ref).norm(dim=1) / math.sqrt(N) / scale).max())
            rerr = row_rel_err(got, ref) if N >= 32 else 0.0
            print(f"linear_fwd {(M, N, K)} strided={int(strided)}: error {err:.2e} row-wise {rerr:.2e} normwise {berr:.2e}")
            assert err < 5e-6 and rerr < 5e-6 and berr < 5e-6, (M, N, K, strided, err, rerr, berr)


def linear_bwd_sweep(m_list=LINEAR_BWD_M, nk_list=LINEAR_NK):
    """adf_op_linear_bwd against float64 products: [(label, worst relative error)] over the variants
    plain (contiguous, dA written, dW and db accumulated onto random content), strided (lda / ldc / ldda larger than the
    width, dA accumulated), odd (row strides of A and dA off the 16-byte grid: the generic weight-gradient kernel and the add
    pass; the products themselves take dC with a stride that is a multiple of 4 only), db_only (column sums without
    a weight gradient) and dA_only (A = None)."""
    o = ops()
    res = []
    for M in m_list:
        for (N, K) in nk_list:
            g = gen(14, M, N, K)
            A = torch.randn(M, K, generator=g, dtype=torch.float32).to(DEV)
            W = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
            dC = torch.randn(M, N, generator=g).to(DEV)
            dW0, db0, dA0 = (torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(M, K, generator=g))
            rW, rb, rA = dC.double().t() @ A.double(), dC.double().sum(0), dC.double() @ W.double()
            Wd = W.contiguous()
            for variant in ("plain", "strided", "odd", "db_only", "dA_only"):
                lda, ldc, ldda = {"strided": (K + 4, N + 4, K + 8), "odd": (K + 1, N + 4, K + 5)}.get(variant, (K, N, K))
                Ain, dCin = Strided(A, ld=lda), Strided(dC, ld=ldc)
                acc = variant in ("strided", "odd")
                want_dA = variant != "db_only"
                want_dW = variant in ("plain", "strided", "odd")
                want_db = variant != "dA_only"
                dA = Guarded(M, K, ld=ldda, init=dA0 if acc else None)
                dW, db = Guarded(N, K, init=dW0), Guarded(1, N, init=db0)
                sc = o.scratch(int(o.lib.adf_op_linear_bwd_scratch(M, N, K)))
                ok(o.lib.adf_op_linear_bwd(Ain.ptr if variant != "dA_only" else None, lda, Wd.data_ptr(), dCin.ptr, ldc,
                                           dA.ptr if want_dA else None, ldda, 1 if acc else 0, dW.ptr if want_dW else None,
                                           db.ptr if want_db else None, 1, M, N, K, sc.data_ptr(), o.s()))
                worst = 0.0
                if want_dA:
                    worst = max(worst, rel_err(dA.result(), (dA0.double() if acc else 0.0) + rA.cpu()))
                else:
                    dA.view.fill_(SENT)
                    dA.result()
                if want_dW:
                    worst = max(worst, rel_err(dW.result(), dW0.double() + rW.cpu()))
                else:
                    assert torch.equal(dW.result(), dW0)
                if want_db:
                    # against max(|db|, |dC|_F): a column sum of M terms may cancel (N = 1: one scalar), its natural size
                    # is the column's norm
                    ref_b = db0.double() + rb.cpu()
                    e_b = float((db.result().reshape(-1).double() - ref_b).norm() / max(float(ref_b.norm()), float(dC.norm())))
                    worst = max(worst, e_b)
                else:
                    assert torch.equal(db.result().reshape(-1), db0)
                res.append((f"linear_bwd M={M} N={N} K={K} {variant}", worst))
    return res


def test_linear_backward_shapes_splits_and_strides():
    """M from one split over the `&~7` rounding and empty trailing splits to the cap at 64; (N, K) over the bf16 kernel, the
    generic kernel with partial tiles and the N <= 4 data-gradient kernel.  1e-5 relative
    (test_linear_backward_weight_gradient_kernels_vs_torch)."""
    res = linear_bwd_sweep()
    for label, e in res:
        print(f"{label}: error {e:.2e}")
    bad = [(label, e) for label, e in res if not e < 1e-5]
    assert not bad, bad


_LINEAR_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
from tests.test_gpu_train_ops import linear_bwd_sweep
print("RES " + json.dumps(linear_bwd_sweep()), flush=True)
"""


@pytest.mark.parametrize("env", [{"ADF_TRAIN_GEMM": "f32"}, {"ADF_WGRAD": "f32"}])
def test_linear_backward_shapes_with_the_exact_f32_kernels(env):
    """The same shape list in a child process under ADF_TRAIN_GEMM=f32 (exact-f32 data-gradient products) and under
    ADF_WGRAD=f32 (tr_wgrad128_kernel); both are read once per process."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parent.parent)
    e = dict(os.environ)
    e.pop("ADF_TRAIN_GEMM", None)
    e.pop("ADF_WGRAD", None)
    e.update(env)
    res = subprocess.run([sys.executable, "-c", _LINEAR_CHILD.format(root=root)], env=e, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.split("RES ")[-1])
    assert len(out) == len(LINEAR_BWD_M) * len(LINEAR_NK) * 5
    worst = max(out, key=lambda t: t[1])
    print(f"{env}: worst {worst[1]:.2e} ({worst[0]})")
    bad = [(label, err) for label, err in out if not err < 1e-5]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ message operators
_MESSAGE_CASES = {}


def _message_case(graph, H, R):
    """Model, engine with the configuration's graph, and that graph as exported (rows in the device's CSR order)."""
    key = (graph, H, R)
    if key not in _MESSAGE_CASES:
        cfg = dict(HT.CONFIGS[graph], H=H, R=R, L=2)
        m = HT.make_config_model(cfg).to(DEV)
        b = HT.make_config_batch(cfg)
        eng = m.engine(DEV)
        E = eng.build_graph(b.clone().to(DEV))
        ei, _, dist, unit = HT.graph_from_export(eng)
        assert ei.shape[1] == E
        indeg = torch.bincount(ei[1], minlength=b.pos.shape[0])
        if graph == "ragged":
            assert int((ei[0] == ei[1]).sum()) > 0
        if graph == "isolated":
            assert int(indeg.min()) == 0
        if graph == "hub":
            assert int(indeg.max()) > 256
        _MESSAGE_CASES.clear()   # one engine at a time
        _MESSAGE_CASES[key] = (m, eng, b, ei, dist, unit)
    m, eng, b, ei, dist, unit = _MESSAGE_CASES[key]
    eng.build_graph(b.clone().to(DEV))
    return m, eng, b, ei, dist, unit


def _message_ref(ei, unit, H, first):
    src, dst = ei

    def fn(xh, vec, x, rbfh):   # message_layer from `g = xh[src] * rbfh` on, then painn_forward's residuals
        g = xh[src] * rbfh
        m_x, g2, g3 = g[:, :H], g[:, H:2 * H], g[:, 2 * H:]
        g2 = g2 * (1 / math.sqrt(3.0))
        u = unit.to(xh.dtype)
        vsrc = torch.zeros_like(vec)[src] if first else vec[src]
        m_v = (vsrc * g2[:, None, :] + g3[:, None, :] * u[:, :, None]) * (1 / math.sqrt(H))
        dx = torch.zeros_like(x).index_add_(0, dst, m_x)
        dvec = torch.zeros_like(vec).index_add_(0, dst, m_v)
        return (x + dx) * (1 / math.sqrt(2.0)), (dvec if first else vec + dvec)
    return fn


MESSAGE_GRID = [("ragged", 128, 128), ("ragged", 192, 96), ("ragged", 512, 32), ("isolated", 128, 32), ("isolated", 192, 128),
                ("hub", 128, 128), ("isolated", 512, 96)]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("graph,H,R", MESSAGE_GRID)
def test_message_operators(graph, H, R, first):
    """adf_op_rbf, edge_owner, message_fwd / message_bwd (plain: 4 * e32), message_fwd_fused / message_bwd_fused in both
    forms and rbf_image + rbf_wgrad_fused (2e-5) on one graph, first (vec_is_zero) or later layer."""
    m, eng, b, ei, dist, unit = _message_case(graph, H, R)
    h, lib, o = eng.handle, ops().lib, ops()
    layer = 0 if first else 1
    N, E = b.pos.shape[0], ei.shape[1]
    shape = (graph, H, R, "first" if first else "later")
    # the radial basis, row by row: pins the order of the exported edge list
    rbf = Guarded(E, R)
    ok(lib.adf_op_rbf(h, rbf.ptr, s()))
    rbf_got = rbf.result()
    # (rows against max(their norm, 1): a row is of order one until the envelope 1 - 21 x^5 + 35 x^6 - 15 x^7 takes it to
    # zero at the cutoff, and that polynomial cancels terms of order 35 - an absolute float32 error of order 35 * 2^-24 in
    # every element whatever its size, in torch as in the kernel; relative to a row of 1e-6 that is noise)
    check("rbf", shape, rbf_got, O.radial_basis(dist.double(), float(m.cutoff), R), O.radial_basis(dist, float(m.cutoff), R),
          floor=1.0)
    owner = torch.full((E + 2 * PAD,), -77, dtype=torch.int32, device=DEV)
    ok(lib.adf_op_edge_owner(h, owner.data_ptr() + 4 * PAD, E, s()))
    torch.cuda.synchronize()
    assert torch.equal(owner[PAD:PAD + E].cpu().long(), ei[1]) and bool((owner[:PAD] == -77).all()) and \
        bool((owner[PAD + E:] == -77).all())

    g = gen(15, H, R, first, len(graph))
    P = {k: v.detach().cpu() for k, v in m.named_parameters()}
    W, bias = P[f"message_layers.{layer}.rbf_proj.weight"], P[f"message_layers.{layer}.rbf_proj.bias"]
    xh, vec, x = torch.randn(N, 3 * H, generator=g), torch.randn(N, 3, H, generator=g), torch.randn(N, H, generator=g)
    gx1, gv1 = torch.randn(N, H, generator=g), torch.randn(N, 3, H, generator=g)
    # rbfh from the device's own basis rows, rounded once from float64: a function of the distance only, as the plain
    # backward assumes (an edge and its reverse hold the same row)
    rbfh = (rbf_got.double() @ W.double().T + bias.double()).float()
    fn = _message_ref(ei, unit, H, first)
    (o64, g64), (o32, g32) = refs(fn, [xh, vec, x, rbfh], [gx1, gv1])
    d = {k: dev(v) for k, v in dict(xh=xh, vec=vec, x=x, rbfh=rbfh, gx1=gx1, gv1=gv1, rbf=rbf_got).items()}
    vptr = None if first else d["vec"].data_ptr()

    # ---- plain kernels
    x1, vec1 = Guarded(N, H), Guarded(3 * N, H)
    ok(lib.adf_op_message_fwd(h, d["xh"].data_ptr(), vptr, d["rbfh"].data_ptr(), d["x"].data_ptr(), x1.ptr, vec1.ptr,
                              1 if first else 0, s()))
    check("message_fwd_x1", shape, x1.result(), o64[0], o32[0])
    check("message_fwd_vec1", shape, vec1.result().reshape(N, -1), o64[1].reshape(N, -1), o32[1].reshape(N, -1))
    dxh, drbfh, dvec, dx = Guarded(N, 3 * H), Guarded(E, 3 * H), Guarded(3 * N, H), Guarded(N, H)
    ok(lib.adf_op_message_bwd(h, d["xh"].data_ptr(), vptr, d["rbfh"].data_ptr(), d["gx1"].data_ptr(), d["gv1"].data_ptr(),
                              dxh.ptr, drbfh.ptr, None if first else dvec.ptr, dx.ptr, 1 if first else 0, s()))
    check("message_bwd_dxh", shape, dxh.result(), g64[0], g32[0])
    check("message_bwd_dx", shape, dx.result(), g64[2], g32[2])
    if not first:
        check("message_bwd_dvec", shape, dvec.result().reshape(N, -1), g64[1].reshape(N, -1), g32[1].reshape(N, -1))
    # d(rbfh) is written at the row of the REVERSE edge: only its contractions with functions of the distance are defined
    rb64 = rbf_got.double()
    dr = drbfh.result().double()
    check("message_bwd_drbfh^T rbf", shape, dr.T @ rb64, g64[3].T @ rb64, g32[3].double().T @ rb64)
    check("message_bwd_drbfh colsum", shape, dr.sum(0), g64[3].sum(0), g32[3].double().sum(0), vector=True)

    # ---- fused kernels: rbfh regenerated from the layer's weights; reference through rbf_proj in float64
    def fn_w(xh_, vec_, x_, W_, b_):
        return fn(xh_, vec_, x_, F.linear(O.radial_basis(dist.to(xh_.dtype), float(m.cutoff), R), W_, b_))

    (f64, gw64), _ = refs(fn_w, [xh, vec, x, W, bias], [gx1, gv1])
    assert bool(lib.adf_op_message_bwd_fused_supported(h))
    x1, vec1 = Guarded(N, H), Guarded(3 * N, H)
    ok(lib.adf_op_message_fwd_fused(h, layer, d["xh"].data_ptr(), vptr, d["x"].data_ptr(), x1.ptr, vec1.ptr, 1 if first else 0,
                                    s()))
    figs = {"fwd_fused_x1": rel_err(x1.result(), f64[0]), "fwd_fused_vec1": rel_err(vec1.result().reshape(N, 3, H), f64[1])}
    # (a) d(rbfh) stored in the kernel's column order, permuted back through message_bwd_perm
    perm = (C.c_int32 * (3 * H))()
    ok(lib.adf_op_message_bwd_perm(h, perm, 3 * H))
    perm = torch.tensor(list(perm), dtype=torch.long)
    assert sorted(perm.tolist()) == list(range(3 * H))
    dxh, dvec, dx = Guarded(N, 3 * H), Guarded(3 * N, H), Guarded(N, H)
    drl = Guarded(E + 1, 3 * H)
    ok(lib.adf_op_message_bwd_fused(h, layer, d["xh"].data_ptr(), vptr, d["gx1"].data_ptr(), d["gv1"].data_ptr(), dxh.ptr,
                                    drl.ptr, E, None if first else dvec.ptr, dx.ptr, 1 if first else 0, None, s()))
    figs["bwd_fused_dxh"] = rel_err(dxh.result(), gw64[0])
    figs["bwd_fused_dx"] = rel_err(dx.result(), gw64[2])
    if not first:
        figs["bwd_fused_dvec"] = rel_err(dvec.result().reshape(N, 3, H), gw64[1])
    drp = drl.result()[:E].double()
    dW_a = torch.zeros(3 * H, R, dtype=torch.float64).index_add_(0, perm, drp.T @ rb64)
    db_a = torch.zeros(3 * H, dtype=torch.float64).index_add_(0, perm, drp.sum(0))
    figs["bwd_fused_drbfh_dW"], figs["bwd_fused_drbfh_db"] = rel_err(dW_a, gw64[3]), rel_err(db_a, gw64[4])
    # (b) nothing per edge: per-atom bias rows, then rbf_image + rbf_wgrad_fused ADD the weight gradient to random content
    ok(lib.adf_op_message_fwd_fused(h, layer, d["xh"].data_ptr(), vptr, d["x"].data_ptr(), x1.ptr, vec1.ptr, 1 if first else 0,
                                    s()))
    dxh, dvec, dx, brow = Guarded(N, 3 * H), Guarded(3 * N, H), Guarded(N, H), Guarded(N, 3 * H)
    ok(lib.adf_op_message_bwd_fused(h, layer, d["xh"].data_ptr(), vptr, d["gx1"].data_ptr(), d["gv1"].data_ptr(), dxh.ptr, None,
                                    E, None if first else dvec.ptr, dx.ptr, 1 if first else 0, brow.ptr, s()))
    figs["bwd_fused_b_dxh"] = rel_err(dxh.result(), gw64[0])
    figs["bwd_fused_b_dx"] = rel_err(dx.result(), gw64[2])
    if not first:
        figs["bwd_fused_b_dvec"] = rel_err(dvec.result().reshape(N, 3, H), gw64[1])
    figs["bwd_fused_bias_rows"] = rel_err(brow.result().double().sum(0), gw64[4])
    nbytes = int(lib.adf_op_rbf_image_bytes(E))
    image = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    ok(lib.adf_op_rbf_image(h, d["rbf"].data_ptr(), E, image.data_ptr(), s()))
    torch.cuda.synchronize()
    assert bool((image[nbytes:] == 0x5A).all()), "rbf_image wrote past adf_op_rbf_image_bytes"
    dW0 = torch.randn(3 * H, R, generator=g) * float(gw64[3].abs().mean())
    dW = Guarded(3 * H, R, init=dW0)
    sc = o.scratch(int(lib.adf_op_rbf_wgrad_fused_scratch(h)))
    own = owner[PAD:PAD + E].clone()
    ok(lib.adf_op_rbf_wgrad_fused(h, d["xh"].data_ptr(), vptr, image.data_ptr(), own.data_ptr(), E, dW.ptr, sc.data_ptr(),
                                  1 if first else 0, s()))
    figs["rbf_wgrad_fused"] = rel_err(dW.result().double() - dW0.double(), gw64[3])
    for k, e in figs.items():
        print(f"{k} {shape}: error {e:.2e}")
    bad = {k: e for k, e in figs.items() if not e < 2e-5}
    assert not bad, (shape, bad)
