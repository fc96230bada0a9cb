"""Training steps of the two EquiformerV2 mirrors on the device.

``EqV2TrainStep``: the score-matching step of the denoiser ``EquiformerV2S_OC20_DenoisingPos``, the counterpart of
``train_step.PaiNNTrainStep`` (``zero_grad``, ``loss_and_grad(batch, targets, grads_ready)`` accumulating into ``param.grad``,
``last_outputs``).  ``EqV2S2EFTrainStep``: the S2EF step of the force field ``EquiformerV2_OC20``, the counterpart of
``train_step.PaiNNS2EFTrainStep``.  Both keep their PaiNN twin's contract, so the trainers, the optimizers, the EMA, the
gradient reducer and the checkpoints work on them unchanged; what they share - embedding, block loop, masks, ``groups``, the
``grads_ready`` hooks - is ``_EqV2StepBase``.  ``EqV2EnergyGradient`` is its third user: the S2EF model's energy
and forces = -dE/dpos of that energy, the backward taken with respect to the edge geometry instead of the weights
(csrc/eqv2_geo.hip).

Where the arithmetic runs:

* EDGE side (E rows; everything ``oracle/eqv2_oracle.py::attention_block`` does per edge, and the edge-degree embedding):
  hand-written HIP behind the stateless ``adf_op_eq_*`` entries (csrc/eqv2_train.hip; the S2EF model's live Gaussian basis:
  csrc/eqv2_s2ef_train.hip), forward and backward, on the graph ``EqV2Engine.export_graph`` hands out.  Each entry is
  wrapped here in a ``torch.autograd.Function`` that owns its saved activations; torch only chains them.
* NODE side (N rows: ``norm_sh``, SO(3) linears, the feed-forward network, the element embedding, the conditional
  model's energy term, the S2EF model's energy head): plain torch operations on the device under autograd, written so that
  no backward uses a float atomic (no gather by index: per-degree slices, a one-hot product for the per-system terms, the
  ordered embedding backward ``adf_op_embed_bwd_ordered``).

Exact f32 throughout, no float atomics: two calls on the same input give the same bits.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from . import lib as _lib
from . import so3_math
from .so3_tables import Igso3Tables


# ------------------------------------------------------------------------------------------------------- graph + entries
class EqGraph:
    """The engine's graph of one batch plus the source-sorted permutation the rotate-in backward sums along."""

    def __init__(self, engine, data, prep) -> None:
        self.prep = prep
        self.eptr, self.src, self.dst, self.vec, self.wig = engine.export_graph(data, prep)
        self.N, self.E = prep.num_atoms, int(self.src.numel())
        self.Z = prep.atomic_numbers                                  # [N] int32
        dev = self.src.device
        order = torch.sort(self.src.long(), stable=True).indices       # ties keep the list order
        self.sperm = order.to(torch.int32).contiguous()
        self.sptr = torch.zeros(self.N + 1, dtype=torch.int32, device=dev)
        self.sptr[1:] = torch.cumsum(torch.bincount(self.src.long(), minlength=self.N), 0).to(torch.int32)
        # 1-based element of every edge's source / target: the row lists of adf_op_embed_bwd_ordered
        self.zs1 = (self.Z[self.src.long()] + 1).contiguous()
        self.zt1 = (self.Z[self.dst.long()] + 1).contiguous()
        self.ones = None
        self.dist = self.dperm = None   # EqOps.edge_distances (the S2EF model's live basis)
        # accumulators of the geometric gradient, dE/dwig [E, DR] and dE/d|vec| [E]: present only while EqV2EnergyGradient
        # differentiates with respect to the edge vectors; the backward of RotateIn, RotateOut and RadialMLPLive adds into them
        self.dwig = self.ddist = None
        self.geo = None                 # the leaf that makes autograd walk a graph none of whose parameters asks for a gradient


class EqOps:
    """Typed wrappers over the adf_op_eq_* entries for one engine (dimensions and constant tables come from its handle)."""

    def __init__(self, engine) -> None:
        m = engine.model
        self.engine, self.lib, self.h, self.dev = engine, engine.lib, engine.handle, engine.device
        self.L, self.M, self.C = engine.lmax, engine.mmax, int(m.sphere_channels)
        L, M = self.L, self.M
        self.S = (L + 1) ** 2
        self.Sr = sum(2 * min(l, M) + 1 for l in range(L + 1))
        self.RW = sum(L - mm + 1 for mm in range(M + 1))
        self.rbase = [0] * (M + 1)
        r = L + 1
        for mm in range(1, M + 1):
            self.rbase[mm] = r
            r += 2 * (L - mm + 1)
        self.NH, self.A, self.V = int(m.num_heads), int(m.attn_alpha_channels), int(m.attn_value_channels)
        self.Hd, self.EC, self.NB = int(m.attn_hidden_channels), int(m.edge_channels), int(m.NUM_GAUSSIANS)
        self.NE = int(m.max_num_elements)
        self._scratch = torch.empty(0, device=self.dev)

    def s(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def new(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    def zeros(self, *shape) -> torch.Tensor:
        return torch.zeros(*shape, dtype=torch.float32, device=self.dev)

    def scratch(self, n: int) -> torch.Tensor:
        if self._scratch.numel() < n:
            self._scratch = torch.empty(int(n * 1.25) + 1024, device=self.dev)
        return self._scratch

    @staticmethod
    def _p(t: Optional[torch.Tensor], off: int = 0):
        return None if t is None else t.data_ptr() + 4 * off

    # ---- dense rows
    def linear(self, A, W, bias, Cm, M, N, K, a_off=0, lda=None, w_off=0, ldw=None, b_off=0, c_off=0, ldc=None, acc=False):
        _lib.check(self.lib.adf_op_eq_linear_fwd(self._p(A, a_off), lda or K, self._p(W, w_off), ldw or K, self._p(bias, b_off),
                                                 self._p(Cm, c_off), ldc or N, 1 if acc else 0, M, N, K, self.s()))
        return Cm

    def linear_bwd(self, A, W, dC, M, N, K, dA=None, dW=None, db=None, a_off=0, lda=None, w_off=0, ldw=None, c_off=0, ldc=None,
                   da_off=0, ldda=None, acc_dA=False, dw_off=0, lddw=None, db_off=0):
        _lib.check(self.lib.adf_op_eq_linear_bwd(
            self._p(A, a_off), lda or K, self._p(W, w_off), ldw or K, self._p(dC, c_off), ldc or N, self._p(dA, da_off),
            ldda or K, 1 if acc_dA else 0, self._p(dW, dw_off), lddw or K, self._p(db, db_off), M, N, K, self.s()))

    def silu(self, x):
        y = torch.empty_like(x)
        _lib.check(self.lib.adf_op_eq_silu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), self.s()))
        return y

    def silu_bwd(self, x, dy):
        dx = torch.empty_like(x)
        _lib.check(self.lib.adf_op_eq_silu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), self.s()))
        return dx

    def layernorm(self, x, w, b):
        rows, H = x.shape
        y, stats = torch.empty_like(x), self.new(rows, 2)
        _lib.check(self.lib.adf_op_layernorm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), stats.data_ptr(), rows,
                                                 H, self.s()))
        return y, stats

    def layernorm_bwd(self, x, w, stats, dy):
        rows, H = x.shape
        dx, dw, db = torch.zeros_like(x), self.new(H), self.new(H)
        _lib.check(self.lib.adf_op_layernorm_bwd(x.data_ptr(), w.data_ptr(), stats.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                                                 dw.data_ptr(), db.data_ptr(), rows, H, self.scratch(1024 * H).data_ptr(),
                                                 self.s()))
        return dx, dw, db

    def embed_bwd(self, dx, idx1, rows):
        """demb [rows, H] with demb[idx1[n] - 1] = sum of dx[n] in a fixed order; rows of absent indices stay exactly zero."""
        n, H = dx.shape
        demb = self.zeros(rows, H)
        if n:
            sc = self.scratch(int(self.lib.adf_op_embed_bwd_ordered_scratch(n, H, rows)))
            _lib.check(self.lib.adf_op_embed_bwd_ordered(dx.data_ptr(), idx1.data_ptr(), demb.data_ptr(), n, H, rows,
                                                         sc.data_ptr(), self.s()))
        return demb

    def edge_scalars(self, g: EqGraph, semb, temb):
        out = self.new(g.E, self.NB + 2 * self.EC)
        _lib.check(self.lib.adf_op_eq_edge_scalars(self.h, g.Z.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(), g.vec.data_ptr(),
                                                   semb.data_ptr(), temb.data_ptr(), g.E, out.data_ptr(), self.s()))
        return out

    # ---- the live Gaussian basis of the S2EF model (csrc/eqv2_s2ef_train.h)
    def edge_distances(self, g: EqGraph):
        """(dist [E], perm [E]) of the graph, formed once per step: the kernels' |vec| and the edges sorted by it (stable:
        ties in list order), the one order adf_op_eq_radial_gauss_bwd sums a column in."""
        if g.dist is None:
            g.dist = self.new(g.E)
            if g.E:
                _lib.check(self.lib.adf_op_eq_edge_dist(_c(g.vec).data_ptr(), g.E, g.dist.data_ptr(), self.s()))
            g.dperm = torch.sort(g.dist, stable=True).indices.to(torch.int32).contiguous()
        return g.dist, g.dperm

    def gauss_fwd(self, g: EqGraph, W0, h0):
        dist, _ = self.edge_distances(g)
        sc = self.scratch(self.NB * self.EC)
        if g.E:
            _lib.check(self.lib.adf_op_eq_radial_gauss_fwd(self.h, dist.data_ptr(), W0.data_ptr(), W0.stride(0), g.E,
                                                           h0.data_ptr(), sc.data_ptr(), sc.numel(), self.s()))
        return h0

    def gauss_bwd(self, g: EqGraph, dh0, dW0):
        dist, perm = self.edge_distances(g)
        sc = self.scratch(4 * g.E)
        if g.E:
            _lib.check(self.lib.adf_op_eq_radial_gauss_bwd(self.h, dist.data_ptr(), perm.data_ptr(), dh0.data_ptr(), g.E,
                                                           dW0.data_ptr(), dW0.stride(0), sc.data_ptr(), sc.numel(), self.s()))
        return dW0


    # ---- the geometric gradient (csrc/eqv2_geo.h)
    def gauss_dgrad(self, g: EqGraph, W0, dh0):
        dist, _ = self.edge_distances(g)
        sc = self.scratch(self.NB * self.EC)
        if g.E:
            _lib.check(self.lib.adf_op_eq_radial_gauss_dgrad(self.h, dist.data_ptr(), W0.data_ptr(), W0.stride(0), dh0.data_ptr(),
                                                             g.E, g.ddist.data_ptr(), sc.data_ptr(), sc.numel(), self.s()))

    def geometry_to_forces(self, g: EqGraph):
        """forces [N, 3] = -dE/dpos from the graph's accumulators (``adf_op_eq_wigner_bwd``, ``adf_op_eq_edge_grad_to_atoms``)."""
        dvec, forces = self.new(g.E, 3), self.new(g.N, 3)
        if g.E:
            _lib.check(self.lib.adf_op_eq_wigner_bwd(self.h, _c(g.vec).data_ptr(), _c(g.wig).data_ptr(), g.dwig.data_ptr(),
                                                     g.ddist.data_ptr(), g.E, dvec.data_ptr(), self.s()))
        _lib.check(self.lib.adf_op_eq_edge_grad_to_atoms(self._p(dvec) if g.E else None, g.eptr.data_ptr(), g.sptr.data_ptr(),
                                                         g.sperm.data_ptr() if g.E else None, g.N, g.E, forces.data_ptr(),
                                                         self.s()))
        return forces


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------------- edge operators
def _radial_tail_fwd(ops: EqOps, E, pad, h0, w1, b1, W3, b3, w4, b4, W6, b6):
    """LayerNorm, SiLU, Linear, LayerNorm, SiLU, Linear behind a radial MLP's first layer h0 [E, EC] -> (out, its row
    stride, the activations the backward reads)."""
    EC, OUT = ops.EC, W6.shape[0]
    y1, st1 = ops.layernorm(h0, w1, b1)
    a1 = ops.silu(y1)
    h3 = ops.linear(a1, W3, b3, ops.new(E, EC), E, EC, EC)
    y4, st4 = ops.layernorm(h3, w4, b4)
    a4 = ops.silu(y4)
    ld = int(pad) if pad else OUT
    out = ops.zeros(E, ld) if ld > OUT else ops.new(E, ld)
    ops.linear(a4, W6, b6, out, E, OUT, EC, ldc=ld)
    return out, ld, (st1, y1, a1, h3, st4, y4, a4)


def _radial_tail_bwd(ops: EqOps, E, ld, dout, w1, W3, w4, W6, h0, st1, y1, a1, h3, st4, y4, a4, wgrad=True):
    """-> dh0 and the gradients of net.1 .. net.6 (dw1, db1, dW3, db3, dw4, db4, dW6, db6); ``wgrad`` off: the data path
    alone, the two weight products are not formed (dW6, db6, dW3, db3 are None)."""
    EC, OUT = ops.EC, W6.shape[0]
    dout = _c(dout)
    dW6, db6 = (torch.zeros_like(W6), ops.zeros(OUT)) if wgrad else (None, None)
    da4 = ops.new(E, EC)
    ops.linear_bwd(a4, W6, dout, E, OUT, EC, dA=da4, dW=dW6, db=db6, ldc=ld)
    dh3, dw4, db4 = ops.layernorm_bwd(h3, w4, st4, ops.silu_bwd(y4, da4))
    dW3, db3 = (torch.zeros_like(W3), ops.zeros(EC)) if wgrad else (None, None)
    da1 = ops.new(E, EC)
    ops.linear_bwd(a1, W3, dh3, E, EC, EC, dA=da1, dW=dW3, db=db3)
    dh0, dw1, db1 = ops.layernorm_bwd(h0, w1, st1, ops.silu_bwd(y1, da1))
    return dh0, dw1, db1, dW3, db3, dw4, db4, dW6, db6


class RadialMLP(torch.autograd.Function):
    """Linear, LayerNorm, SiLU, Linear, LayerNorm, SiLU, Linear on the E rows [basis | semb[Z_src] | temb[Z_dst]]
    (oracle ``radial_mlp``); ``pad``: row stride of the output (> its width: the columns behind it are zero)."""

    @staticmethod
    def forward(ctx, ops: EqOps, g: EqGraph, pad, semb, temb, W0, b0, w1, b1, W3, b3, w4, b4, W6, b6):
        E, EC, IN, OUT = g.E, ops.EC, ops.NB + 2 * ops.EC, W6.shape[0]
        scal = ops.edge_scalars(g, semb, temb)
        h0 = ops.linear(scal, W0, b0, ops.new(E, EC), E, EC, IN)
        out, ld, (st1, y1, a1, h3, st4, y4, a4) = _radial_tail_fwd(ops, E, pad, h0, w1, b1, W3, b3, w4, b4, W6, b6)
        ctx.ops, ctx.g, ctx.ld = ops, g, ld
        ctx.save_for_backward(semb, temb, W0, w1, W3, w4, W6, h0, st1, y1, a1, h3, st4, y4, a4)
        return out

    @staticmethod
    def backward(ctx, dout):
        ops, g, ld = ctx.ops, ctx.g, ctx.ld
        semb, temb, W0, w1, W3, w4, W6, h0, st1, y1, a1, h3, st4, y4, a4 = ctx.saved_tensors
        E, EC, NB = g.E, ops.EC, ops.NB
        IN = NB + 2 * EC
        dh0, dw1, db1, dW3, db3, dw4, db4, dW6, db6 = _radial_tail_bwd(ops, E, ld, dout, w1, W3, w4, W6, h0, st1, y1, a1, h3, st4,
                                                                       y4, a4)
        scal = ops.edge_scalars(g, semb, temb)            # formed again, not kept: 4 (NB + 2 EC) bytes per edge
        dW0, db0 = torch.zeros_like(W0), ops.zeros(EC)
        ops.linear_bwd(scal, W0, dh0, E, EC, IN, dW=dW0, db=db0)
        demb = ops.new(E, 2 * EC)                         # the embedding columns of d scal only
        ops.linear_bwd(None, W0, dh0, E, EC, 2 * EC, dA=demb, w_off=NB, ldw=IN)
        dsemb = ops.embed_bwd(_c(demb[:, :EC]), g.zs1, ops.NE)
        dtemb = ops.embed_bwd(_c(demb[:, EC:]), g.zt1, ops.NE)
        return None, None, None, dsemb, dtemb, dW0, db0, dw1, db1, dW3, db3, dw4, db4, dW6, db6


class RadialMLPLive(torch.autograd.Function):
    """``RadialMLP`` for the S2EF model: the Gaussian basis of the plain distance is live on every edge and
    is the inference forward's (csrc/eqv2_gauss.h).  The first layer is never formed as an [E, NB + 2 EC] product:
    h0 = b0 + Ps[Z_src] + Pt[Z_dst] + (the Gaussian window, ``adf_op_eq_radial_gauss_fwd``) with the element-sized tables
    Ps = semb W0[:, NB:NB+EC]^T and Pt = temb W0[:, NB+EC:]^T.  Backward: the window's weight gradient
    (``adf_op_eq_radial_gauss_bwd``), the gather's through ``adf_op_embed_bwd_ordered``, db0 a column sum in row order.
    ``geo`` (optional; ``EqGraph.geo``): when no parameter asks for a gradient, the backward takes the data path alone and
    adds d/d|vec| of the Gaussian window into ``g.ddist`` (``adf_op_eq_radial_gauss_dgrad``)."""

    @staticmethod
    def forward(ctx, ops: EqOps, g: EqGraph, pad, semb, temb, W0, b0, w1, b1, W3, b3, w4, b4, W6, b6, geo=None):
        E, EC, NB = g.E, ops.EC, ops.NB
        Ps, Pt = semb @ W0[:, NB:NB + EC].t(), temb @ W0[:, NB + EC:].t()        # [max_num_elements, EC]
        h0 = _c(b0[None, :] + Ps[g.zs1.long() - 1] + Pt[g.zt1.long() - 1])
        ops.gauss_fwd(g, W0, h0)
        out, ld, (st1, y1, a1, h3, st4, y4, a4) = _radial_tail_fwd(ops, E, pad, h0, w1, b1, W3, b3, w4, b4, W6, b6)
        ctx.ops, ctx.g, ctx.ld = ops, g, ld
        ctx.save_for_backward(semb, temb, W0, w1, W3, w4, W6, h0, st1, y1, a1, h3, st4, y4, a4)
        return out

    @staticmethod
    def backward(ctx, dout):
        ops, g, ld = ctx.ops, ctx.g, ctx.ld
        semb, temb, W0, w1, W3, w4, W6, h0, st1, y1, a1, h3, st4, y4, a4 = ctx.saved_tensors
        E, EC, NB = g.E, ops.EC, ops.NB
        wgrad = any(ctx.needs_input_grad[3:15])
        dh0, dw1, db1, dW3, db3, dw4, db4, dW6, db6 = _radial_tail_bwd(ops, E, ld, dout, w1, W3, w4, W6, h0, st1, y1, a1, h3, st4,
                                                                       y4, a4, wgrad)
        if getattr(g, "ddist", None) is not None:      # (a graph stand-in of a test carries no accumulators)
            ops.gauss_dgrad(g, W0, dh0)
        if not wgrad:
            return (None,) * 16
        dW0, db0 = torch.zeros_like(W0), ops.zeros(EC)
        ops.gauss_bwd(g, dh0, dW0)
        ops.linear_bwd(None, None, dh0, E, EC, 1, db=db0)
        dPs, dPt = ops.embed_bwd(dh0, g.zs1, ops.NE), ops.embed_bwd(dh0, g.zt1, ops.NE)
        Ws, Wt = W0[:, NB:NB + EC], W0[:, NB + EC:]
        dW0[:, NB:NB + EC] = dPs.t() @ semb
        dW0[:, NB + EC:] = dPt.t() @ temb
        return None, None, None, dPs @ Ws, dPt @ Wt, dW0, db0, dw1, db1, dW3, db3, dw4, db4, dW6, db6, None


class RotateIn(torch.autograd.Function):
    """[x[src] | x[dst]] into the edges' frames (rows |m| <= mmax, order-major) times the radial weights."""

    @staticmethod
    def forward(ctx, ops: EqOps, g: EqGraph, x, radial):
        x, radial = _c(x), _c(radial)
        out = ops.new(g.E, ops.Sr, 2 * ops.C)
        _lib.check(ops.lib.adf_op_eq_rotate_in_fwd(ops.h, x.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(), g.wig.data_ptr(),
                                                   radial.data_ptr(), g.E, out.data_ptr(), ops.s()))
        ctx.ops, ctx.g = ops, g
        ctx.save_for_backward(x, radial)
        return out

    @staticmethod
    def backward(ctx, dout):
        ops, g = ctx.ops, ctx.g
        x, radial = ctx.saved_tensors
        dout = _c(dout)
        dradial, dx = torch.empty_like(radial), torch.empty_like(x)
        _lib.check(ops.lib.adf_op_eq_rotate_in_bwd(
            ops.h, x.data_ptr(), g.eptr.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(), g.wig.data_ptr(), radial.data_ptr(),
            dout.data_ptr(), g.sptr.data_ptr(), g.sperm.data_ptr(), g.N, g.E, dradial.data_ptr(), dx.data_ptr(), ops.s()))
        if getattr(g, "dwig", None) is not None:
            _lib.check(ops.lib.adf_op_eq_rotate_in_bwd_wig(ops.h, x.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(),
                                                           radial.data_ptr(), dout.data_ptr(), g.E, g.dwig.data_ptr(), ops.s()))
        return None, None, dx, dradial


def _so2_block_weight(W, h, k):
    """[[Wr, -Wi], [Wi, Wr]] of fc.weight = [Wr; Wi]: the (+m, -m) pair mixed like a complex product as ONE map on
    [x(+m) | x(-m)] (plus = Wr x+ - Wi x-, minus = Wi x+ + Wr x-; so2_ops.py:52-66)."""
    Wr, Wi = W[:h], W[h:]
    return torch.cat([torch.cat([Wr, -Wi], 1), torch.cat([Wi, Wr], 1)], 0).contiguous()


class SO2Conv(torch.autograd.Function):
    """SO(2) convolution on order-major coefficients x [E, S_r, cin] -> out [E, S_r, cout] and the `extra` scalar outputs
    [E, extra] of fc_m0 (oracle ``so2_conv`` without the radial weighting, which RotateIn applies)."""

    @staticmethod
    def forward(ctx, ops: EqOps, x, extra, cout, W0, b0, *Wm):
        x = _c(x)
        E, Sr, cin = x.shape
        L, M = ops.L, ops.M
        K0 = (L + 1) * cin
        out = ops.new(E, Sr, cout)
        ex = ops.new(E, max(extra, 1))
        if extra:
            ops.linear(x, W0, b0, ex, E, extra, K0, lda=Sr * cin)
        ops.linear(x, W0, b0, out, E, (L + 1) * cout, K0, lda=Sr * cin, w_off=extra * K0, b_off=extra, ldc=Sr * cout)
        Wbs = []
        for mm in range(1, M + 1):
            nm = L - mm + 1
            h, k = nm * cout, nm * cin
            Wb = _so2_block_weight(Wm[mm - 1], h, k)
            Wbs.append(Wb)
            ops.linear(x, Wb, None, out, E, 2 * h, 2 * k, a_off=ops.rbase[mm] * cin, lda=Sr * cin, c_off=ops.rbase[mm] * cout,
                       ldc=Sr * cout)
        ctx.ops, ctx.extra, ctx.cout = ops, extra, cout
        ctx.save_for_backward(x, W0, *Wbs)
        ctx.mark_non_differentiable(*([] if extra else [ex]))
        return out, ex

    @staticmethod
    def backward(ctx, dout, dex):
        ops, extra, cout = ctx.ops, ctx.extra, ctx.cout
        x, W0, *Wbs = ctx.saved_tensors
        E, Sr, cin = x.shape
        L, M = ops.L, ops.M
        K0 = (L + 1) * cin
        dout = _c(dout)
        dx = torch.empty_like(x)
        wgrad = any(ctx.needs_input_grad[4:])     # off: the data gradient alone, no weight product is formed
        dW0, db0 = (torch.zeros_like(W0), ops.zeros(W0.shape[0])) if wgrad else (None, None)
        ops.linear_bwd(x, W0, dout, E, (L + 1) * cout, K0, dA=dx, dW=dW0, db=db0, lda=Sr * cin, w_off=extra * K0, ldc=Sr * cout,
                       ldda=Sr * cin, dw_off=extra * K0, db_off=extra)
        if extra and dex is not None:
            dex = _c(dex)
            ops.linear_bwd(x, W0, dex, E, extra, K0, dA=dx, dW=dW0, db=db0, lda=Sr * cin, ldda=Sr * cin, acc_dA=True)
        dWm = []
        for mm in range(1, M + 1):
            nm = L - mm + 1
            h, k = nm * cout, nm * cin
            dWb = torch.zeros_like(Wbs[mm - 1]) if wgrad else None
            ops.linear_bwd(x, Wbs[mm - 1], dout, E, 2 * h, 2 * k, dA=dx, dW=dWb, a_off=ops.rbase[mm] * cin, lda=Sr * cin,
                           c_off=ops.rbase[mm] * cout, ldc=Sr * cout, da_off=ops.rbase[mm] * cin, ldda=Sr * cin)
            dWm.append(torch.cat([dWb[:h, :k] + dWb[h:, k:], dWb[h:, :k] - dWb[:h, k:]], 0) if wgrad else None)
        return (None, dx, None, None, dW0, db0, *dWm)


class S2Act(torch.autograd.Function):
    """Separable S2 activation: SiLU on the gate columns of `ex` for l = 0, point-wise SiLU on the reduced grid for the rest."""

    @staticmethod
    def forward(ctx, ops: EqOps, y, ex, gate_off):
        y, ex = _c(y), _c(ex)
        E, Sr, W = y.shape
        out = torch.empty_like(y)
        _lib.check(ops.lib.adf_op_eq_s2act_fwd(ops.h, y.data_ptr(), ops._p(ex, gate_off), ex.shape[1], W, E, out.data_ptr(),
                                               ops.s()))
        ctx.ops, ctx.gate_off = ops, gate_off
        ctx.save_for_backward(y, ex)
        return out

    @staticmethod
    def backward(ctx, dout):
        ops, gate_off = ctx.ops, ctx.gate_off
        y, ex = ctx.saved_tensors
        E, Sr, W = y.shape
        dout = _c(dout)
        dy, dex = torch.empty_like(y), torch.zeros_like(ex)
        _lib.check(ops.lib.adf_op_eq_s2act_bwd(ops.h, y.data_ptr(), ops._p(ex, gate_off), ex.shape[1], dout.data_ptr(), W, E,
                                               dy.data_ptr(), ops._p(dex, gate_off), ex.shape[1], ops.s()))
        return None, dy, dex, None


class AttnWeights(torch.autograd.Function):
    """LayerNorm over a head's alpha channels, smooth leaky ReLU, dot with alpha_dot, softmax over a target's edges, dropout
    mask -> alpha [E, heads].  `ex` [E, extra]: the alpha channels are its first heads * alpha columns."""

    @staticmethod
    def forward(ctx, ops: EqOps, g: EqGraph, ex, ln_w, ln_b, adot, mask):
        ex = _c(ex)
        soft, alpha = ops.new(g.E, ops.NH), ops.new(g.E, ops.NH)
        mask = None if mask is None else _c(mask.to(torch.float32))
        _lib.check(ops.lib.adf_op_eq_alpha_fwd(ops.h, ex.data_ptr(), ex.shape[1], ln_w.data_ptr(), ln_b.data_ptr(),
                                               adot.data_ptr(), g.eptr.data_ptr(), ops._p(mask), g.N, g.E, soft.data_ptr(),
                                               alpha.data_ptr(), ops.s()))
        ctx.ops, ctx.g, ctx.mask = ops, g, mask
        ctx.save_for_backward(ex, ln_w, ln_b, adot, soft)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        ops, g, mask = ctx.ops, ctx.g, ctx.mask
        ex, ln_w, ln_b, adot, soft = ctx.saved_tensors
        dalpha = _c(dalpha)
        HA = ops.NH * ops.A
        dex = torch.zeros_like(ex)
        if any(ctx.needs_input_grad[3:6]):
            dw, db, dadot = torch.zeros_like(ln_w), torch.zeros_like(ln_b), torch.zeros_like(adot)
        else:
            dw = db = dadot = None     # the entry then skips its parameter pass
        need = 3 * g.E * ops.NH + (3 * ((g.E + 255) // 256) + 2) * HA
        sc = ops.scratch(need)
        _lib.check(ops.lib.adf_op_eq_alpha_bwd(
            ops.h, ex.data_ptr(), ex.shape[1], ln_w.data_ptr(), ln_b.data_ptr(), adot.data_ptr(), g.eptr.data_ptr(),
            ops._p(mask), soft.data_ptr(), dalpha.data_ptr(), g.N, g.E, dex.data_ptr(), ex.shape[1], ops._p(dw),
            ops._p(db), ops._p(dadot), sc.data_ptr(), sc.numel(), ops.s()))
        return None, None, dex, dw, db, dadot, None


class RotateOut(torch.autograd.Function):
    """alpha-weighted rotation back (D^T with the truncation rescale) summed over a target's edges -> [N, S, heads * V]."""

    @staticmethod
    def forward(ctx, ops: EqOps, g: EqGraph, z, alpha, NH, V, only_l):
        z, alpha = _c(z), _c(alpha)
        agg = ops.new(g.N, ops.S, NH * V)
        _lib.check(ops.lib.adf_op_eq_rotate_out_fwd(ops.h, z.data_ptr(), alpha.data_ptr(), NH, V, g.eptr.data_ptr(),
                                                    g.wig.data_ptr(), only_l, g.N, agg.data_ptr(), ops.s()))
        ctx.ops, ctx.g, ctx.dims = ops, g, (NH, V, only_l)
        ctx.save_for_backward(z, alpha)
        return agg

    @staticmethod
    def backward(ctx, dagg):
        ops, g, (NH, V, only_l) = ctx.ops, ctx.g, ctx.dims
        z, alpha = ctx.saved_tensors
        dagg = _c(dagg)
        dz, dalpha = torch.empty_like(z), torch.empty_like(alpha)
        _lib.check(ops.lib.adf_op_eq_rotate_out_bwd(ops.h, z.data_ptr(), alpha.data_ptr(), NH, V, g.dst.data_ptr(),
                                                    g.wig.data_ptr(), dagg.data_ptr(), only_l, g.E, dz.data_ptr(),
                                                    dalpha.data_ptr(), ops.s()))
        if getattr(g, "dwig", None) is not None:
            _lib.check(ops.lib.adf_op_eq_rotate_out_bwd_wig(ops.h, z.data_ptr(), alpha.data_ptr(), NH, V, g.dst.data_ptr(),
                                                            dagg.data_ptr(), only_l, g.E, g.dwig.data_ptr(), ops.s()))
        return None, None, dz, dalpha, None, None, None


class OrderedEmbedding(torch.autograd.Function):
    """weight[Z] with the backward summed in a fixed order (``adf_op_embed_bwd_ordered``); absent rows get exactly zero."""

    @staticmethod
    def forward(ctx, ops: EqOps, weight, Z):
        ctx.ops, ctx.rows = ops, weight.shape[0]
        ctx.save_for_backward(Z)
        return weight[Z.long()]

    @staticmethod
    def backward(ctx, dx):
        (Z,) = ctx.saved_tensors
        return None, ctx.ops.embed_bwd(_c(dx), (Z + 1).contiguous(), ctx.rows), None


# ------------------------------------------------------------------------------------------------------- node side (torch)
def _mm(x, W, fold: bool = False):
    """x [..., K] @ W^T.  ``fold`` off (the training steps): torch.matmul as ever.  ``fold`` on (``EqV2EnergyGradient``, whose
    weights ask for no gradient): ONE product on the rows of x, written out.  That is what torch.matmul itself runs for a weight
    that asks for a gradient - it folds the leading dimensions and calls mm - while for one that asks for none it may run a
    batched product with other bits; folded, the energy-gradient forward reproduces the training forward's bits
    (tests/test_gpu_eqv2_grad_forces.py::test_reported_energy)."""
    if not fold:
        return x @ W.t()
    return (x.reshape(-1, x.shape[-1]) @ W.t()).reshape(*x.shape[:-1], W.shape[0])


def so3_linear(weight, bias, x, L: int, fold: bool = False):
    """One weight matrix per degree, bias on l = 0 (so3.py:694-745); per-degree slices, no gather."""
    out = []
    for l in range(L + 1):
        y = _mm(x[:, l * l:(l + 1) ** 2], weight[l], fold)
        out.append(y + bias if l == 0 else y)
    return torch.cat(out, 1)


def norm_sh(affine, w0, b0, x, L: int, eps: float = 1e-5):
    """layer_norm_sh (layer_norm.py:129-250): LayerNorm on l = 0, one degree-balanced RMS over l > 0."""
    x0 = x[:, :1]
    mu = x0.mean(-1, keepdim=True)
    var = ((x0 - mu) ** 2).mean(-1, keepdim=True)
    out = [(x0 - mu) * torch.rsqrt(var + eps) * w0 + b0]
    ms = 0.0
    for l in range(1, L + 1):
        ms = ms + (x[:, l * l:(l + 1) ** 2] ** 2).sum(1) / ((2 * l + 1) * L)     # [N, C]
    scale = torch.rsqrt(ms.mean(1) + eps)[:, None, None]
    for l in range(1, L + 1):
        out.append(x[:, l * l:(l + 1) ** 2] * scale * affine[l - 1][None, None, :])
    return torch.cat(out, 1)


# ------------------------------------------------------------------------------------------------------- the step
def _rad_params(P, pre):
    return [P[pre + f"net.{i}.{k}"] for i in (0, 1, 3, 4, 6) for k in ("weight", "bias")]


def mask_generator(device, seed: int, step: int) -> torch.Generator:
    """The device generator of a step's dropout / drop-path draws: a function of (seed, step) alone."""
    gen = torch.Generator(device=device)
    gen.manual_seed((int(seed) * 1000003 + int(step) * 7919 + 12345) & 0x7FFFFFFFFFFFFFFF)
    return gen


class _EqV2StepBase:
    """What the training steps of both EquiformerV2 mirrors share: the element embedding, the edge-degree embedding, the
    block loop and the final norm as a graph of the operators above (``_trunk``), an attention block and a feed-forward
    network, the dropout / drop-path masks, ``zero_grad``, ``groups`` and the backward with its ``grads_ready`` hooks.  A
    subclass adds its heads and its objective."""

    # no path to the loss: the reference's autograd leaves them at None
    UNUSED_PREFIXES: tuple = ()
    # the parameters whose gradients are final first (``groups``): the heads and the final norm
    HEAD_PREFIXES: tuple = ()
    # the radial MLP of this model: a basis that is identically zero (the denoiser, RadialMLP) or live (RadialMLPLive)
    radial = RadialMLP
    # False: the forward is the one of eval() whatever model.training says (no dropout, no drop path)
    stochastic = True
    # True: the node side's products are written as one folded product (``_mm``); the training steps keep torch.matmul
    fold_products = False

    def _params(self) -> dict:
        """name -> tensor the forward reads."""
        return dict(self.model.named_parameters())

    def _graph(self, eng, batch, prep) -> EqGraph:
        return EqGraph(eng, batch, prep)

    def _rows(self, fn, x):
        """``fn`` on the node rows ``x`` [N, ...] -> [N, ...] (``fn`` maps every atom's row on its own)."""
        return fn(x)

    def _setup(self, model, device) -> None:
        self.model = model
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs a ROCm device (the HIP path has no CPU fallback)")
        if float(getattr(model, "proj_drop", 0.0)) != 0.0:
            raise NotImplementedError("proj_drop != 0 is not offered by the EquiformerV2 training step")
        self.lib = _lib.load()
        self.ordered_embedding_backward = True   # always: kept for the trainer, which sets it on every step object
        self.mask_seed, self.mask_step = 0, 0
        self.last_outputs = None
        self.last_masks = None
        L, M = int(model.lmax_list[0]), int(model.mmax_list[0])
        t = so3_math.device_tables(L, M, int(model.grid_resolution))
        self._to_full = torch.from_numpy(t["to_full"]).to(self.dev)      # [G, S]
        self._from_full = torch.from_numpy(t["from_full"]).to(self.dev)
        self._scratch = torch.empty(0, device=self.dev)

    # ------------------------------------------------------------------ helpers
    def _unused(self, name: str) -> bool:
        return bool(self.UNUSED_PREFIXES) and name.startswith(self.UNUSED_PREFIXES)

    def _final_from_start(self, name: str) -> bool:
        """Parameters the graph never reaches although they count as used: their gradient is the zero tensor ``zero_grad``
        left.  A force block's output is its l = 1 rows, which proj.bias (l = 0) never reaches."""
        return name.startswith("force_block") and name.endswith("proj.bias")

    def zero_grad(self) -> None:
        for name, p in self.model.named_parameters():
            if not p.requires_grad:
                continue
            if self._unused(name):
                p.grad = None
            elif p.grad is None:
                p.grad = torch.zeros_like(p)
            else:
                p.grad.zero_()

    def groups(self) -> List[List[str]]:
        """Parameter names in the order their gradients become final: force blocks, blocks last to first, embeddings."""
        names = [n for n, p in self.model.named_parameters() if p.requires_grad and not self._unused(n)]
        out = [[n for n in names if n.startswith(self.HEAD_PREFIXES)]]
        for i in range(self.model.num_layers - 1, -1, -1):
            out.append([n for n in names if n.startswith(f"blocks.{i}.")])
        seen = {n for grp in out for n in grp}
        out.append([n for n in names if n not in seen])
        return [grp for grp in out if grp]

    def draw_masks(self, g: EqGraph, B: int) -> Optional[dict]:
        """The step's dropout masks from (mask_seed, mask_step): ``alpha`` [layers][E, heads] and ``path`` [layers, 2, B] of
        0 / 1 (1 = kept), or None when both rates are 0."""
        m = self.model
        pa, pp = float(getattr(m, "alpha_drop", 0.0)), float(getattr(m, "drop_path_rate", 0.0))
        if pa == 0.0 and pp == 0.0:
            return None
        gen = mask_generator(self.dev, self.mask_seed, self.mask_step)
        nl = m.num_layers
        path = (torch.rand(nl, 2, B, device=self.dev, generator=gen) >= pp).to(torch.float32)
        alpha = [(torch.rand(g.E, m.num_heads, device=self.dev, generator=gen) >= pa).to(torch.float32) for _ in range(nl)]
        return {"alpha": alpha, "path": path}

    # ------------------------------------------------------------------ forward pieces
    def _radial(self, ops: EqOps, g: EqGraph, pad, P, emb_pre: str, rad_pre: str):
        """The radial MLP of one attention block or of the edge-degree embedding on the graph's edges."""
        geo = () if getattr(g, "geo", None) is None else (g.geo,)
        return self.radial.apply(ops, g, pad, P[emb_pre + "source_embedding.weight"], P[emb_pre + "target_embedding.weight"],
                                 *_rad_params(P, rad_pre), *geo)

    def _attention(self, ops: EqOps, g: EqGraph, P, pre: str, x, mask, only_l: int):
        """SO2EquivariantGraphAttention (oracle ``attention_block``) -> [N, S, out_channels]."""
        NH, A, V, Hd = ops.NH, ops.A, ops.V, ops.Hd
        radial = self._radial(ops, g, 0, P, pre, pre + "so2_conv_1.rad_func.")
        msg = RotateIn.apply(ops, g, x, radial)
        extra = NH * A + Hd
        msg, ex = SO2Conv.apply(ops, msg, extra, Hd, P[pre + "so2_conv_1.fc_m0.weight"], P[pre + "so2_conv_1.fc_m0.bias"],
                                *[P[pre + f"so2_conv_1.so2_m_conv.{k}.fc.weight"] for k in range(ops.M)])
        msg = S2Act.apply(ops, msg, ex, NH * A)
        msg, _ = SO2Conv.apply(ops, msg, 0, NH * V, P[pre + "so2_conv_2.fc_m0.weight"], P[pre + "so2_conv_2.fc_m0.bias"],
                               *[P[pre + f"so2_conv_2.so2_m_conv.{k}.fc.weight"] for k in range(ops.M)])
        alpha = AttnWeights.apply(ops, g, ex, P[pre + "alpha_norm.weight"], P[pre + "alpha_norm.bias"], P[pre + "alpha_dot"],
                                  mask)
        agg = RotateOut.apply(ops, g, msg, alpha, NH, V, only_l)
        if only_l >= 0:   # the force blocks: the l = 1 rows alone reach the output
            sl = slice(only_l * only_l, (only_l + 1) ** 2)
            return agg[:, sl] @ P[pre + "proj.weight"][only_l].t()
        return self._rows(lambda a: so3_linear(P[pre + "proj.weight"], P[pre + "proj.bias"], a, ops.L, self.fold_products), agg)

    def _feed_forward(self, ops: EqOps, P, pre: str, x):
        F = torch.nn.functional
        fold = self.fold_products
        gate = F.silu(_mm(x[:, :1], P[pre + "scalar_mlp.0.weight"], fold) + P[pre + "scalar_mlp.0.bias"])
        h = so3_linear(P[pre + "so3_linear_1.weight"], P[pre + "so3_linear_1.bias"], x, ops.L, fold)
        gr = torch.einsum("gi,nic->ngc", self._to_full, h)
        gr = _mm(F.silu(_mm(F.silu(_mm(gr, P[pre + "grid_mlp.0.weight"], fold)), P[pre + "grid_mlp.2.weight"], fold)),
                 P[pre + "grid_mlp.4.weight"], fold)
        h = torch.einsum("gi,ngc->nic", self._from_full, gr)
        h = torch.cat([gate, h[:, 1:]], 1)
        return so3_linear(P[pre + "so3_linear_2.weight"], P[pre + "so3_linear_2.bias"], h, ops.L, fold)

    def _node_term(self, P, batch, prep):
        """What joins the element embedding on l = 0 ([N, C]), or None."""
        return None

    def _trunk(self, batch, masks=None):
        """Embedding, blocks and the final norm of the training forward -> (x [N, S, C], ops, graph, prep, P)."""
        m = self.model
        eng = m.engine(self.dev, refresh=False)
        ops = EqOps(eng)
        prep = eng.prepare(batch)
        g = self._graph(eng, batch, prep)
        P = self._params()
        N, B, L, C_ = g.N, prep.num_systems, ops.L, ops.C
        training = bool(m.training) and self.stochastic
        if not training:
            masks = None
        elif masks is None:
            masks = self.draw_masks(g, B)
        pa, pp = float(getattr(m, "alpha_drop", 0.0)), float(getattr(m, "drop_path_rate", 0.0))
        self.last_masks = masks
        # node embedding: element embedding (+ a subclass's term) on l = 0, plus the edge-degree embedding
        x0 = OrderedEmbedding.apply(ops, P["sphere_embedding.weight"], g.Z)
        term = self._node_term(P, batch, prep)
        if term is not None:
            x0 = x0 + term
        pre = "edge_degree_embedding."
        m0 = self._radial(ops, g, ops.Sr * C_, P, pre, pre + "rad_func.")
        if g.ones is None:
            g.ones = torch.ones(g.E, 1, device=self.dev)
        deg = RotateOut.apply(ops, g, m0.reshape(g.E, ops.Sr, C_), g.ones, 1, C_, -1) / float(m.avg_degree)
        x = torch.cat([deg[:, :1] + x0[:, None, :], deg[:, 1:]], 1)
        sysidx = prep.batch.long()
        for i in range(m.num_layers):
            p = f"blocks.{i}."
            amask = None
            if masks is not None and pa > 0.0:
                amask = masks["alpha"][i].to(self.dev, torch.float32) / (1.0 - pa)
            y = self._attention(ops, g, P, p + "ga.", self._rows(
                lambda r: norm_sh(P[p + "norm_1.affine_weight"], P[p + "norm_1.norm_l0.weight"], P[p + "norm_1.norm_l0.bias"], r, L),
                x), amask, -1)
            if masks is not None and pp > 0.0:
                y = y * (masks["path"][i, 0].to(self.dev, torch.float32) / (1.0 - pp))[sysidx][:, None, None]
            x = x + y
            y = self._rows(lambda r: self._feed_forward(ops, P, p + "ffn.", norm_sh(
                P[p + "norm_2.affine_weight"], P[p + "norm_2.norm_l0.weight"], P[p + "norm_2.norm_l0.bias"], r, L)), x)
            if masks is not None and pp > 0.0:
                y = y * (masks["path"][i, 1].to(self.dev, torch.float32) / (1.0 - pp))[sysidx][:, None, None]
            x = x + y
        x = self._rows(lambda r: norm_sh(P["norm.affine_weight"], P["norm.norm_l0.weight"], P["norm.norm_l0.bias"], r, L), x)
        return x, ops, g, prep, P

    def _force_head(self, ops: EqOps, g: EqGraph, P, hname: str, x):
        """A force block: the l = 1 rows of its attention, one channel -> [N, 3]."""
        return self._attention(ops, g, P, hname, x, None, 1)[:, :, 0].contiguous()

    def _require_zeroed(self) -> None:
        for name, p in self.model.named_parameters():
            if p.requires_grad and not self._unused(name) and p.grad is None:
                raise RuntimeError("call zero_grad() before loss_and_grad()")

    def _backward(self, outs, douts, grads_ready=None) -> None:
        """The operators' own backwards chained by autograd, seeded with ``douts``; a group of ``groups()`` is announced to
        ``grads_ready`` when its last gradient landed."""
        hooks = []
        if grads_ready is not None:
            P = dict(self.model.named_parameters())
            groups = self.groups()
            pending = [{n for n in grp if not self._final_from_start(n)} for grp in groups]
            state = {"next": 0}

            def landed(name):
                def hook(_):
                    for s in pending:
                        s.discard(name)
                    while state["next"] < len(groups) and not pending[state["next"]]:
                        grads_ready(list(groups[state["next"]]))
                        state["next"] += 1
                return hook

            for grp in groups:
                for name in grp:
                    hooks.append(P[name].register_post_accumulate_grad_hook(landed(name)))
        try:
            torch.autograd.backward(outs, douts)
        except torch.OutOfMemoryError as e:
            raise RuntimeError(f"HIP out of memory: {e}") from e
        finally:
            for hk in hooks:
                hk.remove()
        if grads_ready is not None:
            while state["next"] < len(groups):   # a group none of whose parameters the graph reached (no edges at all)
                grads_ready(list(groups[state["next"]]))
                state["next"] += 1
        if self.model.training:
            self.mask_step += 1


class EqV2TrainStep(_EqV2StepBase):
    """loss + gradients of the score-matching objective for a mirror ``EquiformerV2S_OC20_DenoisingPos`` on a ROCm device."""

    # no path to the loss (equiformer_v2_denoising.py:300-318): the reference's autograd leaves them at None
    UNUSED_PREFIXES = ("energy_block.",)
    HEAD_PREFIXES = ("force_block.", "force_block2.", "norm.")

    def __init__(self, model, device="cuda:0", igso3: Optional[Igso3Tables] = None) -> None:
        from .equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos

        if not isinstance(model, EquiformerV2S_OC20_DenoisingPos):
            raise NotImplementedError(f"EqV2TrainStep trains EquiformerV2S_OC20_DenoisingPos, got {type(model).__name__} "
                                      "(the EquiformerV2 S2EF force field's step is EqV2S2EFTrainStep)")
        self._setup(model, device)
        self.two_heads = bool(model.so3_denoising)
        self.igso3 = (igso3 or Igso3Tables.shared()) if self.two_heads else igso3

    def _unused(self, name: str) -> bool:
        if name.startswith(self.UNUSED_PREFIXES) or name == "atom_radii":
            return True
        return not self.two_heads and name.startswith("force_block2.")

    def _node_term(self, P, batch, prep):
        if getattr(self.model, "energy_embedding", None) is None:
            return None
        return self._energy_term(P, batch, prep)

    def _energy_term(self, P, batch, prep):
        """The conditional model's per-atom term (equiformer_v2_denoising.py:258-264): the layer runs in fp16 in the
        reference and in the inference forward, so the VALUE is fp16(fp16(e) fp16(W) + fp16(b)); the gradient is the one of
        e W + b (the rounding is passed straight through)."""
        m = self.model
        B, N = prep.num_systems, prep.num_atoms
        W, b = P["energy_embedding.weight"].reshape(-1), P["energy_embedding.bias"]
        if m.sampling:
            e = torch.zeros(B, device=self.dev)
        else:
            energy = getattr(batch, "energy", None)
            if energy is None:
                raise ValueError("the conditional EquiformerV2 (energy_encoding='scalar') with sampling=False reads "
                                 "data.energy (one value per system); the batch has none")
            e = torch.as_tensor(energy).to(self.dev, torch.float32).reshape(-1)
            if e.numel() != B:
                raise ValueError(f"data.energy has {e.numel()} values for {B} systems")
        t = e[:, None] * W[None, :] + b[None, :]
        t16 = (e.half().float()[:, None] * W.detach().half().float()[None, :] + b.detach().half().float()[None, :]).half().float()
        t = t + (t16 - t).detach()
        onehot = torch.zeros(N, B, device=self.dev)
        onehot[torch.arange(N, device=self.dev), prep.batch.long()] = 1.0
        return onehot @ t       # a product, not a gather: its backward needs no float atomic

    def forward(self, batch, masks=None):
        """The training forward -> (outputs [(N,3)] per head, graph, masks in force)."""
        x, ops, g, prep, P = self._trunk(batch, masks)
        outs = [self._force_head(ops, g, P, hname, x)
                for hname in (("force_block.", "force_block2.") if self.two_heads else ("force_block.",))]
        return outs, g, prep

    # ------------------------------------------------------------------ the step
    def loss_and_grad(self, batch, targets: dict, grads_ready=None, masks=None) -> torch.Tensor:
        """``PaiNNTrainStep.loss_and_grad``'s contract: accumulates into ``param.grad`` (call ``zero_grad`` first) and returns
        the device tensor (loss, translation term, rotation term; 0 for one head).  ``masks``: replaces the dropout /
        drop-path draws (``draw_masks``'s layout).  ``grads_ready(names)`` is called as soon as a group of parameters is
        final: the force blocks (with the final norm), then the blocks from the last to the first, then the embeddings."""
        lib = self.lib
        self._require_zeroed()
        if getattr(batch, "tags", None) is None:
            raise ValueError("batch.tags is required (tag 2 marks the adsorbate)")
        try:
            with torch.enable_grad():
                outs, g, prep = self.forward(batch, masks)
        except torch.OutOfMemoryError as e:   # as the rest of the library: an allocation failure is a RuntimeError
            raise RuntimeError(f"HIP out of memory: {e}") from e
        N, B = g.N, prep.num_systems
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        keys = ("tr_sigma", "rot_sigma", "tr_score", "rot_score") if self.two_heads else ("tr_sigma", "tr_score")
        t = {k: targets[k].to(self.dev, torch.float32).contiguous() for k in keys}
        loss = torch.empty(3, device=self.dev)
        douts = [torch.empty(N, 3, device=self.dev) for _ in outs]
        scratch = torch.empty(2 * B + 16, device=self.dev)
        f = [o.detach() for o in outs]
        with torch.cuda.device(self.dev):
            if self.two_heads:
                rot_norm = targets.get("rot_norm")
                if rot_norm is None:
                    from .noising import device_score_norm

                    rot_norm = device_score_norm(t["rot_sigma"], self.igso3, self.dev)
                rot_norm = rot_norm.to(self.dev, torch.float32).reshape(-1).contiguous()
                _lib.check(lib.adf_op_score_loss(f[0].data_ptr(), f[1].data_ptr(), prep.tags.data_ptr(),
                                                 prep.atom_offset.data_ptr(), t["tr_sigma"].data_ptr(), t["rot_sigma"].data_ptr(),
                                                 t["tr_score"].data_ptr(), t["rot_score"].data_ptr(), rot_norm.data_ptr(),
                                                 loss.data_ptr(), douts[0].data_ptr(), douts[1].data_ptr(), B, scratch.data_ptr(),
                                                 stream))
            else:
                _lib.check(lib.adf_op_score_loss_tr(f[0].data_ptr(), prep.tags.data_ptr(), prep.atom_offset.data_ptr(),
                                                    t["tr_sigma"].data_ptr(), t["tr_score"].data_ptr(), loss.data_ptr(),
                                                    douts[0].data_ptr(), B, scratch.data_ptr(), stream))
        self._backward(outs, douts, grads_ready)
        self.last_outputs = tuple(f)
        return loss


class EqV2S2EFTrainStep(_EqV2StepBase):
    """loss + gradients of the S2EF objective for a mirror ``equiformer_v2_oc20.EquiformerV2_OC20`` on a ROCm device
    (DESIGN.md 6h): ``PaiNNS2EFTrainStep``'s contract, so ``ForcesTrainer`` works on it unchanged.  The model's own forward
    (equiformer_v2_oc20.py:415-562) as a training graph: raw atomic numbers, the graph of the model's S2EF handle, the
    Gaussian basis live in all 1 + num_layers + 1 radial functions (``RadialMLPLive``), the energy head on the final-normed
    l = 0 row, one force block.  Energy loss "mae", force loss "l2mae" (``adf_op_s2ef_loss``); dE and dF seed the backward.

    Every parameter counts as used.  The parts of ``energy_block`` the l = 0 output does not depend on with the shipped
    switches (``so3_linear_1.*``, ``grid_mlp.*``, rows l >= 1 of ``so3_linear_2.weight``) take part in the reference's graph
    and get zero tensors there; here they keep the zeros ``zero_grad`` wrote - nothing is evaluated through the grid - so the
    optimizer's weight decay acts on them as it does in the reference."""

    HEAD_PREFIXES = ("force_block.", "energy_block.", "norm.")
    radial = RadialMLPLive
    _ENERGY_DEAD = ("energy_block.so3_linear_1.", "energy_block.grid_mlp.")

    def __init__(self, model, device="cuda:0", normalizers: Optional[dict] = None, energy_coefficient: float = 1,
                 force_coefficient: float = 30, train_on_free_atoms: bool = True) -> None:
        from .equiformer_v2_oc20 import EquiformerV2_OC20

        if not isinstance(model, EquiformerV2_OC20):
            raise NotImplementedError(f"EqV2S2EFTrainStep trains equiformer_v2_oc20.EquiformerV2_OC20, got {type(model).__name__}")
        if getattr(model, "force_mode", "direct") == "energy_gradient":
            raise NotImplementedError(
                "training with force_mode='energy_gradient' needs a second-order backward, which is not offered: "
                "train with force_mode='direct'")
        self._setup(model, device)
        self.energy_coefficient, self.force_coefficient = float(energy_coefficient), float(force_coefficient)
        self.train_on_free_atoms = bool(train_on_free_atoms)
        self.norm = {}
        for key in ("energy", "forces"):
            nz = (normalizers or {}).get(key)
            if nz is None or nz is False:
                self.norm[key] = (0.0, 1.0)
            elif isinstance(nz, dict):
                self.norm[key] = (float(nz.get("mean", 0.0)), float(nz.get("stdev", nz.get("std", 1.0))))
            else:
                self.norm[key] = (float(nz.mean), float(nz.std))
        self.metrics = None

    def _final_from_start(self, name: str) -> bool:
        return name.startswith(self._ENERGY_DEAD) or super()._final_from_start(name)

    def _energy(self, P, x, g: EqGraph, prep):
        """Per-system energies [B] from the final-normed embedding (the formula ``adf_eqv2_set_energy_head`` documents): per
        atom so3_linear_2.weight[0, 0] . SiLU(scalar_mlp.0(x[:, 0, :])) + so3_linear_2.bias, summed per system as a product
        with the one-hot membership (its backward needs no float atomic), divided by avg_num_nodes, plus the frozen
        energy_lin_ref[Z] with use_energy_lin_ref."""
        return self._energy_of(P, x, g.Z, prep.batch.long(), prep.num_systems)

    def _energy_of(self, P, x, Z, sysidx, B: int):
        """``_energy`` on the rows ``x`` [n, S, C] of the atoms ``Z`` [n] that belong to the systems ``sysidx`` [n] of ``B``."""
        m = self.model
        N = int(x.shape[0])
        hid = torch.nn.functional.silu(x[:, 0, :] @ P["energy_block.scalar_mlp.0.weight"].t() + P["energy_block.scalar_mlp.0.bias"])
        e_atom = hid @ P["energy_block.so3_linear_2.weight"][0, 0] + P["energy_block.so3_linear_2.bias"]
        onehot = torch.zeros(B, N, device=self.dev)
        onehot[sysidx, torch.arange(N, device=self.dev)] = 1.0
        energy = (onehot @ e_atom) / float(m.avg_num_nodes)
        if m.use_energy_lin_ref:
            energy = energy + onehot @ m.energy_lin_ref.detach().to(self.dev, torch.float32)[Z.long()]
        return energy

    def forward(self, batch, masks=None):
        """The training forward -> (energy [B], forces [N, 3] | None, graph, prep)."""
        x, ops, g, prep, P = self._trunk(batch, masks)
        energy = self._energy(P, x, g, prep)
        forces = self._force_head(ops, g, P, "force_block.", x) if self.model.regress_forces else None
        return energy, forces, g, prep

    def loss_and_grad(self, batch, grads_ready=None, counts: Optional[torch.Tensor] = None, masks=None) -> torch.Tensor:
        """``PaiNNS2EFTrainStep.loss_and_grad``'s contract: ``batch`` carries pos, atomic_numbers, batch, natoms, cell and the
        targets energy [B], forces [N,3], fixed [N]; accumulates into ``param.grad`` (call ``zero_grad`` first) and returns
        the device tensor (loss, energy term, force term); ``metrics``: (energy MAE, force MAE per component over the free
        atoms) in target units.  ``counts``: device int64 ``[B_glob, M_glob, W]`` of a multi-rank step.  ``masks``: replaces
        the dropout / drop-path draws.  ``grads_ready(names)``: ``force_block.``, ``energy_block.`` and ``norm.`` first, then
        the blocks from the last to the first, then the embeddings."""
        m, lib = self.model, self.lib
        self._require_zeroed()
        forces_on = bool(m.regress_forces)
        for key in ("energy",) + (("forces",) if forces_on else ()):
            if getattr(batch, key, None) is None:
                raise ValueError(f"batch.{key} is required (the S2EF target)")
        if self.train_on_free_atoms and forces_on and getattr(batch, "fixed", None) is None:
            raise ValueError("batch.fixed is required with train_on_free_atoms")
        if counts is not None and (counts.dtype != torch.int64 or counts.numel() != 3 or not counts.is_cuda):
            raise ValueError("counts: a device int64 tensor [B_glob, M_glob, W]")
        try:
            with torch.enable_grad():
                energy, forces, g, prep = self.forward(batch, masks)
        except torch.OutOfMemoryError as e:   # as the rest of the library: an allocation failure is a RuntimeError
            raise RuntimeError(f"HIP out of memory: {e}") from e
        N, B = g.N, prep.num_systems
        e_pred = energy.detach().contiguous()
        f_pred = forces.detach() if forces_on else None
        e_tgt = batch.energy.to(self.dev, torch.float32).reshape(-1).contiguous()
        f_tgt = batch.forces.to(self.dev, torch.float32).reshape(N, 3).contiguous() if forces_on else None
        if e_tgt.numel() != B:
            raise ValueError(f"batch.energy has {e_tgt.numel()} entries for {B} systems")
        loss, metrics = torch.empty(3, device=self.dev), torch.empty(2, device=self.dev)
        dE = torch.empty(B, device=self.dev)
        dF = torch.empty(N, 3, device=self.dev) if forces_on else None
        scratch = torch.empty(int(lib.adf_op_s2ef_loss_scratch(B)), device=self.dev)
        (mean_e, std_e), (mean_f, std_f) = self.norm["energy"], self.norm["forces"]
        with torch.cuda.device(self.dev):
            _lib.check(lib.adf_op_s2ef_loss(
                e_pred.data_ptr(), f_pred.data_ptr() if forces_on else None, e_tgt.data_ptr(),
                f_tgt.data_ptr() if forces_on else None, prep.fixed.data_ptr() if prep.fixed is not None else None,
                prep.atom_offset.data_ptr(), B, 1 if self.train_on_free_atoms else 0, C.c_float(mean_e), C.c_float(std_e),
                C.c_float(mean_f), C.c_float(std_f), C.c_float(self.energy_coefficient), C.c_float(self.force_coefficient),
                counts.data_ptr() if counts is not None else None, loss.data_ptr(), dE.data_ptr(),
                dF.data_ptr() if forces_on else None, metrics.data_ptr(), scratch.data_ptr(),
                C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)))
        self._backward([energy, forces] if forces_on else [energy], [dE, dF] if forces_on else [dE], grads_ready)
        self.metrics = metrics
        self.last_outputs = (e_pred, f_pred)
        return loss


class EqV2EnergyGradient(_EqV2StepBase):
    """Energy and forces = -dE/dpos of that energy for a mirror ``equiformer_v2_oc20.EquiformerV2_OC20`` on a ROCm device
    (DESIGN.md 6i): what ``torch.autograd.grad(energy.sum(), pos)`` gives on the reference model with the edge set held fixed.

    The graph is ``EqV2S2EFTrainStep.forward``'s in ``eval()`` - exact f32, no dropout, trunk, final norm, energy head; the
    force block is neither needed nor evaluated - so the energy reported is bit for bit that forward's, and within 1.3e-6 of
    max|E| of the inference forward's (f16x3 products, README).  No parameter asks for a gradient: the operators' backwards
    take their data paths alone (``needs_input_grad``), and RotateIn, RotateOut and RadialMLPLive add what they owe to the
    Wigner rows and to the distances into ``EqGraph.dwig`` / ``EqGraph.ddist``.  Two launches then turn (dwig, ddist, vec) into
    dE/dvec and into forces (``EqOps.geometry_to_forces``).  ``energy_lin_ref[Z]`` does not depend on the positions.

    The node side (torch) runs system by system: the dense products torch picks depend on the number of rows, so only then
    does a system get the same bits alone and among batch mates (the edge side's kernels treat every edge and every atom on
    its own).  Each system's rows are what the training forward computes for that system alone."""

    radial = RadialMLPLive
    stochastic = False
    fold_products = True

    def __init__(self, model, device="cuda:0") -> None:
        from .equiformer_v2_oc20 import EquiformerV2_OC20

        if not isinstance(model, EquiformerV2_OC20):
            raise NotImplementedError(f"EqV2EnergyGradient differentiates equiformer_v2_oc20.EquiformerV2_OC20, got "
                                      f"{type(model).__name__}")
        self._setup(model, device)

    _energy_of = EqV2S2EFTrainStep._energy_of

    def _rows(self, fn, x):
        # one system goes through split and cat too: the order in which autograd adds the gradients of a tensor with
        # several uses depends on the graph's shape, and a system alone must build the graph it builds among batch mates
        return torch.cat([fn(part) for part in torch.split(x, self._sizes, 0)], 0)

    def _energy(self, P, x, g: EqGraph, prep):
        parts = zip(torch.split(x, self._sizes, 0), torch.split(g.Z, self._sizes, 0))
        return torch.cat([self._energy_of(P, xb, zb, torch.zeros(xb.shape[0], dtype=torch.long, device=self.dev), 1)
                          for xb, zb in parts], 0)

    def _params(self) -> dict:
        return {k: v.detach() for k, v in self.model.named_parameters()}

    def _graph(self, eng, batch, prep) -> EqGraph:
        g = EqGraph(eng, batch, prep)
        self._sizes = [int(n) for n in batch.natoms.tolist()]     # atoms per system: the node side's row blocks
        DR = int(g.wig.shape[1])
        g.dwig = torch.zeros(g.E, DR, dtype=torch.float32, device=self.dev)
        g.ddist = torch.zeros(g.E, dtype=torch.float32, device=self.dev)
        g.geo = torch.zeros((), dtype=torch.float32, device=self.dev, requires_grad=True)
        return g

    def __call__(self, batch):
        """-> (energy [B], forces [N, 3]); an allocation failure is a ``RuntimeError`` (``ml_relax`` then halves the batch)."""
        try:
            with torch.enable_grad():
                x, ops, g, prep, P = self._trunk(batch)
                energy = self._energy(P, x, g, prep)
                if energy.requires_grad:   # (a graph without edges has no path to the geometry)
                    torch.autograd.backward([energy], [torch.ones_like(energy)])
            with torch.no_grad(), torch.cuda.device(self.dev):
                forces = ops.geometry_to_forces(g)
        except torch.OutOfMemoryError as e:
            raise RuntimeError(f"HIP out of memory: {e}") from e
        return energy.detach(), forces
