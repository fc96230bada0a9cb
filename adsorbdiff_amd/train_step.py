"""Score-matching training step of the PaiNN denoiser on the device (BASELINE config 5).

Replaces, for this model, what the reference's trainer does per step
(adsorbdiff/trainers/sde_denoising_trainer.py:370-537, 675-728; base_trainer.py:787-820):

    tr_so3_schedule (noising)  ->  model forward  ->  _compute_loss  ->  loss.backward()
    ->  clip_grad_norm_  ->  AdamW.step  ->  EMA.update           (+ DDP gradient all-reduce)

Every arithmetic operation of forward, loss, backward and optimizer runs in hand-written HIP kernels behind the C ABI
(csrc/train.hip, csrc/gemm.hip, csrc/graph.hip); this module only sequences the calls and owns the buffers (PyTorch as
allocator / stream / collective plumbing).  There is no autograd graph: `PaiNNTrainStep.loss_and_grad` writes the
gradients straight into ``param.grad`` of the mirror module, so ``torch.nn.parallel``-style code, checkpoints and the
reference's parameter naming keep working.

Status (round 4): products on the f16-rate matrix cores (f16x3 forward / data gradients, three-term bf16 split for the weight
gradients), message forward AND backward through fused kernels that regenerate the radial projection (nothing of size
[E, 3H] is kept from the forward), elementwise kernels unfused.  Pinned against the reference's own autograd
(tests/golden/train_small.npz, train_full.npz: loss + gradients, oracle/make_golden.py sections 6 and 10).
"""
from __future__ import annotations

import copy
import os

import ctypes as C
import math
from typing import Dict, List, Optional

import numpy as np
import torch

from . import lib as _lib
from .so3_tables import Igso3Tables


class _Ops:
    """Thin typed wrappers over the adf_op_* entry points (device pointers in, status out)."""

    def __init__(self, device) -> None:
        self.lib = _lib.load()
        self.dev = torch.device(device)
        self._scratch = torch.empty(0, device=self.dev)

    def s(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def scratch(self, n: int) -> torch.Tensor:
        if self._scratch.numel() < n:
            self._scratch = torch.empty(int(n * 1.25) + 1024, device=self.dev)
        return self._scratch

    def new(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    def linear(self, A, W, b, M, N, K, lda=None, out=None, ldc=None):
        if out is None:
            out = self.new(M, N)
        _lib.check(self.lib.adf_op_linear_fwd(A.data_ptr(), lda or K, W.data_ptr(), b.data_ptr() if b is not None else None,
                                              out.data_ptr(), ldc or N, M, N, K, self.s()))
        return out

    def linear_bwd(self, A, W, dC, M, N, K, dW, db, want_dA=True, dA=None, lda=None, ldc=None, ldda=None, acc_dA=False):
        if want_dA and dA is None:
            dA = self.new(M, K)
        sc = self.scratch(int(self.lib.adf_op_linear_bwd_scratch(M, N, K)))
        _lib.check(self.lib.adf_op_linear_bwd(
            A.data_ptr() if A is not None else None, lda or K, W.data_ptr(), dC.data_ptr(), ldc or N,
            dA.data_ptr() if want_dA else None, ldda or K, 1 if acc_dA else 0,
            dW.data_ptr() if dW is not None else None, db.data_ptr() if db is not None else None, 1, M, N, K,
            sc.data_ptr(), self.s()))
        return dA


class _StepContext:
    """What one loss_and_grad call shares between the trunk, the heads and the loss."""

    __slots__ = ("P", "G", "eng", "h", "prep", "E", "N", "B", "scales", "fused_bwd")


class _PaiNNStepBase:
    """The part of a training step both PaiNN mirrors share: graph, embedding, radial basis and the message / update layers
    forward with saved activations, the gated output head forward and backward, and the layers / rbf weight gradient /
    embedding backward.  A subclass adds its heads and its objective."""

    # parameters the objective never reads: the reference's autograd leaves their .grad at None (DDP runs with
    # find_unused_parameters, base_trainer.py:442-447) and torch.optim.AdamW then skips them - no weight decay either
    UNUSED_PREFIXES: tuple = ()

    def __init__(self, model, device) -> None:
        self.model = model
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs a ROCm device (the HIP path has no CPU fallback)")
        # forward of the message block through the sampler's fused kernel (ADF_TRAIN_MSG=plain: the rbfh-reading kernel)
        self.fused_message_forward = os.environ.get("ADF_TRAIN_MSG", "fused") != "plain"
        # backward of the message block with rbfh regenerated inside the kernel (message_bwd.hip) instead of kept from the
        # forward: needs the fused forward (it builds the layer's rbf_proj images) and the f16x3 arithmetic;
        # ADF_TRAIN_MSG_BWD=plain: the rbfh-reading kernel
        self.fused_message_backward = self.fused_message_forward and os.environ.get("ADF_TRAIN_MSG_BWD", "fused") != "plain"
        self._bwd_perm = None
        # rbf_proj's weight gradient without d(rbfh) [E, 3H] in memory (csrc/rbf_wgrad.hip: the fused backward stores
        # nothing per edge and the weight-gradient kernel forms d(rbfh) again while it stages its product);
        # ADF_TRAIN_RBF_WGRAD=materialised: the round-4 path (d(rbfh) written by the backward, read by adf_op_linear_bwd)
        self.rbf_wgrad_fused = os.environ.get("ADF_TRAIN_RBF_WGRAD", "fused") != "materialised"
        # basis sizes the step's kernels take, checked here and not in the middle of a step: the fused message kernels
        # stage the basis in blocks of 8, and without them the projection rbfh = rbf W^T is a product over num_rbf, which
        # csrc/gemm.hip takes in blocks of 32 (the handle itself accepts any even num_rbf <= 128)
        R = int(model.num_rbf)
        if R % 32 != 0 and (R % 8 != 0 or not self.fused_message_backward):
            raise NotImplementedError(
                f"the training step needs num_rbf to be a multiple of 32 (a multiple of 8 with the fused message "
                f"backward), got {R}")
        self.ops = _Ops(self.dev)
        self.lib = self.ops.lib
        # the embedding gradient summed in a fixed order (csrc/optimizer.hip: adf_op_embed_bwd_ordered) instead of with
        # float atomics: with it every gradient of the step is bit-reproducible (setup_training(reproducible=True))
        self.ordered_embedding_backward = False

    # ------------------------------------------------------------------ helpers
    def _params(self) -> Dict[str, torch.nn.Parameter]:
        return dict(self.model.named_parameters())

    def zero_grad(self) -> None:
        for name, p in self.model.named_parameters():
            if not p.requires_grad:
                continue
            if self.UNUSED_PREFIXES and name.startswith(self.UNUSED_PREFIXES):
                p.grad = None
            elif p.grad is None:
                p.grad = torch.zeros_like(p)
            else:
                p.grad.zero_()

    def _begin(self, batch) -> _StepContext:
        """Graph of ``batch`` on the model's engine, the parameters and their gradient buffers."""
        c = _StepContext()
        c.P = self._params()
        c.eng = self.model.engine(self.dev, refresh=False)
        c.h = c.eng.handle
        c.prep = c.eng.prepare(batch)
        c.E = c.eng.build_graph(batch, c.prep)
        c.N, c.B = c.prep.num_atoms, c.prep.num_systems
        return c

    def _bind_gradients(self, c: _StepContext) -> None:
        m, lib = self.model, self.lib
        H = m.hidden_channels
        c.G = {k: p.grad for k, p in c.P.items()
               if p.requires_grad and not (self.UNUSED_PREFIXES and k.startswith(self.UNUSED_PREFIXES))}
        for k, g in c.G.items():
            if g is None:
                raise RuntimeError("call zero_grad() before loss_and_grad()")
        c.scales = m.scale_factors()
        c.fused_bwd = self.fused_message_backward and bool(lib.adf_op_message_bwd_fused_supported(c.h))
        if c.fused_bwd and self._bwd_perm is None:
            perm = (C.c_int32 * (3 * H))()
            _lib.check(lib.adf_op_message_bwd_perm(c.h, perm, 3 * H))
            self._bwd_perm = torch.tensor(list(perm), dtype=torch.long, device=self.dev)

    # ------------------------------------------------------------------ trunk forward
    def _trunk_forward(self, c: _StepContext):
        """Embedding, radial basis and the layers with saved activations -> (x, vec, saved, rbf)."""
        m, ops, lib = self.model, self.ops, self.lib
        P, h, prep, E, N = c.P, c.h, c.prep, c.E, c.N
        H, L, R = m.hidden_channels, m.num_layers, m.num_rbf
        scales, fused_bwd = c.scales, c.fused_bwd
        s = ops.s
        x = ops.new(N, H)
        _lib.check(lib.adf_op_embed_fwd(h, prep.atomic_numbers.data_ptr(), N, x.data_ptr(), s()))
        c.eng.check_flags()
        rbf = ops.new(E, R)
        _lib.check(lib.adf_op_rbf(h, rbf.data_ptr(), s()))
        vec = None
        saved: List[dict] = []
        for l in range(L):
            mp, up = f"message_layers.{l}.", f"update_layers.{l}."
            a = {"x": x, "vec": vec}
            a["y"], a["stats"] = ops.new(N, H), ops.new(N, 2)
            _lib.check(lib.adf_op_layernorm_fwd(x.data_ptr(), P[mp + "x_layernorm.weight"].data_ptr(),
                                                P[mp + "x_layernorm.bias"].data_ptr(), a["y"].data_ptr(),
                                                a["stats"].data_ptr(), N, H, s()))
            a["h0"] = ops.linear(a["y"], P[mp + "x_proj.0.weight"], P[mp + "x_proj.0.bias"], N, H, H)
            a["c"] = ops.new(N, H)
            _lib.check(lib.adf_op_ssilu_fwd(a["h0"].data_ptr(), a["c"].data_ptr(), N * H, s()))
            a["xh"] = ops.linear(a["c"], P[mp + "x_proj.2.weight"], P[mp + "x_proj.2.bias"], N, 3 * H, H)
            if not fused_bwd:  # kept for the rbfh-reading backward (6 KB per edge and layer)
                a["rbfh"] = ops.linear(rbf, P[mp + "rbf_proj.weight"], P[mp + "rbf_proj.bias"], E, 3 * H, R)
            a["x1"], a["vec1"] = ops.new(N, H), ops.new(N, 3, H)
            if self.fused_message_forward:
                # the sampler's fused kernel (no read of the 6 KB-per-edge rbfh)
                _lib.check(lib.adf_op_message_fwd_fused(h, l, a["xh"].data_ptr(), vec.data_ptr() if vec is not None else None,
                                                        x.data_ptr(), a["x1"].data_ptr(), a["vec1"].data_ptr(),
                                                        1 if vec is None else 0, s()))
            else:
                _lib.check(lib.adf_op_message_fwd(h, a["xh"].data_ptr(), vec.data_ptr() if vec is not None else None,
                                                  a["rbfh"].data_ptr(), x.data_ptr(), a["x1"].data_ptr(), a["vec1"].data_ptr(),
                                                  1 if vec is None else 0, s()))
            a["vv"] = ops.linear(a["vec1"], P[up + "vec_proj.weight"], None, 3 * N, 2 * H, H)
            a["cat"], a["dot"] = ops.new(N, 2 * H), ops.new(N, H)
            _lib.check(lib.adf_op_copy_rows(a["x1"].data_ptr(), H, a["cat"].data_ptr(), 2 * H, N, H, 0, s()))
            _lib.check(lib.adf_op_vdot_fwd(a["vv"].data_ptr(), a["dot"].data_ptr(), a["cat"].data_ptr() + 4 * H, 2 * H, N, H,
                                           C.c_float(1e-8), s()))
            a["u0"] = ops.linear(a["cat"], P[up + "xvec_proj.0.weight"], P[up + "xvec_proj.0.bias"], N, H, 2 * H)
            a["ua"] = ops.new(N, H)
            _lib.check(lib.adf_op_ssilu_fwd(a["u0"].data_ptr(), a["ua"].data_ptr(), N * H, s()))
            a["a"] = ops.linear(a["ua"], P[up + "xvec_proj.2.weight"], P[up + "xvec_proj.2.bias"], N, 3 * H, H)
            x2, vec2 = ops.new(N, H), ops.new(N, 3, H)
            _lib.check(lib.adf_op_update_out_fwd(a["x1"].data_ptr(), a["vec1"].data_ptr(), a["a"].data_ptr(),
                                                 a["dot"].data_ptr(), a["vv"].data_ptr(), C.c_float(scales[l]),
                                                 x2.data_ptr(), vec2.data_ptr(), N, H, s()))
            saved.append(a)
            x, vec = x2, vec2
        return x, vec, saved, rbf

    # ------------------------------------------------------------------ gated output head
    def _head_forward(self, c: _StepContext, hname: str, x, vec):
        """One ``PaiNNOutput`` head (two gated equivariant blocks) -> (saved blocks, output [N, 3])."""
        ops, lib = self.ops, self.lib
        P, N = c.P, c.N
        H = self.model.hidden_channels
        s = ops.s
        hs = {}
        xin, vin, Cin = x, vec, H
        for blk, Cout in ((0, H // 2), (1, 1)):
            q = f"{hname}.output_network.{blk}."
            b = {"xin": xin, "vin": vin, "Cin": Cin, "Cout": Cout}
            b["t1"] = ops.linear(vin, P[q + "vec1_proj.weight"], None, 3 * N, Cin, Cin)
            b["cat"] = ops.new(N, 2 * Cin)
            _lib.check(lib.adf_op_copy_rows(xin.data_ptr(), Cin, b["cat"].data_ptr(), 2 * Cin, N, Cin, 0, s()))
            _lib.check(lib.adf_op_vnorm_fwd(b["t1"].data_ptr(), b["cat"].data_ptr() + 4 * Cin, 2 * Cin, N, Cin, s()))
            b["t2"] = ops.linear(vin, P[q + "vec2_proj.weight"], None, 3 * N, Cout, Cin)
            b["g0"] = ops.linear(b["cat"], P[q + "update_net.0.weight"], P[q + "update_net.0.bias"], N, Cin, 2 * Cin)
            b["ga"] = ops.new(N, Cin)
            _lib.check(lib.adf_op_ssilu_fwd(b["g0"].data_ptr(), b["ga"].data_ptr(), N * Cin, s()))
            b["o"] = ops.linear(b["ga"], P[q + "update_net.2.weight"], P[q + "update_net.2.bias"], N, 2 * Cout, Cin)
            b["xs"], b["vout"] = ops.new(N, Cout), ops.new(N, 3, Cout)
            _lib.check(lib.adf_op_gate_fwd(b["o"].data_ptr(), b["t2"].data_ptr(), b["xs"].data_ptr(), Cout,
                                           b["vout"].data_ptr(), N, Cout, s()))
            hs[blk] = b
            xin, vin, Cin = b["xs"], b["vout"], Cout
        return hs, vin.reshape(N, 3)

    def _head_backward(self, c: _StepContext, hname: str, hs, dout, dx, dvec) -> None:
        """Backward of one head from ``dout`` [N, 3]: its parameters' gradients, and its inputs' accumulated into dx / dvec."""
        ops, lib = self.ops, self.lib
        P, G, N = c.P, c.G, c.N
        H = self.model.hidden_channels
        s = ops.s
        dxs, dv = None, dout.reshape(N, 3, 1)
        for blk in (1, 0):
            b = hs[blk]
            q = f"{hname}.output_network.{blk}."
            Cin, Cout = b["Cin"], b["Cout"]
            d_o, dt2 = ops.new(N, 2 * Cout), ops.new(N, 3, Cout)
            _lib.check(lib.adf_op_gate_bwd(b["o"].data_ptr(), b["t2"].data_ptr(), dxs.data_ptr() if dxs is not None else None,
                                           Cout, dv.data_ptr(), d_o.data_ptr(), dt2.data_ptr(), N, Cout, s()))
            dga = ops.linear_bwd(b["ga"], P[q + "update_net.2.weight"], d_o, N, 2 * Cout, Cin,
                                 G[q + "update_net.2.weight"], G[q + "update_net.2.bias"])
            dg0 = ops.new(N, Cin)
            _lib.check(lib.adf_op_ssilu_bwd(b["g0"].data_ptr(), dga.data_ptr(), dg0.data_ptr(), N * Cin, s()))
            dcat = ops.linear_bwd(b["cat"], P[q + "update_net.0.weight"], dg0, N, Cin, 2 * Cin,
                                  G[q + "update_net.0.weight"], G[q + "update_net.0.bias"])
            dt1 = ops.new(N, 3, Cin)
            _lib.check(lib.adf_op_vnorm_bwd(b["t1"].data_ptr(), b["cat"].data_ptr() + 4 * Cin, 2 * Cin,
                                            dcat.data_ptr() + 4 * Cin, 2 * Cin, dt1.data_ptr(), N, Cin, s()))
            # gradient of this block's inputs: x from the left half of dcat, v from the two projections
            if blk == 1:
                dxs_in, dv_in = ops.new(N, Cin), ops.new(N, 3, Cin)
                tgt_x, ldx, tgt_v, acc = dxs_in, Cin, dv_in, False
            else:
                tgt_x, ldx, tgt_v, acc = dx, H, dvec, True
            _lib.check(lib.adf_op_copy_rows(dcat.data_ptr(), 2 * Cin, tgt_x.data_ptr(), ldx, N, Cin, 1 if acc else 0, s()))
            ops.linear_bwd(b["vin"], P[q + "vec1_proj.weight"], dt1, 3 * N, Cin, Cin, G[q + "vec1_proj.weight"], None,
                           dA=tgt_v, acc_dA=acc)
            ops.linear_bwd(b["vin"], P[q + "vec2_proj.weight"], dt2, 3 * N, Cout, Cin, G[q + "vec2_proj.weight"], None,
                           dA=tgt_v, acc_dA=True)
            if blk == 1:
                dxs, dv = dxs_in, dv_in

    # ------------------------------------------------------------------ trunk backward
    def _trunk_backward(self, c: _StepContext, dx, dvec, saved, rbf, grads_ready=None) -> None:
        """Layers from the last to the first, the rbf weight gradient and the embedding, from d(x), d(vec) of the last layer."""
        m, ops, lib = self.model, self.ops, self.lib
        P, G, h, prep, E, N = c.P, c.G, c.h, c.prep, c.E, c.N
        H, L, R = m.hidden_channels, m.num_layers, m.num_rbf
        scales, fused_bwd = c.scales, c.fused_bwd
        s = ops.s
        edge_owner = rbf_image = None
        for l in range(L - 1, -1, -1):
            a = saved[l]
            mp, up = f"message_layers.{l}.", f"update_layers.{l}."
            # update block
            da, ddot, dv1 = ops.new(N, 3 * H), ops.new(N, H), ops.new(N, 3, H)
            dx1, dvec1 = ops.new(N, H), ops.new(N, 3, H)
            _lib.check(lib.adf_op_update_out_bwd(a["a"].data_ptr(), a["dot"].data_ptr(), a["vv"].data_ptr(),
                                                 C.c_float(scales[l]), dx.data_ptr(), dvec.data_ptr(), da.data_ptr(),
                                                 ddot.data_ptr(), dv1.data_ptr(), dx1.data_ptr(), dvec1.data_ptr(), N, H, s()))
            dua = ops.linear_bwd(a["ua"], P[up + "xvec_proj.2.weight"], da, N, 3 * H, H, G[up + "xvec_proj.2.weight"],
                                 G[up + "xvec_proj.2.bias"])
            du0 = ops.new(N, H)
            _lib.check(lib.adf_op_ssilu_bwd(a["u0"].data_ptr(), dua.data_ptr(), du0.data_ptr(), N * H, s()))
            dcat = ops.linear_bwd(a["cat"], P[up + "xvec_proj.0.weight"], du0, N, H, 2 * H, G[up + "xvec_proj.0.weight"],
                                  G[up + "xvec_proj.0.bias"])
            _lib.check(lib.adf_op_copy_rows(dcat.data_ptr(), 2 * H, dx1.data_ptr(), H, N, H, 1, s()))
            dvv = ops.new(N, 3, 2 * H)
            _lib.check(lib.adf_op_vdot_bwd(a["vv"].data_ptr(), a["cat"].data_ptr() + 4 * H, 2 * H, ddot.data_ptr(),
                                           dcat.data_ptr() + 4 * H, 2 * H, dv1.data_ptr(), dvv.data_ptr(), N, H, s()))
            ops.linear_bwd(a["vec1"], P[up + "vec_proj.weight"], dvv, 3 * N, 2 * H, H, G[up + "vec_proj.weight"], None,
                           dA=dvec1, acc_dA=True)
            # message block
            first = a["vec"] is None
            dxh = ops.new(N, 3 * H)
            dvec_in = None if first else ops.new(N, 3, H)
            dx_in = ops.new(N, H)
            if fused_bwd and self.rbf_wgrad_fused:
                # nothing per edge leaves the backward; the bias gradient arrives as per-atom column sums
                db_rows = ops.new(N, 3 * H)
                _lib.check(lib.adf_op_message_bwd_fused(h, l, a["xh"].data_ptr(), a["vec"].data_ptr() if not first else None,
                                                        dx1.data_ptr(), dvec1.data_ptr(), dxh.data_ptr(), None, E,
                                                        dvec_in.data_ptr() if not first else None, dx_in.data_ptr(),
                                                        1 if first else 0, db_rows.data_ptr(), s()))
                if edge_owner is None:   # once per step: the graph and the radial basis are the same for every layer
                    edge_owner = torch.empty(E, dtype=torch.int32, device=self.dev)
                    _lib.check(lib.adf_op_edge_owner(h, edge_owner.data_ptr(), E, s()))
                    rbf_image = torch.empty(int(lib.adf_op_rbf_image_bytes(E)), dtype=torch.uint8, device=self.dev)
                    _lib.check(lib.adf_op_rbf_image(h, rbf.data_ptr(), E, rbf_image.data_ptr(), s()))
                sc = ops.scratch(int(lib.adf_op_rbf_wgrad_fused_scratch(h)))
                _lib.check(lib.adf_op_rbf_wgrad_fused(h, a["xh"].data_ptr(), a["vec"].data_ptr() if not first else None,
                                                      rbf_image.data_ptr(), edge_owner.data_ptr(), E,
                                                      G[mp + "rbf_proj.weight"].data_ptr(), sc.data_ptr(), 1 if first else 0, s()))
                ops.linear_bwd(None, P[mp + "rbf_proj.weight"], db_rows, N, 3 * H, R, None, G[mp + "rbf_proj.bias"],
                               want_dA=False)
            elif fused_bwd:
                drbfh = ops.new(E + 1, 3 * H)  # (+1: the fused kernel's spare row)
                # drbfh comes back with its columns in the kernel's own order: the weight gradient is formed on that order
                # and its rows are permuted back (3H x R, tiny)
                _lib.check(lib.adf_op_message_bwd_fused(h, l, a["xh"].data_ptr(), a["vec"].data_ptr() if not first else None,
                                                        dx1.data_ptr(), dvec1.data_ptr(), dxh.data_ptr(), drbfh.data_ptr(), E,
                                                        dvec_in.data_ptr() if not first else None, dx_in.data_ptr(),
                                                        1 if first else 0, None, s()))
                dwp = torch.zeros(3 * H, R, dtype=torch.float32, device=self.dev)
                dbp = torch.zeros(3 * H, dtype=torch.float32, device=self.dev)
                ops.linear_bwd(rbf, P[mp + "rbf_proj.weight"], drbfh, E, 3 * H, R, dwp, dbp, want_dA=False)
                G[mp + "rbf_proj.weight"].index_add_(0, self._bwd_perm, dwp)
                G[mp + "rbf_proj.bias"].index_add_(0, self._bwd_perm, dbp)
            else:
                drbfh = ops.new(E, 3 * H)
                _lib.check(lib.adf_op_message_bwd(h, a["xh"].data_ptr(), a["vec"].data_ptr() if not first else None,
                                                  a["rbfh"].data_ptr(), dx1.data_ptr(), dvec1.data_ptr(), dxh.data_ptr(),
                                                  drbfh.data_ptr(), dvec_in.data_ptr() if not first else None,
                                                  dx_in.data_ptr(), 1 if first else 0, s()))
                ops.linear_bwd(rbf, P[mp + "rbf_proj.weight"], drbfh, E, 3 * H, R, G[mp + "rbf_proj.weight"],
                               G[mp + "rbf_proj.bias"], want_dA=False)
            dc = ops.linear_bwd(a["c"], P[mp + "x_proj.2.weight"], dxh, N, 3 * H, H, G[mp + "x_proj.2.weight"],
                                G[mp + "x_proj.2.bias"])
            dh0 = ops.new(N, H)
            _lib.check(lib.adf_op_ssilu_bwd(a["h0"].data_ptr(), dc.data_ptr(), dh0.data_ptr(), N * H, s()))
            dy = ops.linear_bwd(a["y"], P[mp + "x_proj.0.weight"], dh0, N, H, H, G[mp + "x_proj.0.weight"],
                                G[mp + "x_proj.0.bias"])
            dlw, dlb = ops.new(H), ops.new(H)
            _lib.check(lib.adf_op_layernorm_bwd(a["x"].data_ptr(), P[mp + "x_layernorm.weight"].data_ptr(),
                                                a["stats"].data_ptr(), dy.data_ptr(), dx_in.data_ptr(), dlw.data_ptr(),
                                                dlb.data_ptr(), N, H, ops.scratch(512 * 2 * H + 16).data_ptr(), s()))
            _lib.check(lib.adf_op_copy_rows(dlw.data_ptr(), H, G[mp + "x_layernorm.weight"].data_ptr(), H, 1, H, 1, s()))
            _lib.check(lib.adf_op_copy_rows(dlb.data_ptr(), H, G[mp + "x_layernorm.bias"].data_ptr(), H, 1, H, 1, s()))
            dx, dvec = dx_in, dvec_in
            if grads_ready is not None:
                grads_ready([mp, up])
        demb = G["atom_emb.embeddings.weight"]
        if self.ordered_embedding_backward:
            rows = int(demb.shape[0])
            sc = ops.scratch(int(lib.adf_op_embed_bwd_ordered_scratch(N, H, rows)))
            _lib.check(lib.adf_op_embed_bwd_ordered(dx.data_ptr(), prep.atomic_numbers.data_ptr(), demb.data_ptr(), N, H, rows,
                                                    sc.data_ptr(), s()))
        else:
            _lib.check(lib.adf_op_embed_bwd(dx.data_ptr(), prep.atomic_numbers.data_ptr(), demb.data_ptr(), N, H, s()))
        if grads_ready is not None:
            grads_ready(["atom_emb."])


class PaiNNTrainStep(_PaiNNStepBase):
    """loss + gradients of the score-matching objective for a mirror ``PaiNN`` module on a ROCm device."""

    # the score path never reads the energy head
    UNUSED_PREFIXES = ("out_energy.",)

    def __init__(self, model, device="cuda:0", igso3: Optional[Igso3Tables] = None) -> None:
        super().__init__(model, device)
        # one head (so3_denoising=False): the translation term alone; the rotation tables are neither needed nor loaded
        self.two_heads = bool(model.so3_denoising)
        self.igso3 = (igso3 or Igso3Tables.shared()) if self.two_heads else igso3

    # ------------------------------------------------------------------ the step
    def loss_and_grad(self, batch, targets: dict, grads_ready=None) -> torch.Tensor:
        """``batch``: noised batch on the device (pos, atomic_numbers, tags, batch, natoms, cell); ``targets``: tr_sigma
        [B,1], rot_sigma [B,1], tr_score [B,3], rot_score [B,3] (what tr_so3_schedule attaches to the batch) and, optionally,
        rot_norm [B] (the expected score norm of every rot_sigma, as the device noising returns it; absent: looked up on
        the device).  A one-head model (``so3_denoising=False``) takes tr_sigma and tr_score only (what
        ads_COM_gaussian_schedule attaches).  Accumulates into ``param.grad`` (call zero_grad first, like
        optimizer.zero_grad) and returns the device tensor (loss, translation term, rotation term; 0 for one head).
        ``grads_ready(names)`` (optional) is called as soon as the gradients of a group of parameters are final: the
        head(s), then each layer from the last to the first, then the embedding."""
        m, ops, lib = self.model, self.ops, self.lib
        H = m.hidden_channels
        c = self._begin(batch)
        prep, N, B = c.prep, c.N, c.B
        if prep.tags is None:
            raise ValueError("batch.tags is required (tag 2 marks the adsorbate)")
        s = ops.s
        self._bind_gradients(c)
        hnames = ("out_forces", "out_forces2") if self.two_heads else ("out_forces",)

        # ---------------- forward with saved activations
        x, vec, saved, rbf = self._trunk_forward(c)
        heads = []
        outs = []
        for hname in hnames:
            hs, out = self._head_forward(c, hname, x, vec)
            heads.append(hs)
            outs.append(out)

        # ---------------- loss and its gradient with respect to the heads' outputs
        keys = ("tr_sigma", "rot_sigma", "tr_score", "rot_score") if self.two_heads else ("tr_sigma", "tr_score")
        t = {k: targets[k].to(self.dev, torch.float32).contiguous() for k in keys}
        loss = ops.new(3)
        douts = [ops.new(N, 3) for _ in hnames]
        if self.two_heads:
            rot_norm = targets.get("rot_norm")
            if rot_norm is None:
                from .noising import device_score_norm

                rot_norm = device_score_norm(t["rot_sigma"], self.igso3, self.dev)
            rot_norm = rot_norm.to(self.dev, torch.float32).reshape(-1).contiguous()
            _lib.check(lib.adf_op_score_loss(outs[0].data_ptr(), outs[1].data_ptr(), prep.tags.data_ptr(),
                                             prep.atom_offset.data_ptr(), t["tr_sigma"].data_ptr(), t["rot_sigma"].data_ptr(),
                                             t["tr_score"].data_ptr(), t["rot_score"].data_ptr(), rot_norm.data_ptr(),
                                             loss.data_ptr(), douts[0].data_ptr(), douts[1].data_ptr(), B,
                                             ops.scratch(2 * B + 16).data_ptr(), s()))
        else:
            _lib.check(lib.adf_op_score_loss_tr(outs[0].data_ptr(), prep.tags.data_ptr(), prep.atom_offset.data_ptr(),
                                                t["tr_sigma"].data_ptr(), t["tr_score"].data_ptr(), loss.data_ptr(),
                                                douts[0].data_ptr(), B, ops.scratch(B + 16).data_ptr(), s()))

        # ---------------- backward: heads
        dx = torch.zeros(N, H, device=self.dev)
        dvec = torch.zeros(N, 3, H, device=self.dev)
        for hname, hs, dout in zip(hnames, heads, douts):
            self._head_backward(c, hname, hs, dout, dx, dvec)
        if grads_ready is not None:
            grads_ready([h + "." for h in hnames])
        # ---------------- backward: layers, last to first, then the embedding
        self._trunk_backward(c, dx, dvec, saved, rbf, grads_ready)
        self.last_outputs = tuple(outs)
        return loss


class PaiNNS2EFTrainStep(_PaiNNStepBase):
    """loss + gradients of the S2EF objective for a mirror ``adsorbdiff_amd.painn.PaiNN`` (the force field ``ml_relax``
    relaxes with) on a ROCm device: what ``OCPTrainer._compute_loss`` + ``loss.backward()`` do for it
    (trainers/ocp_trainer.py:308-356, modules/loss.py:48-102) with energy loss "mae" and force loss "l2mae"; the model's
    outputs are normalised predictions, the targets ``batch.energy [B]``, ``batch.forces [N,3]`` are normalised with
    ``normalizers`` (absent: mean 0, std 1).  Defaults: utils/utils.py:1227,1257 and base_trainer.py:382-390.  Shares the
    trunk with ``PaiNNTrainStep``; the heads are one gated force head (none with ``regress_forces=False``: the loss is the
    energy term alone) and the energy head, whose backward is ``adf_op_energy_head_bwd`` + ``adf_op_linear_bwd``.  Every
    parameter of this model is used: none is left at ``grad = None``.  The engine supplies the 1e-6 distance floor."""

    def __init__(self, model, device="cuda:0", normalizers: Optional[dict] = None, energy_coefficient: float = 1,
                 force_coefficient: float = 30, train_on_free_atoms: bool = True) -> None:
        from .painn import PaiNN as S2EFPaiNN

        if not isinstance(model, S2EFPaiNN):
            raise NotImplementedError(
                f"PaiNNS2EFTrainStep trains adsorbdiff_amd.painn.PaiNN (energy + force heads), got {type(model).__name__}; "
                "the denoiser's step is PaiNNTrainStep")
        if model.force_mode == "energy_gradient":
            raise NotImplementedError(
                "training with force_mode='energy_gradient' needs a second-order backward, which this direct-force step "
                "does not have: pass force_objective='energy_gradient' to setup_training (PaiNNGradForceTrainStep), or "
                "train with force_mode='direct'")
        super().__init__(model, device)
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
        self.last_outputs = None

    def loss_and_grad(self, batch, grads_ready=None, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``batch``: pos, atomic_numbers, batch, natoms, cell and the targets energy [B], forces [N,3], fixed [N] on the
        device.  Accumulates into ``param.grad`` (call zero_grad first) and returns the device tensor (loss, energy term,
        force term); ``metrics`` then holds the device tensor (energy MAE, force MAE per component over the free atoms) in
        target units.  ``counts``: device int64 ``[B_glob, M_glob, W]`` of a multi-rank step (None: this batch's own
        counts, W = 1).  ``grads_ready(names)``: ``out_energy.`` together with ``out_forces.``, then each layer from the
        last to the first, then the embedding."""
        m, ops, lib = self.model, self.ops, self.lib
        H = m.hidden_channels
        H2 = H // 2
        c = self._begin(batch)
        prep, N, B, P = c.prep, c.N, c.B, c.P
        forces_on = bool(m.regress_forces)
        for key in ("energy",) + (("forces",) if forces_on else ()):
            if getattr(batch, key, None) is None:
                raise ValueError(f"batch.{key} is required (the S2EF target)")
        if self.train_on_free_atoms and forces_on and prep.fixed is None:
            raise ValueError("batch.fixed is required with train_on_free_atoms")
        if counts is not None and (counts.dtype != torch.int64 or counts.numel() != 3 or not counts.is_cuda):
            raise ValueError("counts: a device int64 tensor [B_glob, M_glob, W]")
        s = ops.s
        self._bind_gradients(c)
        G = c.G

        # ---------------- forward with saved activations
        x, vec, saved, rbf = self._trunk_forward(c)
        hs = f_pred = None
        if forces_on:
            hs, f_pred = self._head_forward(c, "out_forces", x, vec)
        he0 = ops.linear(x, P["out_energy.0.weight"], P["out_energy.0.bias"], N, H2, H)
        hea = ops.new(N, H2)
        _lib.check(lib.adf_op_ssilu_fwd(he0.data_ptr(), hea.data_ptr(), N * H2, s()))
        e_pred = ops.new(B)
        _lib.check(lib.adf_op_energy_sum(hea.data_ptr(), H2, P["out_energy.2.weight"].data_ptr(),
                                         P["out_energy.2.bias"].data_ptr(), prep.atom_offset.data_ptr(), e_pred.data_ptr(), B,
                                         s()))

        # ---------------- loss and its gradient with respect to the predictions
        e_tgt = batch.energy.to(self.dev, torch.float32).reshape(-1).contiguous()
        f_tgt = batch.forces.to(self.dev, torch.float32).reshape(N, 3).contiguous() if forces_on else None
        if e_tgt.numel() != B:
            raise ValueError(f"batch.energy has {e_tgt.numel()} entries for {B} systems")
        loss, metrics = ops.new(3), ops.new(2)
        dE = ops.new(B)
        dF = ops.new(N, 3) if forces_on else None
        (mean_e, std_e), (mean_f, std_f) = self.norm["energy"], self.norm["forces"]
        _lib.check(lib.adf_op_s2ef_loss(
            e_pred.data_ptr(), f_pred.data_ptr() if forces_on else None, e_tgt.data_ptr(),
            f_tgt.data_ptr() if forces_on else None, prep.fixed.data_ptr() if prep.fixed is not None else None,
            prep.atom_offset.data_ptr(), B, 1 if self.train_on_free_atoms else 0, C.c_float(mean_e), C.c_float(std_e),
            C.c_float(mean_f), C.c_float(std_f), C.c_float(self.energy_coefficient), C.c_float(self.force_coefficient),
            counts.data_ptr() if counts is not None else None, loss.data_ptr(), dE.data_ptr(),
            dF.data_ptr() if forces_on else None, metrics.data_ptr(),
            ops.scratch(int(lib.adf_op_s2ef_loss_scratch(B))).data_ptr(), s()))

        # ---------------- backward: the force head, then the energy head on top of it
        dx = torch.zeros(N, H, device=self.dev)
        dvec = torch.zeros(N, 3, H, device=self.dev)
        if forces_on:
            self._head_backward(c, "out_forces", hs, dF, dx, dvec)
        dhe0 = ops.new(N, H2)
        _lib.check(lib.adf_op_energy_head_bwd(
            he0.data_ptr(), P["out_energy.2.weight"].data_ptr(), dE.data_ptr(), prep.batch.data_ptr(), dhe0.data_ptr(),
            G["out_energy.2.weight"].data_ptr(), G["out_energy.2.bias"].data_ptr(), 1, N, H2,
            ops.scratch(int(lib.adf_op_energy_head_bwd_scratch(N, H2))).data_ptr(), s()))
        ops.linear_bwd(x, P["out_energy.0.weight"], dhe0, N, H2, H, G["out_energy.0.weight"], G["out_energy.0.bias"],
                       dA=dx, acc_dA=True)
        if grads_ready is not None:
            grads_ready(["out_energy.", "out_forces."])
        # ---------------- backward: layers, last to first, then the embedding
        self._trunk_backward(c, dx, dvec, saved, rbf, grads_ready)
        self.metrics = metrics
        self.last_outputs = (e_pred, f_pred)
        return loss


class PaiNNGradForceTrainStep(_PaiNNStepBase):
    """loss + gradients of the S2EF objective with the forces ``-d(sum_b E_b)/d(pos)`` of ``force_mode="energy_gradient"``
    in the loss: what the reference does with ``torch.autograd.grad(energy.sum(), pos, create_graph=True)`` followed by
    ``OCPTrainer._compute_loss`` and ``loss.backward()`` (models/painn/painn.py:417-429 applied to the energy, DESIGN.md 4e /
    6j).  Same contract as ``PaiNNS2EFTrainStep``; works without a force head, and the parameters of a force head are not part
    of the objective (``grad`` stays None, both optimizers skip them).

    The predicted forces are the gradient of the model's NORMALISED energy, so the force targets are normalised with mean 0
    and the ENERGY normaliser's stdev - the pair ``ForcesTrainer.validate`` / ``predict`` denormalise these forces with.  The
    forces normaliser is not used.

    Four phases.  (1) energy and forces by ``adf_painn_forward_energy_gradient`` as ``model(batch)`` calls it: the reported
    predictions are that call's bits.  (2) ``adf_op_s2ef_loss``: loss, metrics, w = dL/dE [B], v = dL/dF [N,3], constants of
    the backward.  (3) the dual forward: with D = d/d eps sum_b E_b(pos + eps v), the force term's parameter gradient is
    -grad_theta D; every activation carries its tangent, started from the edge tangents (``adf_op_edge_tangent``), primal and
    tangent rows stacked so that each linear layer is one product over twice the rows, the nonlinear operators in their dual
    forms (csrc/dual_ops.hip, csrc/message_dual.hip).  (4) one reverse pass through the joint graph, seeded with w on E and
    -1 on D.  The radial projection rbfh [2E, 3H] is formed again in the backward instead of kept per layer."""

    UNUSED_PREFIXES = ("out_forces.",)

    def __init__(self, model, device="cuda:0", normalizers: Optional[dict] = None, energy_coefficient: float = 1,
                 force_coefficient: float = 30, train_on_free_atoms: bool = True) -> None:
        from .painn import PaiNN as S2EFPaiNN

        if not isinstance(model, S2EFPaiNN):
            raise NotImplementedError(
                f"PaiNNGradForceTrainStep trains adsorbdiff_amd.painn.PaiNN, got {type(model).__name__}")
        if model.force_mode != "energy_gradient":
            raise ValueError(
                f"force_objective='energy_gradient' trains the forces of model.force_mode='energy_gradient', but "
                f"model.force_mode is {model.force_mode!r}: set both, so that validate / predict / ml_relax evaluate what was "
                "trained")
        super().__init__(model, device)
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
        # the objective's force normaliser (what ForcesTrainer.validate reads back for its loss): mean 0, the energy stdev
        self.norm["forces"] = (0.0, self.norm["energy"][1])
        self.metrics = None
        self.last_outputs = None

    # ------------------------------------------------------------------ stacked linear layers
    def _lin2(self, A2, W, b, M, N, K):
        """[A; A_dot] W^T over 2M rows; the bias goes to the M primal rows only."""
        out = self.ops.linear(A2, W, None, 2 * M, N, K)
        if b is not None:
            _lib.check(self.lib.adf_op_dual_bias(out.data_ptr(), N, b.data_ptr(), M, N, self.ops.s()))
        return out

    def _lin2_bwd(self, A2, W, dC2, M, N, K, dW, db, want_dA=True, dA=None, acc_dA=False):
        """dW += dC^T A + dC_dot^T A_dot in one product; db += the column sums of the primal rows of dC alone."""
        dA = self.ops.linear_bwd(A2, W, dC2, 2 * M, N, K, dW, None, want_dA=want_dA, dA=dA, acc_dA=acc_dA)
        if db is not None:
            self.ops.linear_bwd(None, W, dC2, M, N, K, None, db, want_dA=False)
        return dA

    # ------------------------------------------------------------------ the step
    def loss_and_grad(self, batch, grads_ready=None, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """As ``PaiNNS2EFTrainStep.loss_and_grad``: targets ``batch.energy [B]``, ``batch.forces [N,3]``, ``batch.fixed [N]``;
        returns the device tensor (loss, energy term, force term); ``metrics`` = (energy MAE, force MAE per component over
        the free atoms) in target units; ``last_outputs = (e_pred, f_pred)``, bit for bit what ``model(batch)`` returns.
        ``grads_ready(names)``: ``out_energy.`` together with ``out_forces.``, then each layer from the last to the first,
        then the embedding."""
        m, ops, lib = self.model, self.ops, self.lib
        H, L, R = m.hidden_channels, m.num_layers, m.num_rbf
        H2 = H // 2
        for key in ("energy", "forces"):
            if getattr(batch, key, None) is None:
                raise ValueError(f"batch.{key} is required (the S2EF target)")
        if counts is not None and (counts.dtype != torch.int64 or counts.numel() != 3 or not counts.is_cuda):
            raise ValueError("counts: a device int64 tensor [B_glob, M_glob, W]")
        # ---------------- phase 1: the predictions, as model(batch) forms them (engine with the current weights bound)
        e_pred, f_pred = m.engine(self.dev).forward_energy_gradient(batch)
        c = self._begin(batch)
        prep, N, B, P, E, h = c.prep, c.N, c.B, c.P, c.E, c.h
        if self.train_on_free_atoms and prep.fixed is None:
            raise ValueError("batch.fixed is required with train_on_free_atoms")
        s = ops.s
        self._bind_gradients(c)
        G, scales = c.G, c.scales

        # ---------------- phase 2: loss, w = dL/dE, v = dL/dF
        e_tgt = batch.energy.to(self.dev, torch.float32).reshape(-1).contiguous()
        f_tgt = batch.forces.to(self.dev, torch.float32).reshape(N, 3).contiguous()
        if e_tgt.numel() != B:
            raise ValueError(f"batch.energy has {e_tgt.numel()} entries for {B} systems")
        loss, metrics = ops.new(3), ops.new(2)
        dE, dF = ops.new(B), ops.new(N, 3)
        mean_e, std_e = self.norm["energy"]
        _lib.check(lib.adf_op_s2ef_loss(
            e_pred.data_ptr(), f_pred.data_ptr(), e_tgt.data_ptr(), f_tgt.data_ptr(),
            prep.fixed.data_ptr() if prep.fixed is not None else None, prep.atom_offset.data_ptr(), B,
            1 if self.train_on_free_atoms else 0, C.c_float(mean_e), C.c_float(std_e), C.c_float(0.0), C.c_float(std_e),
            C.c_float(self.energy_coefficient), C.c_float(self.force_coefficient),
            counts.data_ptr() if counts is not None else None, loss.data_ptr(), dE.data_ptr(), dF.data_ptr(),
            metrics.data_ptr(), ops.scratch(int(lib.adf_op_s2ef_loss_scratch(B))).data_ptr(), s()))

        # ---------------- phase 3: the dual forward along v, keeping what the backward reads
        e_tan = ops.new(max(E, 1), 4)
        _lib.check(lib.adf_op_edge_tangent(h, dF.data_ptr(), e_tan.data_ptr(), E, s()))
        rbf2 = ops.new(2 * E, R)
        _lib.check(lib.adf_op_rbf_dual(h, e_tan.data_ptr(), rbf2.data_ptr(), E, s()))
        x2 = torch.zeros(2, N, H, dtype=torch.float32, device=self.dev)   # the embedding does not depend on the positions
        _lib.check(lib.adf_op_embed_fwd(h, prep.atomic_numbers.data_ptr(), N, x2.data_ptr(), s()))
        c.eng.check_flags()
        vec2 = None
        saved: List[dict] = []

        def rbfh_of(l):
            mp = f"message_layers.{l}."
            return self._lin2(rbf2, P[mp + "rbf_proj.weight"], P[mp + "rbf_proj.bias"], E, 3 * H, R)

        for l in range(L):
            mp, up = f"message_layers.{l}.", f"update_layers.{l}."
            a = {"x": x2, "vec": vec2}
            a["y"], a["stats"] = ops.new(2, N, H), ops.new(N, 2)
            _lib.check(lib.adf_op_layernorm_dual_fwd(x2.data_ptr(), P[mp + "x_layernorm.weight"].data_ptr(),
                                                     P[mp + "x_layernorm.bias"].data_ptr(), a["y"].data_ptr(),
                                                     a["stats"].data_ptr(), N, H, s()))
            a["h0"] = self._lin2(a["y"], P[mp + "x_proj.0.weight"], P[mp + "x_proj.0.bias"], N, H, H)
            a["c"] = ops.new(2, N, H)
            _lib.check(lib.adf_op_ssilu_dual_fwd(a["h0"].data_ptr(), a["c"].data_ptr(), N * H, s()))
            a["xh"] = self._lin2(a["c"], P[mp + "x_proj.2.weight"], P[mp + "x_proj.2.bias"], N, 3 * H, H)
            rbfh2 = rbfh_of(l)
            x1, a["vec1"] = ops.new(2, N, H), ops.new(2, N, 3, H)
            _lib.check(lib.adf_op_message_dual_fwd(h, e_tan.data_ptr(), a["xh"].data_ptr(),
                                                   vec2.data_ptr() if vec2 is not None else None, rbfh2.data_ptr(),
                                                   x2.data_ptr(), x1.data_ptr(), a["vec1"].data_ptr(),
                                                   1 if vec2 is None else 0, E, s()))
            del rbfh2
            a["vv"] = self._lin2(a["vec1"], P[up + "vec_proj.weight"], None, 3 * N, 2 * H, H)
            a["cat"], a["dot"] = ops.new(2, N, 2 * H), ops.new(2, N, H)
            _lib.check(lib.adf_op_copy_rows(x1.data_ptr(), H, a["cat"].data_ptr(), 2 * H, 2 * N, H, 0, s()))
            _lib.check(lib.adf_op_vdot_dual_fwd(a["vv"].data_ptr(), a["dot"].data_ptr(), a["cat"].data_ptr() + 4 * H, 2 * H,
                                                N, H, C.c_float(1e-8), s()))
            a["u0"] = self._lin2(a["cat"], P[up + "xvec_proj.0.weight"], P[up + "xvec_proj.0.bias"], N, H, 2 * H)
            a["ua"] = ops.new(2, N, H)
            _lib.check(lib.adf_op_ssilu_dual_fwd(a["u0"].data_ptr(), a["ua"].data_ptr(), N * H, s()))
            a["a"] = self._lin2(a["ua"], P[up + "xvec_proj.2.weight"], P[up + "xvec_proj.2.bias"], N, 3 * H, H)
            xn, vn = ops.new(2, N, H), ops.new(2, N, 3, H)
            _lib.check(lib.adf_op_update_out_dual_fwd(x1.data_ptr(), a["vec1"].data_ptr(), a["a"].data_ptr(),
                                                      a["dot"].data_ptr(), a["vv"].data_ptr(), C.c_float(scales[l]),
                                                      xn.data_ptr(), vn.data_ptr(), N, H, s()))
            saved.append(a)
            x2, vec2 = xn, vn
        he0 = self._lin2(x2, P["out_energy.0.weight"], P["out_energy.0.bias"], N, H2, H)
        hea = ops.new(2, N, H2)
        _lib.check(lib.adf_op_ssilu_dual_fwd(he0.data_ptr(), hea.data_ptr(), N * H2, s()))

        # ---------------- phase 4: the joint backward, seeded with w on the atoms' energies and -1 on their tangents
        seed = torch.cat([dE.index_select(0, prep.batch.long()), torch.full((N,), -1.0, device=self.dev)]).reshape(2 * N, 1)
        seed = seed.contiguous()
        dhea = self._lin2_bwd(hea, P["out_energy.2.weight"], seed, N, 1, H2, G["out_energy.2.weight"],
                              G["out_energy.2.bias"])
        dhe0 = ops.new(2, N, H2)
        _lib.check(lib.adf_op_ssilu_dual_bwd(he0.data_ptr(), dhea.data_ptr(), dhe0.data_ptr(), N * H2, s()))
        dx = self._lin2_bwd(x2, P["out_energy.0.weight"], dhe0, N, H2, H, G["out_energy.0.weight"], G["out_energy.0.bias"])
        dvec = torch.zeros(2, N, 3, H, dtype=torch.float32, device=self.dev)
        if grads_ready is not None:
            grads_ready(["out_energy.", "out_forces."])
        for l in range(L - 1, -1, -1):
            a = saved[l]
            mp, up = f"message_layers.{l}.", f"update_layers.{l}."
            # update block
            da, ddot, dv1 = ops.new(2, N, 3 * H), ops.new(2, N, H), ops.new(2, N, 3, H)
            dx1, dvec1 = ops.new(2, N, H), ops.new(2, N, 3, H)
            _lib.check(lib.adf_op_update_out_dual_bwd(a["a"].data_ptr(), a["dot"].data_ptr(), a["vv"].data_ptr(),
                                                      C.c_float(scales[l]), dx.data_ptr(), dvec.data_ptr(), da.data_ptr(),
                                                      ddot.data_ptr(), dv1.data_ptr(), dx1.data_ptr(), dvec1.data_ptr(), N, H,
                                                      s()))
            dua = self._lin2_bwd(a["ua"], P[up + "xvec_proj.2.weight"], da, N, 3 * H, H, G[up + "xvec_proj.2.weight"],
                                 G[up + "xvec_proj.2.bias"])
            du0 = ops.new(2, N, H)
            _lib.check(lib.adf_op_ssilu_dual_bwd(a["u0"].data_ptr(), dua.data_ptr(), du0.data_ptr(), N * H, s()))
            dcat = self._lin2_bwd(a["cat"], P[up + "xvec_proj.0.weight"], du0, N, H, 2 * H, G[up + "xvec_proj.0.weight"],
                                  G[up + "xvec_proj.0.bias"])
            _lib.check(lib.adf_op_copy_rows(dcat.data_ptr(), 2 * H, dx1.data_ptr(), H, 2 * N, H, 1, s()))
            dvv = ops.new(2, N, 3, 2 * H)
            _lib.check(lib.adf_op_vdot_dual_bwd(a["vv"].data_ptr(), a["cat"].data_ptr() + 4 * H, 2 * H, ddot.data_ptr(),
                                                dcat.data_ptr() + 4 * H, 2 * H, dv1.data_ptr(), dvv.data_ptr(), N, H, s()))
            self._lin2_bwd(a["vec1"], P[up + "vec_proj.weight"], dvv, 3 * N, 2 * H, H, G[up + "vec_proj.weight"], None,
                           dA=dvec1, acc_dA=True)
            # message block
            first = a["vec"] is None
            rbfh2 = rbfh_of(l)
            dxh, drbfh = ops.new(2, N, 3 * H), ops.new(2 * E, 3 * H)
            dvec_in = None if first else ops.new(2, N, 3, H)
            dx_in = ops.new(2, N, H)
            _lib.check(lib.adf_op_message_dual_bwd(h, e_tan.data_ptr(), a["xh"].data_ptr(),
                                                   a["vec"].data_ptr() if not first else None, rbfh2.data_ptr(),
                                                   dx1.data_ptr(), dvec1.data_ptr(), dxh.data_ptr(), drbfh.data_ptr(),
                                                   dvec_in.data_ptr() if not first else None, dx_in.data_ptr(),
                                                   1 if first else 0, E, s()))
            del rbfh2
            self._lin2_bwd(rbf2, P[mp + "rbf_proj.weight"], drbfh, E, 3 * H, R, G[mp + "rbf_proj.weight"],
                           G[mp + "rbf_proj.bias"], want_dA=False)
            del drbfh
            dc = self._lin2_bwd(a["c"], P[mp + "x_proj.2.weight"], dxh, N, 3 * H, H, G[mp + "x_proj.2.weight"],
                                G[mp + "x_proj.2.bias"])
            dh0 = ops.new(2, N, H)
            _lib.check(lib.adf_op_ssilu_dual_bwd(a["h0"].data_ptr(), dc.data_ptr(), dh0.data_ptr(), N * H, s()))
            dy = self._lin2_bwd(a["y"], P[mp + "x_proj.0.weight"], dh0, N, H, H, G[mp + "x_proj.0.weight"],
                                G[mp + "x_proj.0.bias"])
            dlw, dlb = ops.new(H), ops.new(H)
            _lib.check(lib.adf_op_layernorm_dual_bwd(a["x"].data_ptr(), P[mp + "x_layernorm.weight"].data_ptr(),
                                                     a["stats"].data_ptr(), dy.data_ptr(), dx_in.data_ptr(), dlw.data_ptr(),
                                                     dlb.data_ptr(), N, H, ops.scratch(512 * 2 * H + 16).data_ptr(), s()))
            _lib.check(lib.adf_op_copy_rows(dlw.data_ptr(), H, G[mp + "x_layernorm.weight"].data_ptr(), H, 1, H, 1, s()))
            _lib.check(lib.adf_op_copy_rows(dlb.data_ptr(), H, G[mp + "x_layernorm.bias"].data_ptr(), H, 1, H, 1, s()))
            saved[l] = None
            dx, dvec = dx_in, dvec_in
            if grads_ready is not None:
                grads_ready([mp, up])
        # the embedding: the primal block of dx (the tangent of the embedding rows is zero, a constant)
        demb = G["atom_emb.embeddings.weight"]
        if self.ordered_embedding_backward:
            rows = int(demb.shape[0])
            sc = ops.scratch(int(lib.adf_op_embed_bwd_ordered_scratch(N, H, rows)))
            _lib.check(lib.adf_op_embed_bwd_ordered(dx.data_ptr(), prep.atomic_numbers.data_ptr(), demb.data_ptr(), N, H, rows,
                                                    sc.data_ptr(), s()))
        else:
            _lib.check(lib.adf_op_embed_bwd(dx.data_ptr(), prep.atomic_numbers.data_ptr(), demb.data_ptr(), N, H, s()))
        if grads_ready is not None:
            grads_ready(["atom_emb."])
        self.metrics = metrics
        self.last_outputs = (e_pred, f_pred)
        return loss


class FusedAdamW:
    """AdamW + global-norm clipping + EMA, one HIP launch per parameter tensor (csrc/train.hip: tr_adamw_kernel).
    Same update as torch.optim.AdamW(lr, betas, eps, weight_decay) preceded by clip_grad_norm_(max_norm) and followed
    by ExponentialMovingAverage.update (base_trainer.py:787-820); parameters named by ``no_decay`` get weight_decay 0
    (base_trainer.py:571-600, model.no_weight_decay())."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm: Optional[float] = None,
                 ema=None) -> None:
        self.lib = _lib.load()
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        self.ema = ema
        self.step_count = 0
        no_decay = set(model.no_weight_decay()) if hasattr(model, "no_weight_decay") else set()
        self.entries = []
        for name, p in model.named_parameters():
            if p.requires_grad:
                self.entries.append((name, p, torch.zeros_like(p), torch.zeros_like(p), name in no_decay))
        self.sqnorm = None

    def step(self) -> torch.Tensor:
        """Applies the update from ``param.grad``; returns the (pre-clip) global gradient norm as a device tensor."""
        self.step_count += 1
        dev = self.entries[0][1].device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if self.sqnorm is None:
            self.sqnorm = torch.zeros(1, device=dev)
        self.sqnorm.zero_()
        for _, p, _, _, _ in self.entries:
            if p.grad is not None:
                _lib.check(self.lib.adf_op_sqnorm_accumulate(p.grad.data_ptr(), p.numel(), self.sqnorm.data_ptr(), stream))
        shadows = self.ema.shadow_params if self.ema is not None else None
        decay = 0.0
        if self.ema is not None:
            decay = self.ema.decay
            if self.ema.num_updates is not None:
                self.ema.num_updates += 1
                decay = min(decay, (1 + self.ema.num_updates) / (10 + self.ema.num_updates))
        i = 0
        for _, p, m_, v_, nodecay in self.entries:
            if p.grad is None:
                i += 1
                continue
            _lib.check(self.lib.adf_op_adamw_step(
                p.data_ptr(), p.grad.data_ptr(), m_.data_ptr(), v_.data_ptr(),
                shadows[i].data_ptr() if shadows is not None else None, p.numel(), self.sqnorm.data_ptr(),
                C.c_float(self.max_grad_norm or 0.0), C.c_float(self.lr), C.c_float(self.betas[0]), C.c_float(self.betas[1]),
                C.c_float(self.eps), C.c_float(0.0 if nodecay else self.weight_decay), self.step_count, C.c_float(decay),
                stream))
            i += 1
        return self.sqnorm.sqrt()


# ------------------------------------------------------------------------------------------------ reproducible optimizer
def reference_param_groups(model, weight_decay: float) -> list:
    """The parameter groups of the reference's ``load_optimizer`` (base_trainer.py:556-609).  ``weight_decay > 0``: group 0
    holds the trainable parameters whose name ends with one of ``model.no_weight_decay()`` (weight decay 0), group 1 the
    other trainable ones, each in ``named_parameters()`` order; ``weight_decay == 0``: one group of ``model.parameters()``."""
    if weight_decay > 0:
        skip = tuple(model.no_weight_decay()) if hasattr(model, "no_weight_decay") else ()
        no_decay, decay = [], []
        for name, p in model.named_parameters():
            if not p.requires_grad:
                continue
            (no_decay if any(name.endswith(s) for s in skip) else decay).append(p)
        return [{"params": no_decay, "weight_decay": 0}, {"params": decay, "weight_decay": weight_decay}]
    return [{"params": list(model.parameters())}]


def adamw_state_to_flat(state_dict: dict):
    """``torch.optim.AdamW.state_dict()`` -> ``(step, {index: (exp_avg, exp_avg_sq)}, param_groups)``: the one step counter
    the multi-tensor optimizer keeps (0 for an empty state) and the moments by parameter index.  Per-parameter ``step``
    values that differ raise ``ValueError``: there is one counter."""
    steps = sorted({float(e["step"]) for e in state_dict["state"].values()})
    if len(steps) > 1:
        raise ValueError(f"the per-parameter step counts differ ({steps}); MultiTensorAdamW keeps one counter")
    step = int(steps[0]) if steps else 0
    if steps and float(step) != steps[0]:
        raise ValueError(f"step count {steps[0]} is not an integer")
    moments = {int(i): (e["exp_avg"], e["exp_avg_sq"]) for i, e in state_dict["state"].items()}
    return step, moments, [dict(g) for g in state_dict["param_groups"]]


def flat_to_adamw_state(step: int, moments: dict, param_groups: list) -> dict:
    """The inverse of ``adamw_state_to_flat``: torch's AdamW layout, ``step`` as the float32 CPU scalar torch keeps."""
    state = {int(i): {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
             for i, (m, v) in moments.items()}
    return {"state": state, "param_groups": [dict(g) for g in param_groups]}


class MultiTensorAdamW(torch.optim.Optimizer):
    """AdamW + global-norm clipping + EMA over every parameter tensor in three launches (csrc/optimizer.hip): the squared
    gradient norm in a fixed order (``adf_op_grad_sqnorm_multi``: one partial per chunk of ``chunk`` elements, added in index
    order in double) and ``tr_adamw_kernel``'s arithmetic over all chunks (``adf_op_adamw_multi``).  The step counter, the bias
    corrections, the clip factor and the EMA decay of the step live in a device state block; a step with a non-finite norm
    changes nothing but the block's ``skipped`` count.  ``step()`` reads nothing back.

    A ``torch.optim.Optimizer``: ``param_groups`` as the reference builds them (``reference_param_groups``), so torch's
    schedulers accept it, and ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.AdamW``'s layout.  ``step()`` takes
    the learning rate from ``param_groups[0]["lr"]`` and passes it to the kernel as an argument."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm: Optional[float] = None,
                 ema=None) -> None:
        # torch's own defaults for this version, so that a state written here loads into torch.optim.AdamW and runs
        defaults = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(reference_param_groups(model, weight_decay), defaults)
        self.lib = _lib.load()
        self.model = model
        self.max_grad_norm = max_grad_norm
        self.ema = ema
        self.chunk = int(self.lib.adf_op_optimizer_chunk())
        self.params = [p for g in self.param_groups for p in g["params"]]
        if not self.params:
            raise ValueError("MultiTensorAdamW: the model has no parameters")
        self.dev = self.params[0].device
        if self.dev.type != "cuda":
            raise RuntimeError("MultiTensorAdamW needs a ROCm device (the HIP path has no CPU fallback)")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.dev:
                raise ValueError("MultiTensorAdamW: parameters must be contiguous float32 tensors on one device")
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.had_grad = [False] * len(self.params)
        # chunk table: fixed for the life of the optimizer (every tensor, with or without a gradient)
        chunks = []
        for t, p in enumerate(self.params):
            chunks += [(t, o) for o in range(0, p.numel(), self.chunk)]
        self._chunks = np.asarray(chunks, dtype=np.int64).reshape(-1, 2)
        self.nchunks = int(self._chunks.shape[0])
        T = len(self.params)
        self._tables = torch.zeros(8 * T + 2 * self.nchunks, dtype=torch.int64, device=self.dev)
        self._partials = torch.zeros(self.nchunks, dtype=torch.float32, device=self.dev)
        # state block: int64 applied, skipped; int32 apply; float clip, bc1, bc2, ema_decay, sqnorm
        self._state = torch.zeros(5, dtype=torch.int64, device=self.dev)
        self._sqnorm = self._state.view(torch.float32)[9:10]
        self._signature = None
        self._applied_sync = 0     # the device counter as last read or written by the host
        self.resync_ema()

    # ------------------------------------------------------------------ tables
    def _shadow_of(self) -> dict:
        if self.ema is None:
            return {}
        trainable = [p for p in self.model.parameters() if p.requires_grad]
        return {id(p): s for p, s in zip(trainable, self.ema.shadow_params)}

    def _refresh_tables(self) -> None:
        """Rebuilds and uploads the tables (one asynchronous copy) when a pointer or a gradient's presence changed."""
        shadows = self._shadow_of()
        rows = []
        for i, p in enumerate(self.params):
            g = p.grad if p.requires_grad else None
            s = shadows.get(id(p))
            rows.append((p.data_ptr(), g.data_ptr() if g is not None else 0, self.exp_avg[i].data_ptr(),
                         self.exp_avg_sq[i].data_ptr(), s.data_ptr() if s is not None else 0))
        signature = tuple(rows)
        if signature == self._signature:
            return
        decay = {id(p): 1 if g.get("weight_decay", 0) else 0 for g in self.param_groups for p in g["params"]}
        host = torch.empty(self._tables.numel(), dtype=torch.int64).pin_memory()
        tab = host.numpy()
        T = len(self.params)
        for i, (p, row) in enumerate(zip(self.params, rows)):
            g = p.grad if p.requires_grad else None
            if g is not None:
                if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                    raise ValueError("MultiTensorAdamW: gradients must be contiguous float32 tensors of their parameter's shape")
                self.had_grad[i] = True
            s = shadows.get(id(p))
            if s is not None and (s.dtype != torch.float32 or not s.is_contiguous() or s.shape != p.shape
                                  or s.device != p.device):
                raise ValueError("MultiTensorAdamW: EMA shadows must be contiguous float32 tensors of their parameter's shape")
            tab[8 * i: 8 * i + 8] = (*row, p.numel(), decay[id(p)], 0)
        tab[8 * T:] = self._chunks.reshape(-1)
        self._tables.copy_(host, non_blocking=True)
        self._signature = signature

    def _weight_decay(self) -> float:
        values = {float(g.get("weight_decay", 0)) for g in self.param_groups} - {0.0}
        if len(values) > 1:
            raise ValueError(f"MultiTensorAdamW takes one non-zero weight decay, the groups hold {sorted(values)}")
        return values.pop() if values else 0.0

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None) -> torch.Tensor:
        """Applies the update from ``param.grad``; returns the (pre-clip) global gradient norm as a device tensor."""
        if closure is not None:
            raise NotImplementedError("MultiTensorAdamW.step takes no closure")
        g0 = self.param_groups[0]
        beta1, beta2 = g0["betas"]
        with torch.cuda.device(self.dev):
            self._refresh_tables()
            stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            tensors = self._tables.data_ptr()
            chunks = tensors + 8 * 8 * len(self.params)
            _lib.check(self.lib.adf_op_grad_sqnorm_multi(
                tensors, chunks, self.nchunks, self._partials.data_ptr(), self._state.data_ptr(),
                C.c_float(self.max_grad_norm or 0.0), C.c_double(beta1), C.c_double(beta2),
                C.c_float(self.ema.decay if self.ema is not None else 0.0), self._ema_n0, stream))
            _lib.check(self.lib.adf_op_adamw_multi(
                tensors, chunks, self.nchunks, self._state.data_ptr(), C.c_float(g0["lr"]), C.c_float(beta1),
                C.c_float(beta2), C.c_float(g0["eps"]), C.c_float(self._weight_decay()), stream))
        return self._sqnorm.sqrt()

    # ------------------------------------------------------------------ counters and state
    def counters(self) -> dict:
        """``{"applied", "skipped"}`` read from the device (a synchronising read: not for the step loop)."""
        applied, skipped = (int(v) for v in self._state[:2].tolist())
        return {"applied": applied, "skipped": skipped}

    def resync_ema(self) -> None:
        """Call after ``ema.load_state_dict`` / a new ``ema.num_updates``: the device forms the EMA decay of a step from
        ``num_updates`` at the last synchronisation plus the updates applied since."""
        n = getattr(self.ema, "num_updates", None) if self.ema is not None else None
        self._ema_n0 = -1 if n is None else int(n) - self._applied_sync
        self._signature = None   # the shadow tensors may be new ones

    def _sync_counter(self) -> int:
        applied = self.counters()["applied"]
        if self.ema is not None and self.ema.num_updates is not None:
            self.ema.num_updates = self._ema_n0 + applied
        self._applied_sync = applied
        return applied

    def state_dict(self) -> dict:
        """``torch.optim.AdamW``'s layout; ``step`` is the device counter, read here and only here, and
        ``ema.num_updates`` is refreshed from it.  A parameter that never had a gradient has no entry."""
        applied = self._sync_counter()
        moments = {i: (self.exp_avg[i], self.exp_avg_sq[i]) for i in range(len(self.params)) if self.had_grad[i]}
        groups, start = [], 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(start, start + len(g["params"])))
            start += len(g["params"])
            groups.append(packed)
        return flat_to_adamw_state(applied, moments, groups)

    def load_state_dict(self, state_dict: dict) -> None:
        step, moments, groups = adamw_state_to_flat(state_dict)
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"])
                                                        for a, b in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict has different parameter groups")
        for i, (m, v) in moments.items():
            if not 0 <= i < len(self.params) or m.shape != self.params[i].shape or v.shape != self.params[i].shape:
                raise ValueError(f"loaded state of parameter {i} does not fit")
        with torch.no_grad():
            for i in range(len(self.params)):
                if i in moments:
                    self.exp_avg[i].copy_(moments[i][0])
                    self.exp_avg_sq[i].copy_(moments[i][1])
                else:
                    self.exp_avg[i].zero_()
                    self.exp_avg_sq[i].zero_()
                self.had_grad[i] = i in moments
        for mine, theirs in zip(self.param_groups, groups):
            mine.update({k: copy.deepcopy(v) for k, v in theirs.items() if k != "params"})
        self._state.zero_()
        self._state[0] = step
        self._applied_sync = step
        self.resync_ema()


class GradientReducer:
    """Bucketed gradient all-reduce ISSUED FROM the backward pass (DDP over RCCL / xGMI, the reference's
    ``DistributedDataParallel(find_unused_parameters=True)``, base_trainer.py:442-447): ``ready(names)`` is called by
    ``PaiNNTrainStep.loss_and_grad`` as soon as the gradients of a group of parameters are final - the two heads first, then
    layer L-1 ... 0, the embedding last - and starts that bucket's all-reduce asynchronously (backend nccl = RCCL: the
    collective runs on the process group's own stream behind the kernels already enqueued, the remaining backward kernels
    keep the compute stream busy); ``finish()`` waits for the buckets, divides by the world size and writes the averages back.
    Parameters without a gradient on any rank (out_energy.*) are skipped consistently.  Buckets are one group each unless
    ``bucket_mb`` is smaller than a group (then the group is cut): a layer of the H = 512 model is 14.7 MB of gradients."""

    def __init__(self, model, world_size: int, bucket_mb: float = 64.0):
        self.world = int(world_size)
        self.limit = max(1, int(bucket_mb * 2**20 / 4))
        self.named = {k: p for k, p in model.named_parameters() if p.requires_grad}
        self.pending = []
        self.done_names = set()

    def _launch(self, grads) -> None:
        import torch.distributed as dist

        flat = torch.cat([g.reshape(-1) for g in grads])
        if dist.get_backend() == "gloo" and flat.is_cuda:  # test configuration: several ranks on one GPU
            host = flat.cpu()
            work = dist.all_reduce(host, op=dist.ReduceOp.SUM, async_op=True)
            self.pending.append((work, host, flat, grads))
        else:
            work = dist.all_reduce(flat, op=dist.ReduceOp.SUM, async_op=True)
            self.pending.append((work, flat, flat, grads))

    def ready(self, names) -> None:
        """The gradients of the parameters ``names`` (exact names or prefixes) are final."""
        if self.world <= 1:
            return
        sel = [k for k in self.named if k not in self.done_names and any(k == n or k.startswith(n) for n in names)]
        self.done_names.update(sel)
        bucket, size = [], 0
        for k in sel:
            g = self.named[k].grad
            if g is None:
                continue
            bucket.append(g)
            size += g.numel()
            if size >= self.limit:
                self._launch(bucket)
                bucket, size = [], 0
        if bucket:
            self._launch(bucket)

    def finish(self) -> None:
        if self.world <= 1:
            return
        self.ready([""])   # whatever was not announced (a caller without hooks): everything that is left
        for work, red, flat, grads in self.pending:
            work.wait()
            if red is not flat:
                flat.copy_(red)
            flat.div_(self.world)
            o = 0
            for g in grads:
                g.copy_(flat[o : o + g.numel()].view_as(g))
                o += g.numel()
        self.pending = []
        self.done_names = set()


def allreduce_gradients(model, world_size: int, bucket_mb: float = 64.0) -> None:
    """DDP step after a finished backward: average ``param.grad`` over the ranks in flat buckets (RCCL all-reduce over xGMI
    under backend nccl).  The training step itself overlaps the buckets with the backward (``GradientReducer``)."""
    if world_size <= 1:
        return
    GradientReducer(model, world_size, bucket_mb).finish()
