"""Device-side engine of the EquiformerV2 denoiser and of the S2EF force field built from the same blocks
(``equiformer_v2_oc20.EquiformerV2_OC20``: ``forward_energy``): owns the ``adf_eqv2`` handle, hands over the constant SO(3) tables
(so3_math.py) and the module's parameters, and enqueues forward calls on torch's current HIP stream; the stepper and
sampling calls are ``engine.Engine``'s, shared with ``PaiNNEngine``.  PyTorch is plumbing here; nothing in this file
computes a model output on the host.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import lib as _lib
from . import so3_math
from .engine import Engine, PreparedBatch, _require_gpu


def attn_weight_names(prefix: str, mmax: int) -> List[str]:
    rad = [f"net.{i}.{k}" for i in (0, 1, 3, 4, 6) for k in ("weight", "bias")]
    names = [prefix + "alpha_dot", prefix + "source_embedding.weight", prefix + "target_embedding.weight",
             prefix + "so2_conv_1.fc_m0.weight", prefix + "so2_conv_1.fc_m0.bias"]
    names += [prefix + f"so2_conv_1.so2_m_conv.{m}.fc.weight" for m in range(mmax)]
    names += [prefix + "so2_conv_1.rad_func." + r for r in rad]
    names += [prefix + "alpha_norm.weight", prefix + "alpha_norm.bias", prefix + "so2_conv_2.fc_m0.weight",
              prefix + "so2_conv_2.fc_m0.bias"]
    names += [prefix + f"so2_conv_2.so2_m_conv.{m}.fc.weight" for m in range(mmax)]
    names += [prefix + "proj.weight", prefix + "proj.bias"]
    return names


def weight_names(num_layers: int, mmax: int) -> List[str]:
    """The table order of ``adf_eqv2_set_weights`` (include/adsorbdiff_hip.h) in reference state_dict names."""
    rad = [f"net.{i}.{k}" for i in (0, 1, 3, 4, 6) for k in ("weight", "bias")]
    norm = ["affine_weight", "norm_l0.weight", "norm_l0.bias"]
    names = ["atom_radii", "sphere_embedding.weight", "edge_degree_embedding.source_embedding.weight",
             "edge_degree_embedding.target_embedding.weight"]
    names += ["edge_degree_embedding.rad_func." + r for r in rad]
    for i in range(num_layers):
        p = f"blocks.{i}."
        names += [p + "norm_1." + n for n in norm]
        names += attn_weight_names(p + "ga.", mmax)
        names += [p + "norm_2." + n for n in norm]
        names += [p + "ffn." + n for n in ("so3_linear_1.weight", "so3_linear_1.bias", "scalar_mlp.0.weight",
                                            "scalar_mlp.0.bias", "grid_mlp.0.weight", "grid_mlp.2.weight",
                                            "grid_mlp.4.weight", "so3_linear_2.weight", "so3_linear_2.bias")]
    names += ["norm." + n for n in norm]
    names += attn_weight_names("force_block.", mmax)
    names += attn_weight_names("force_block2.", mmax)
    return names


def s2ef_weight_names(num_layers: int, mmax: int) -> List[str]:
    """The table order of ``adf_eqv2_set_weights_s2ef``: the denoiser's table without ``atom_radii`` and without
    ``force_block2``."""
    return [n for n in weight_names(num_layers, mmax)[1:] if not n.startswith("force_block2.")]


# energy_block entries the energy reaches (adf_eqv2_set_energy_head); row 0 of so3_linear_2.weight[0] is sliced out
ENERGY_HEAD_NAMES = ["energy_block.scalar_mlp.0.weight", "energy_block.scalar_mlp.0.bias",
                     "energy_block.so3_linear_2.weight", "energy_block.so3_linear_2.bias"]


class EqV2Engine(Engine):
    PROFILE_CATEGORIES = ("graph", "radial", "rotate", "so2_conv", "s2_act", "attn_weights", "node", "ffn_grid", "stepper")
    SYMBOLS = dict(set_moving="adf_eqv2_set_moving", check_flags="adf_eqv2_check_flags",
                   set_arithmetic="adf_eqv2_set_arithmetic", set_incremental="adf_eqv2_set_incremental",
                   init_placement="adf_eqv2_init_placement", sde_step="adf_eqv2_sde_step", sample="adf_eqv2_sample",
                   sample_traj="adf_eqv2_sample_traj", tr_step="adf_eqv2_tr_step", tr_sample="adf_eqv2_tr_sample",
                   tr_sample_traj="adf_eqv2_tr_sample_traj", profile_enable="adf_eqv2_profile_enable",
                   set_per_system_stop="adf_eqv2_set_per_system_stop", destroy="adf_eqv2_destroy")
    num_heads = 2   # force_block and force_block2

    def __init__(self, model, device) -> None:
        super().__init__(model, device)
        self.s2ef = bool(getattr(model, "s2ef", False))
        if self.s2ef:
            self.num_heads = 1 if model.regress_forces else 0
        self.lmax, self.mmax = int(model.lmax_list[0]), int(model.mmax_list[0])
        hp = _lib.EqV2Hparams(
            lmax=self.lmax, mmax=self.mmax, num_layers=model.num_layers, sphere_channels=model.sphere_channels,
            attn_hidden_channels=model.attn_hidden_channels, num_heads=model.num_heads,
            attn_alpha_channels=model.attn_alpha_channels, attn_value_channels=model.attn_value_channels,
            ffn_hidden_channels=model.ffn_hidden_channels, grid_resolution=int(model.grid_resolution),
            edge_channels=model.edge_channels, num_distance_basis=model.NUM_GAUSSIANS,
            max_num_elements=model.max_num_elements, max_neighbors=model.max_neighbors,
            max_radius=float(model.max_radius), avg_degree=float(model.avg_degree),
        )
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_create(C.byref(hp), C.byref(self.handle)))
            t = so3_math.device_tables(self.lmax, self.mmax, int(model.grid_resolution))
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            _lib.check(self.lib.adf_eqv2_set_constants(self.handle, ptr(t["jd"]), ptr(t["to_red"]), ptr(t["from_red"]),
                                                       ptr(t["to_full"]), ptr(t["from_full"])))
        self._edges_keepalive = None
        self._ext_edges = 0        # edges of the list set_edges last handed over (0: the engine builds its own graph)
        self._energy_keepalive = None
        self._energy_mode = None   # what adf_eqv2_set_system_energy last received: None (never), "zeros", "given"
        self._energy_gradient = None   # eqv2_train_step.EqV2EnergyGradient, made by the first forward_energy_gradient
        self.bind_weights()

    # ------------------------------------------------------------------ weights
    def _tensor(self, sd, n: str) -> torch.Tensor:
        t = sd[n].detach()
        _require_gpu(t, f"parameter {n}")
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        return t

    def _bind_s2ef(self) -> None:
        """The S2EF model: its table (no radii, one force block) and the energy head."""
        m = self.model
        sd = dict(m.named_parameters())
        names = s2ef_weight_names(m.num_layers, self.mmax)
        if not m.regress_forces:   # no force block: the first block's tensors as placeholders; forces = NULL reads none
            if m.num_layers < 1:
                raise ValueError("an energy-only EquiformerV2 needs at least one block")
            names = [n.replace("force_block.", "blocks.0.ga.") for n in names]
        out = [self._tensor(sd, n) for n in names]
        ptrs = (C.c_void_p * len(out))(*[w.data_ptr() for w in out])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_set_weights_s2ef(self.handle, len(out), ptrs, self._stream()))
        head = [self._tensor(sd, n) for n in ENERGY_HEAD_NAMES]
        head[2] = head[2][0, 0].contiguous()   # so3_linear_2.weight [L+1, 1, F]: the l = 0 row
        ref = self._tensor(sd, "energy_lin_ref") if m.use_energy_lin_ref else None
        self._weights_keepalive = out + head + ([ref] if ref is not None else [])
        hptrs = (C.c_void_p * 4)(*[w.data_ptr() for w in head])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_set_energy_head(self.handle, 4, hptrs, float(m.avg_num_nodes),
                                                         ref.data_ptr() if ref is not None else None, self._stream()))

    def bind_weights(self) -> None:
        if self.s2ef:
            return self._bind_s2ef()
        sd = dict(self.model.named_parameters())
        out = [self._tensor(sd, n) for n in weight_names(self.model.num_layers, self.mmax)]
        self._weights_keepalive = out
        ptrs = (C.c_void_p * len(out))(*[w.data_ptr() for w in out])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_set_weights(self.handle, len(out), ptrs, self._stream()))
        ee = getattr(self.model, "energy_embedding", None)
        if ee is not None:  # the conditional model: nn.Linear(1, C), evaluated in fp16 by the library
            wb = [t.detach().to(torch.float32).reshape(-1).contiguous() for t in (ee.weight, ee.bias)]
            for t, n in zip(wb, ("energy_embedding.weight", "energy_embedding.bias")):
                _require_gpu(t, f"parameter {n}")
            self._weights_keepalive += wb
            with torch.cuda.device(self.device):
                _lib.check(self.lib.adf_eqv2_set_energy_embedding(self.handle, wb[0].data_ptr(), wb[1].data_ptr(),
                                                                  self._stream()))

    # ------------------------------------------------------------------ conditional model
    def set_system_energy(self, energy: Optional[torch.Tensor]) -> None:
        """Per-system energies [B] of the conditional model (adf_eqv2_set_system_energy); ``None``: zeros (sampling
        mode).  Drops the incremental blocks' kept state."""
        if energy is None:
            self._energy_keepalive = None
            _lib.check(self.lib.adf_eqv2_set_system_energy(self.handle, None, 0, self._stream()))
            self._energy_mode = "zeros"
            return
        e = energy.to(self.device, torch.float32).reshape(-1).contiguous()
        self._energy_keepalive = e
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_set_system_energy(self.handle, e.data_ptr(), int(e.numel()), self._stream()))
        self._energy_mode = "given"

    def bind_condition(self, data, num_systems: int) -> None:
        """What the conditional model reads from a batch (equiformer_v2_denoising.py:258-264): nothing when
        ``sampling`` (zero energies), else ``data.energy`` per system.  No-op for the unconditional model."""
        if getattr(self.model, "energy_embedding", None) is None:
            return
        if self.model.sampling:
            if self._energy_mode != "zeros":
                self.set_system_energy(None)
            return
        energy = getattr(data, "energy", None)
        if energy is None:
            raise ValueError("the conditional EquiformerV2 (energy_encoding='scalar') with sampling=False reads "
                             "data.energy (one value per system); the batch has none")
        energy = torch.as_tensor(energy).reshape(-1)
        if int(energy.numel()) != int(num_systems):
            raise ValueError(f"data.energy has {int(energy.numel())} values for {int(num_systems)} systems")
        self.set_system_energy(energy)

    def set_edges(self, edge_index: Optional[torch.Tensor], edge_vec: Optional[torch.Tensor]) -> None:
        """Run the next forwards on this edge list ([2,E] (source, target) sorted by target, vectors [E,3]) instead of
        building one; ``None`` switches back.  For parity runs against reference outputs whose choice among exactly tied
        K-th neighbours is implementation-defined."""
        if edge_index is None:
            _lib.check(self.lib.adf_eqv2_set_edges(self.handle, 0, None, None, None, 1, self._stream()))
            self._ext_edges = 0
            return
        dst = edge_index[1].to(self.device, torch.int32).contiguous()
        src = edge_index[0].to(self.device, torch.int32).contiguous()
        if dst.numel() > 1 and bool((dst[1:] < dst[:-1]).any().item()):
            raise ValueError("set_edges: edges must be sorted by target")
        vec = edge_vec.to(self.device, torch.float32).contiguous()
        maxdeg = int(torch.bincount(dst.long()).max().item())
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_set_edges(self.handle, int(dst.numel()), src.data_ptr(), dst.data_ptr(),
                                                   vec.data_ptr(), maxdeg, self._stream()))
        self._ext_edges = int(dst.numel())

    def export_graph(self, data, prep: Optional[PreparedBatch] = None):
        """The graph of ``data`` as the forward builds it (``adf_eqv2_export_graph``; the list of ``set_edges`` while one is
        in force) -> (eptr [N+1], src [E], dst [E], vec [E,3], wig [E,DR]): edges sorted by target, int32 indices, ``wig``
        the Wigner rows kept per edge.  The counterpart of ``PaiNNEngine.export_graph`` for the training step."""
        if prep is None:
            prep = self.prepare(data)
        pos = data.pos.to(torch.float32).contiguous()
        N, dev = prep.num_atoms, self.device
        cap = max(self._ext_edges or N * int(self.model.max_neighbors), 1)
        DR = sum((2 * min(l, self.mmax) + 1) * (2 * l + 1) for l in range(self.lmax + 1))
        eptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        src = torch.empty(cap, dtype=torch.int32, device=dev)
        dst = torch.empty(cap, dtype=torch.int32, device=dev)
        vec = torch.empty(cap, 3, dtype=torch.float32, device=dev)
        wig = torch.empty(cap, DR, dtype=torch.float32, device=dev)
        n = C.c_int64(0)
        desc = prep.desc(pos)
        with torch.cuda.device(dev):
            _lib.check(self.lib.adf_eqv2_export_graph(self.handle, C.byref(desc), cap, eptr.data_ptr(), src.data_ptr(),
                                                      dst.data_ptr(), vec.data_ptr(), wig.data_ptr(), C.byref(n),
                                                      self._stream()))
        self.check_flags()
        E = int(n.value)
        return eptr, src[:E], dst[:E], vec[:E], wig[:E]

    # ------------------------------------------------------------------ calls
    def forward_prepared(self, prep: PreparedBatch, pos: torch.Tensor, f1: torch.Tensor, f2: Optional[torch.Tensor],
                         out_idx=None, x_blocks: Optional[torch.Tensor] = None) -> None:
        """Enqueue one forward; no host synchronisation.  ``out_idx`` (ascending int32 atom indices on the device): only
        those rows of f1 / f2 are evaluated - bit-identical to the full forward's - and written
        (``adf_eqv2_forward_subset``)."""
        desc = prep.desc(pos)
        with torch.cuda.device(self.device):
            if out_idx is not None:
                if x_blocks is not None:
                    raise ValueError("x_blocks are recorded by the full forward only")
                assert out_idx.dtype == torch.int32 and out_idx.is_contiguous() and out_idx.device == pos.device
                _lib.check(self.lib.adf_eqv2_forward_subset(
                    self.handle, C.byref(desc), out_idx.data_ptr(), int(out_idx.numel()), f1.data_ptr(),
                    f2.data_ptr() if f2 is not None else None, self._stream()))
                return
            _lib.check(self.lib.adf_eqv2_forward(
                self.handle, C.byref(desc), f1.data_ptr(), f2.data_ptr() if f2 is not None else None,
                x_blocks.data_ptr() if x_blocks is not None else None, self._stream()))

    def forward_energy_prepared(self, prep: PreparedBatch, pos: torch.Tensor, energy: torch.Tensor,
                                forces: Optional[torch.Tensor], x_blocks: Optional[torch.Tensor] = None) -> None:
        """Enqueue one S2EF forward (``adf_eqv2_forward_energy``): energy [B], forces [N,3] (None: the force block is not
        evaluated); no host synchronisation."""
        desc = prep.desc(pos)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_forward_energy(
                self.handle, C.byref(desc), energy.data_ptr(), forces.data_ptr() if forces is not None else None,
                x_blocks.data_ptr() if x_blocks is not None else None, self._stream()))

    def forward_energy(self, data, return_blocks: bool = False):
        """S2EF forward -> (energy [B], forces [N,3] | None) (+ the block embeddings with ``return_blocks``)."""
        if not self.s2ef:
            raise RuntimeError("forward_energy: this engine is bound to the denoiser (no energy head)")
        prep = self.prepare(data)
        pos = data.pos.to(torch.float32).contiguous()
        energy = torch.empty(prep.num_systems, dtype=torch.float32, device=self.device)
        forces = torch.empty(prep.num_atoms, 3, dtype=torch.float32, device=self.device) if self.num_heads else None
        xb = None
        if return_blocks:
            xb = torch.empty(self.model.num_layers + 1, prep.num_atoms, (self.lmax + 1) ** 2, self.model.sphere_channels,
                             dtype=torch.float32, device=self.device)
        self.forward_energy_prepared(prep, pos, energy, forces, xb)
        self.check_flags()
        return (energy, forces, xb) if return_blocks else (energy, forces)

    def forward_energy_gradient(self, data):
        """-> (energy [B], forces [N,3] = -dE/dpos of that energy, the edge set held fixed).  Works without a force block.
        The energy is the exact-f32 training forward's in ``eval()`` (``EqV2EnergyGradient``), within 1.3e-6 of max|E| of
        ``forward_energy``'s.  Out of memory is a ``RuntimeError`` (``ml_relax`` then halves the batch): this forward holds
        the activations of every block until its backward has run."""
        if not self.s2ef:
            raise RuntimeError("forward_energy_gradient: this engine is bound to the denoiser (no energy head)")
        if self._energy_gradient is None:
            from .eqv2_train_step import EqV2EnergyGradient

            self._energy_gradient = EqV2EnergyGradient(self.model, self.device)
        return self._energy_gradient(data)

    def forward(self, data, return_blocks: bool = False):
        if self.s2ef:
            raise RuntimeError("forward: the S2EF model has one force block and an energy head; use forward_energy")
        prep = self.prepare(data)
        self.bind_condition(data, prep.num_systems)
        pos = data.pos.to(torch.float32).contiguous()
        f1 = torch.empty(prep.num_atoms, 3, dtype=torch.float32, device=self.device)
        f2 = torch.empty_like(f1)
        xb = None
        if return_blocks:
            S = (self.lmax + 1) ** 2
            xb = torch.empty(self.model.num_layers + 1, prep.num_atoms, S, self.model.sphere_channels,
                             dtype=torch.float32, device=self.device)
        self.forward_prepared(prep, pos, f1, f2, x_blocks=xb)
        self.check_flags()
        return (f1, f2, xb) if return_blocks else (f1, f2)

    def set_arithmetic(self, exact_f32: bool) -> None:
        _lib.check(self.lib.adf_eqv2_set_arithmetic(self.handle, 1 if exact_f32 else 0))
        self.exact_f32 = bool(exact_f32)

    def counters(self) -> _lib.EqV2Counters:
        c = _lib.EqV2Counters()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_get_counters(self.handle, C.byref(c), self._stream()))
        return c

    def profile_read(self):
        n = len(self.PROFILE_CATEGORIES)
        ms = (C.c_float * n)()
        cnt = (C.c_int64 * n)()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_eqv2_profile_read(self.handle, ms, cnt, self._stream()))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.PROFILE_CATEGORIES)}
