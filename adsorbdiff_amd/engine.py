"""Device-side engines of the score models: ``Engine`` converts a (PyG-like) batch into the ``adf_batch``
descriptor and enqueues the stepper and sampling-loop calls of either model on torch's current HIP stream;
``PaiNNEngine`` owns the PaiNN C-ABI handle, binds the module's parameters and runs its forward.

PyTorch is plumbing here (device memory, streams); all arithmetic is in
libadsorbdiff_hip.so.  Nothing in this file computes a model output on the host.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import lib as _lib


def cell_repeats(cell: torch.Tensor, radius: float, pbc: Sequence[bool] = (True, True, True)) -> List[int]:
    """Periodic images needed per lattice direction, max over the batch — host logic of
    the reference's radius_graph_pbc (adsorbdiff/utils/utils.py:634-662), evaluated with the same
    float32 torch ops on a CPU copy of ``cell``."""
    cell = cell.detach().to("cpu", torch.float32).reshape(-1, 3, 3)
    a1, a2, a3 = cell[:, 0], cell[:, 1], cell[:, 2]
    c23 = torch.cross(a2, a3, dim=-1)
    vol = torch.sum(a1 * c23, dim=-1, keepdim=True)
    crosses = (c23, torch.cross(a3, a1, dim=-1), torch.cross(a1, a2, dim=-1))
    reps = []
    for k in range(3):
        if pbc[k]:
            inv_min_dist = torch.norm(crosses[k] / vol, p=2, dim=-1)
            reps.append(int(torch.ceil(radius * inv_min_dist).max().item()))
        else:
            reps.append(0)
    return reps


def batch_pbc(data) -> List[bool]:
    """Reference: utils/utils.py:566-576 (default all-periodic; mixed PBC in one batch is an error)."""
    pbc = [True, True, True]
    if hasattr(data, "pbc") and getattr(data, "pbc") is not None:
        flags = torch.atleast_2d(data.pbc).to("cpu")
        for i in range(3):
            if not torch.any(flags[:, i]).item():
                pbc[i] = False
            elif torch.all(flags[:, i]).item():
                pbc[i] = True
            else:
                raise RuntimeError(
                    "Different structures in the batch have different PBC configurations. "
                    "This is not currently supported."
                )
    return pbc


@dataclass
class PreparedBatch:
    """Step-invariant device arrays of one batch (everything but positions)."""

    num_systems: int
    num_atoms: int
    cell: torch.Tensor          # [B,3,3] f32
    atomic_numbers: torch.Tensor  # [N] i32
    batch: torch.Tensor         # [N] i32
    atom_offset: torch.Tensor   # [B+1] i32
    reps: List[int]
    tags: Optional[torch.Tensor] = None   # [N] i32
    fixed: Optional[torch.Tensor] = None  # [N] i32
    edge_counts: Optional[Sequence[int]] = None   # [B] host: edges per system of an earlier build (tie-break of split_cut)

    def desc(self, pos: torch.Tensor) -> _lib.BatchDesc:
        d = _lib.BatchDesc()
        d.num_systems, d.num_atoms = self.num_systems, self.num_atoms
        d.pos = pos.data_ptr()
        d.cell = self.cell.data_ptr()
        d.atomic_numbers = self.atomic_numbers.data_ptr()
        d.batch = self.batch.data_ptr()
        d.atom_offset = self.atom_offset.data_ptr()
        d.reps[0], d.reps[1], d.reps[2] = self.reps
        return d


def image_repeats(batch, cutoff: float) -> List[int]:
    """``cell_repeats`` of a whole batch: the number of periodic images the graph search tries per lattice direction.  It is
    the largest need over the batch (as in the reference), so it is the one thing a system's graph takes from its
    batch-mates: an adsorbate atom that has left the cell can gain a neighbour when a mate with a smaller cell raises the
    count.  Pinning it (``denoising_pos_params["image_repeats"]``) removes that."""
    return cell_repeats(batch.cell, float(cutoff), batch_pbc(batch))


def split_cut(natoms: Sequence[int], edges: Optional[Sequence[int]] = None) -> int:
    """Systems of view A when a batch with these atom counts is cut in two for ``adf_sample_split``
    (``adf_split_choose_cut``: host arithmetic in the library, no device): the boundary where the two sides' atom counts
    are closest, ties to the closest ``edges`` (per-system edge counts of an earlier build, optional), then the lowest.
    0 for fewer than two systems: no split."""
    n = (C.c_int32 * max(len(natoms), 1))(*[int(x) for x in natoms])
    e = None
    if edges is not None:
        if len(edges) != len(natoms):
            raise ValueError(f"split_cut: {len(natoms)} atom counts, {len(edges)} edge counts")
        e = (C.c_int64 * max(len(edges), 1))(*[int(x) for x in edges])
    cut = C.c_int32(-1)
    _lib.check(_lib.load().adf_split_choose_cut(n, e, len(natoms), C.byref(cut)))
    return int(cut.value)


def _require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} is on {t.device}: the adsorbdiff_amd HIP path only runs on a ROCm device "
            "(there is no CPU fallback)"
        )


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _numel(t: Optional[torch.Tensor]) -> int:
    return int(t.numel()) if t is not None else 0


def sampler_draws(seed: int, keys: torch.Tensor, site: Optional[torch.Tensor], num_steps: int, device, place: bool = True,
                  z_a: bool = False, z_b: bool = False):
    """The sampler's keyed draws (``adf_sampler_draws``) -> (place [B,3] | None, z_a [T,B,3] | None, z_b | None), float32 on
    ``device``.  A system's rows depend on ``(seed, keys[b], site[b])`` alone."""
    dev = torch.device(device)
    keys = torch.as_tensor(keys, dtype=torch.int64).reshape(-1).to(dev).contiguous()
    B, T = int(keys.shape[0]), int(num_steps)
    if site is not None:
        site = torch.as_tensor(site).reshape(-1).to(dev, torch.int32).contiguous()
        if site.shape[0] != B:
            raise ValueError(f"sampler_draws: {B} keys, {site.shape[0]} site indices")
    out = [torch.empty(shape, dtype=torch.float32, device=dev) if want else None
           for want, shape in ((place, (B, 3)), (z_a, (T, B, 3)), (z_b, (T, B, 3)))]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seed = seed - (1 << 64) if seed >= (1 << 63) else seed
    with torch.cuda.device(dev):
        _lib.check(_lib.load().adf_sampler_draws(seed, keys.data_ptr(), _ptr(site), B, T, *[_ptr(t) for t in out],
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return tuple(out)


class Engine:
    """What both score models' engines share: the stepper entries, the fused sampling loops, the static-atom promise,
    the flags and arithmetic switches and the handle's lifetime.  A subclass creates the handle, binds the weights,
    runs the forward and names its C entries in ``SYMBOLS`` (role -> symbol)."""

    SYMBOLS: dict = {}

    def __init__(self, model, device) -> None:
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs a ROCm device, got {self.device} (no CPU fallback)")
        self.model = model
        self.exact_f32 = os.environ.get("ADF_GEMM") == "f32"
        self._weights_keepalive: List[torch.Tensor] = []
        self._moving_keepalive = None
        self._sys_state_keepalive = None

    def _c(self, role: str):
        return getattr(self.lib, self.SYMBOLS[role])

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ batches
    def prepare(self, data, image_repeats: Optional[Sequence[int]] = None) -> PreparedBatch:
        """``image_repeats``: a floor for the periodic images per direction (never fewer than this batch needs; a
        non-periodic direction stays at 0)."""
        _require_gpu(data.pos, "data.pos")
        dev = self.device
        natoms = data.natoms.to(dev, torch.int64).reshape(-1)
        B = int(natoms.shape[0])
        N = int(data.pos.shape[0])
        off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        off[1:] = torch.cumsum(natoms, 0).to(torch.int32)
        cell = data.cell.to(dev, torch.float32).reshape(B, 3, 3).contiguous()
        reps = cell_repeats(cell, float(self.model.cutoff), batch_pbc(data))
        if image_repeats is not None:
            if len(image_repeats) != 3:
                raise ValueError(f"image_repeats: three counts expected, got {list(image_repeats)}")
            reps = [max(int(r), int(f)) if r > 0 else 0 for r, f in zip(reps, image_repeats)]
        prep = PreparedBatch(
            num_systems=B, num_atoms=N, cell=cell,
            atomic_numbers=data.atomic_numbers.to(dev).long().to(torch.int32).contiguous(),
            batch=data.batch.to(dev, torch.int32).contiguous(),
            atom_offset=off, reps=reps,
        )
        if hasattr(data, "tags") and data.tags is not None:
            prep.tags = data.tags.to(dev, torch.int32).contiguous()
        if hasattr(data, "fixed") and data.fixed is not None:
            prep.fixed = data.fixed.to(dev, torch.int32).contiguous()
        return prep

    def bind_condition(self, data, num_systems: int) -> None:
        """What a conditional model reads from the batch besides the atoms; nothing for the others."""

    def set_moving_atoms(self, prep: Optional[PreparedBatch], moving_mask: Optional[torch.Tensor]) -> None:
        """Declare which atoms may move between the next graph builds of ``prep`` (None switches the
        static-atom cache off).  The arrays are kept alive on the engine until the next call."""
        if moving_mask is None or prep is None:
            self._moving_keepalive = None
            _lib.check(self._c("set_moving")(self.handle, None, None, None))
            return
        mask = moving_mask.to(self.device, torch.int32).contiguous()
        idx = torch.nonzero(mask).reshape(-1).to(torch.int32).contiguous()
        per_sys = torch.bincount(prep.batch[idx.long()].long(), minlength=prep.num_systems)
        off = torch.zeros(prep.num_systems + 1, dtype=torch.int32, device=self.device)
        off[1:] = torch.cumsum(per_sys, 0).to(torch.int32)
        self._moving_keepalive = (mask, idx, off)
        _lib.check(self._c("set_moving")(self.handle, mask.data_ptr(), idx.data_ptr(), off.data_ptr()))

    # ------------------------------------------------------------------ switches
    def check_flags(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self._c("check_flags")(self.handle, self._stream()))

    def use_exact_f32(self) -> bool:
        """Switch the handle to exact-f32 arithmetic (after a NumericRangeError in the default f16x3 mode: an
        activation left the fp16 range).  Returns False if it already was exact."""
        if self.exact_f32:
            return False
        logging.warning("adsorbdiff_amd: non-finite output in f16x3 arithmetic; re-running in exact f32 "
                        "(this engine stays in exact f32)")
        _lib.check(self._c("set_arithmetic")(self.handle, 1))
        self.exact_f32 = True
        return True

    def set_incremental(self, on: bool = True) -> None:
        """Incremental layers / blocks: keep the node state of every layer across the forwards of a static-atom
        promise and recompute only rows whose inputs changed.  Bit-identical outputs."""
        _lib.check(self._c("set_incremental")(self.handle, 1 if on else 0))

    def set_per_system_stop(self, sys_state: Optional[torch.Tensor]) -> None:
        """Per-system early stop of the step entries and fused loops of this handle (``adf_*_set_per_system_stop``):
        ``sys_state`` int32 ``[B,4]`` on the device, rows ``{cvg_count, frozen, steps_applied, stop_step}`` initialised to
        ``{0, 0, 0, -1}``; None switches the mode off.  The tensor is kept alive on the engine until the next call."""
        if sys_state is None:
            self._sys_state_keepalive = None
            _lib.check(self._c("set_per_system_stop")(self.handle, None, 0))
            return
        if (sys_state.dtype != torch.int32 or sys_state.dim() != 2 or sys_state.shape[1] != 4 or not sys_state.is_contiguous()
                or sys_state.device != self.device):
            raise ValueError("set_per_system_stop: contiguous int32 [B,4] on the engine's device expected")
        self._sys_state_keepalive = sys_state
        _lib.check(self._c("set_per_system_stop")(self.handle, sys_state.data_ptr(), int(sys_state.shape[0])))

    # ------------------------------------------------------------------ stepper
    def init_placement(self, prep: PreparedBatch, pos: torch.Tensor, noise: torch.Tensor) -> None:
        desc = prep.desc(pos)
        with torch.cuda.device(self.device):
            _lib.check(self._c("init_placement")(
                self.handle, C.byref(desc), pos.data_ptr(), prep.tags.data_ptr(), noise.data_ptr(), self._stream()))

    def sde_step(self, prep: PreparedBatch, pos, f1, f2, coef: _lib.StepCoef, state, z_tr=None, z_rot=None,
                 early_stop_count: int = 10, dcom=None, drot=None) -> None:
        self._sde_step(prep, pos, f1, f2, coef, None, 0, state, z_tr, z_rot, early_stop_count, dcom, drot)

    def sde_step_scheduled(self, prep: PreparedBatch, pos, f1, f2, coefs_dev: torch.Tensor, num_steps: int, state,
                           z_tr=None, z_rot=None, early_stop_count: int = 10) -> None:
        """Step whose schedule scalars come from a device table indexed by state[4] (graph-capturable)."""
        self._sde_step(prep, pos, f1, f2, None, coefs_dev, num_steps, state, z_tr, z_rot, early_stop_count, None, None)

    def _sde_entry(self, coef, coefs_dev, num_steps):
        """The step entry and its schedule arguments: one entry that takes either form."""
        return self._c("sde_step"), (C.byref(coef) if coef is not None else None, _ptr(coefs_dev), num_steps)

    def _sde_step(self, prep, pos, f1, f2, coef, coefs_dev, num_steps, state, z_tr, z_rot, early_stop_count, dcom, drot):
        desc = prep.desc(pos)
        entry, schedule = self._sde_entry(coef, coefs_dev, num_steps)
        with torch.cuda.device(self.device):
            _lib.check(entry(self.handle, C.byref(desc), pos.data_ptr(), prep.tags.data_ptr(), _ptr(prep.fixed),
                             f1.data_ptr(), f2.data_ptr(), *schedule, _ptr(z_tr), _ptr(z_rot), early_stop_count,
                             state.data_ptr(), _ptr(dcom), _ptr(drot), self._stream()))

    def sample(self, prep: PreparedBatch, pos, f1, f2, coefs_dev: torch.Tensor, num_steps: int, state,
               z_tr_all=None, z_rot_all=None, early_stop_count: int = 10, poll_every: int = 0,
               out_idx: Optional[torch.Tensor] = None, sink=None, frame_every: int = 1,
               split_streams: Optional[bool] = None) -> None:
        """The whole reverse loop in one library call (``adf_sample``; with ``sink`` — a ``trajectory.FrameSink`` —
        ``adf_sample_traj``: a frame of the positions leaves the device after every ``frame_every``-th step).
        ``split_streams``: two half-batches on two streams where the engine has that form (``PaiNNEngine.sample``);
        ignored here."""
        self._loop("sample", prep, pos, [_ptr(prep.fixed), coefs_dev.data_ptr(), num_steps, _ptr(z_tr_all),
                                         _ptr(z_rot_all), early_stop_count, poll_every, state.data_ptr(), _ptr(out_idx),
                                         _numel(out_idx), f1.data_ptr(), f2.data_ptr()], sink, frame_every)

    def tr_step(self, prep: PreparedBatch, pos, f1, state, coef: Optional[_lib.TrCoef] = None,
                coefs_dev: Optional[torch.Tensor] = None, num_steps: int = 0, z=None, early_stop_count: int = 10,
                dcom=None) -> None:
        """One step of the translation-only samplers (``adf_tr_step``): head-1 mean over the adsorbate, dcom =
        coef * score (+ noise * z), COM wrap, pos += dcom.  Scalars from ``coef`` or from the device table
        ``coefs_dev`` [num_steps, 2] indexed by state[4]."""
        desc = prep.desc(pos)
        with torch.cuda.device(self.device):
            _lib.check(self._c("tr_step")(
                self.handle, C.byref(desc), pos.data_ptr(), prep.tags.data_ptr(), f1.data_ptr(),
                C.byref(coef) if coef is not None else None, _ptr(coefs_dev), int(num_steps), _ptr(z), early_stop_count,
                state.data_ptr(), _ptr(dcom), self._stream()))

    def tr_sample(self, prep: PreparedBatch, pos, f1, coefs_dev: torch.Tensor, num_steps: int, state, z_all=None,
                  early_stop_count: int = 10, poll_every: int = 0, out_idx=None, sink=None, frame_every: int = 1) -> None:
        """The whole translation-only loop in one library call (``adf_tr_sample[_traj]``); the forward inside
        evaluates head 1 only."""
        self._loop("tr_sample", prep, pos, [coefs_dev.data_ptr(), int(num_steps), _ptr(z_all), early_stop_count,
                                            poll_every, state.data_ptr(), _ptr(out_idx), _numel(out_idx), f1.data_ptr()],
                   sink, frame_every)

    def _loop(self, role: str, prep: PreparedBatch, pos, args: list, sink, frame_every: int) -> None:
        desc = prep.desc(pos)
        head = [self.handle, C.byref(desc), pos.data_ptr(), prep.tags.data_ptr()]
        with torch.cuda.device(self.device):
            if sink is None:
                _lib.check(self._c(role)(*head, *args, self._stream()))
            else:
                _lib.check(self._c(role + "_traj")(*head, *args, sink.handle, int(frame_every), self._stream()))

    # ------------------------------------------------------------------ lifetime
    def profile_enable(self, on: bool = True) -> None:
        _lib.check(self._c("profile_enable")(self.handle, 1 if on else 0))

    def close(self) -> None:
        if getattr(self, "handle", None) is not None and self.handle:
            with torch.cuda.device(self.device):
                torch.cuda.synchronize(self.device)
                twin = getattr(self, "_twin", None)
                if twin is not None and twin:   # it reads this handle's weight images: it goes first
                    self._c("destroy")(twin)
                    self._twin = None
                self._c("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PaiNNEngine(Engine):
    SYMBOLS = dict(set_moving="adf_graph_set_moving", check_flags="adf_check_flags",
                   set_arithmetic="adf_painn_set_arithmetic", set_incremental="adf_painn_set_incremental",
                   init_placement="adf_sde_init_placement", sample="adf_sample", sample_traj="adf_sample_traj",
                   tr_step="adf_tr_step", tr_sample="adf_tr_sample", tr_sample_traj="adf_tr_sample_traj",
                   set_per_system_stop="adf_painn_set_per_system_stop",
                   profile_enable="adf_profile_enable", destroy="adf_painn_destroy")

    def __init__(self, model, device) -> None:
        super().__init__(model, device)
        hp = _lib.Hparams(
            hidden_channels=model.hidden_channels, num_layers=model.num_layers, num_rbf=model.num_rbf,
            num_elements=model.num_elements, max_neighbors=model.max_neighbors,
            envelope_exponent=int(model.radial_basis.envelope.p),
            num_heads=getattr(model, "num_force_heads", 2 if model.so3_denoising else 1),
            cutoff=float(model.cutoff),
        )
        self.num_heads = hp.num_heads
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_painn_create(C.byref(hp), C.byref(self.handle)))
        self._last_graph_N = 0
        self._twin = None                 # adf_painn_create_twin, made by the first split run
        self._split_keepalive = None      # view B's re-based index arrays of the last split run
        self._moving_gen = 0
        self._split_moving = None         # view B's re-based moving lists of the promise in force: (key, mov_idx, mov_off)
        self._split_default = bool(self.get_tune()["sample_split"])   # ADF_SAMPLE_SPLIT as the handle read it
        floor = getattr(model, "distance_floor", None)   # the S2EF PaiNN: 1e-6 (painn.py:334-335); default 1e-3
        if floor is not None:
            _lib.check(self.lib.adf_painn_set_distance_floor(self.handle, float(floor)))
        self.bind_weights()

    # ------------------------------------------------------------------ weights
    def _weight_list(self) -> List[torch.Tensor]:
        m = self.model
        sd = dict(m.named_parameters())
        sd.update(dict(m.named_buffers()))
        names = ["atom_emb.embeddings.weight", "radial_basis.rbf.offset"]
        for i in range(m.num_layers):
            p, u = f"message_layers.{i}.", f"update_layers.{i}."
            names += [
                p + "x_layernorm.weight", p + "x_layernorm.bias", p + "x_proj.0.weight", p + "x_proj.0.bias",
                p + "x_proj.2.weight", p + "x_proj.2.bias", p + "rbf_proj.weight", p + "rbf_proj.bias",
                u + "vec_proj.weight", u + "xvec_proj.0.weight", u + "xvec_proj.0.bias",
                u + "xvec_proj.2.weight", u + "xvec_proj.2.bias",
            ]
        heads = ["out_forces", "out_forces2"][:self.num_heads]
        for hname in heads:
            for b in range(2):
                q = f"{hname}.output_network.{b}."
                names += [q + "vec1_proj.weight", q + "vec2_proj.weight", q + "update_net.0.weight",
                          q + "update_net.0.bias", q + "update_net.2.weight", q + "update_net.2.bias"]
        out = []
        for n in names:
            t = sd[n].detach()
            _require_gpu(t, f"parameter {n}")
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            out.append(t)
        return out

    def bind_weights(self) -> None:
        ws = self._weight_list()
        self._weights_keepalive = ws
        ptrs = (C.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
        scales = self.model.scale_factors()
        sf = (C.c_float * len(scales))(*scales)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_painn_set_weights(self.handle, len(ws), ptrs, sf, self._stream()))
        if getattr(self.model, "energy_head", False):   # S2EF PaiNN: out_energy (adf_painn_set_energy_head)
            oe = self.model.out_energy
            es = [t.detach().to(torch.float32).contiguous() for t in (oe[0].weight, oe[0].bias, oe[2].weight, oe[2].bias)]
            for t in es:
                _require_gpu(t, "out_energy parameter")
            self._weights_keepalive = ws + es
            eptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in es])
            with torch.cuda.device(self.device):
                _lib.check(self.lib.adf_painn_set_energy_head(self.handle, 4, eptrs, self._stream()))

    # ------------------------------------------------------------------ two half-batches, two streams
    def set_moving_atoms(self, prep, moving_mask) -> None:
        self._moving_gen += 1
        super().set_moving_atoms(prep, moving_mask)

    def split_view(self, prep: PreparedBatch, out_idx: Optional[torch.Tensor]):
        """View B of ``prep`` for ``adf_sample_split`` -> (``lib.SplitView``, the tensors it points into).  The cut comes
        from ``adf_split_choose_cut`` on the host copy of the atom counts (ties go to ``prep.edge_counts`` where the caller
        has set them); what counts atoms or systems from the start of the batch (atom offsets, system index, ``out_idx``,
        the moving lists) is re-based to view B's first atom / system.  The cut and the batch's own arrays are kept on
        ``prep``; the moving lists on the engine for as long as the static-atom promise they belong to, because the twin
        reads them until the promise changes; ``out_idx``'s share is formed anew at every call."""
        cached = getattr(prep, "_split_cut", None)
        if cached is None:
            off = prep.atom_offset.cpu()
            cut = split_cut((off[1:] - off[:-1]).tolist(), prep.edge_counts)
            na = int(off[cut])
            cached = prep._split_cut = (cut, na, (prep.atom_offset[cut:] - na).contiguous(), (prep.batch[na:] - cut).contiguous())
        cut, na, off_b, batch_b = cached
        v = _lib.SplitView()
        v.cut, v.atoms_a, v.atom_offset, v.batch = cut, na, off_b.data_ptr(), batch_b.data_ptr()
        keep = [off_b, batch_b]
        if out_idx is not None:
            n_a = int((out_idx < na).sum().item())
            keep.append((out_idx[n_a:] - na).contiguous())
            v.n_out_a, v.n_out_b, v.out_idx = n_a, int(out_idx.numel()) - n_a, keep[-1].data_ptr()
        if self._moving_keepalive is not None:
            if self._split_moving is None or self._split_moving[0] != (self._moving_gen, cut, na):
                _, idx, moff = self._moving_keepalive
                m0 = int(moff[cut].item())
                self._split_moving = ((self._moving_gen, cut, na), (idx[m0:] - na).contiguous(), (moff[cut:] - m0).contiguous())
            v.mov_idx, v.mov_off = self._split_moving[1].data_ptr(), self._split_moving[2].data_ptr()
        return v, keep

    def split_stats(self):
        """(runs of ``sample`` that went through the split loop, runs that ``adf_sample_split`` gave to the one-stream loop)."""
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(self.lib.adf_split_stats(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def sample(self, prep: PreparedBatch, pos, f1, f2, coefs_dev: torch.Tensor, num_steps: int, state,
               z_tr_all=None, z_rot_all=None, early_stop_count: int = 10, poll_every: int = 0,
               out_idx: Optional[torch.Tensor] = None, sink=None, frame_every: int = 1,
               split_streams: Optional[bool] = None) -> None:
        """``Engine.sample``; with ``split_streams`` (default: ``ADF_SAMPLE_SPLIT`` as the handle read it) the two sides of a
        cut at a system boundary run on two streams (``adf_sample_split``; include/adsorbdiff_hip.h, section "Two
        half-batches, two streams") - same bits.  A trajectory sink and a batch of one system take the one-stream
        loop here; the library's own fallbacks (exact f32, the coupled early stop) are counted by ``split_stats``."""
        want = self._split_default if split_streams is None else bool(split_streams)
        if not want or sink is not None or prep.num_systems < 2:
            return super().sample(prep, pos, f1, f2, coefs_dev, num_steps, state, z_tr_all, z_rot_all, early_stop_count,
                                  poll_every, out_idx, sink, frame_every)
        with torch.cuda.device(self.device):
            if self._twin is None:
                twin = C.c_void_p()
                _lib.check(self.lib.adf_painn_create_twin(self.handle, C.byref(twin)))
                self._twin = twin
            _lib.check(self.lib.adf_painn_set_split(self.handle, 1))
            view, keep = self.split_view(prep, out_idx)
            self._split_keepalive = keep
            desc = prep.desc(pos)
            _lib.check(self.lib.adf_sample_split(
                self.handle, self._twin, C.byref(desc), C.byref(view), pos.data_ptr(), prep.tags.data_ptr(), _ptr(prep.fixed),
                coefs_dev.data_ptr(), num_steps, _ptr(z_tr_all), _ptr(z_rot_all), early_stop_count, poll_every,
                state.data_ptr(), _ptr(out_idx), _numel(out_idx), f1.data_ptr(), f2.data_ptr(), self._stream()))

    # ------------------------------------------------------------------ calls
    def forward_prepared(self, prep: PreparedBatch, pos: torch.Tensor, f1: torch.Tensor, f2: Optional[torch.Tensor],
                         out_idx: Optional[torch.Tensor] = None) -> None:
        """Enqueue one forward; no host synchronisation.  ``out_idx`` (ascending int32 atom indices on the
        device): evaluate the outputs of these atoms only — their rows of f1 / f2 are bit-identical to the full
        forward's, the other rows are left untouched (``adf_painn_forward_subset``)."""
        desc = prep.desc(pos)
        with torch.cuda.device(self.device):
            if out_idx is None:
                _lib.check(self.lib.adf_painn_forward(
                    self.handle, C.byref(desc), f1.data_ptr(), f2.data_ptr() if f2 is not None else None, self._stream()))
            else:
                assert out_idx.dtype == torch.int32 and out_idx.is_contiguous() and out_idx.device == pos.device
                _lib.check(self.lib.adf_painn_forward_subset(
                    self.handle, C.byref(desc), out_idx.data_ptr(), int(out_idx.numel()), f1.data_ptr(),
                    f2.data_ptr() if f2 is not None else None, self._stream()))

    def forward(self, data):
        prep = self.prepare(data)
        pos = data.pos.to(torch.float32).contiguous()
        f1 = torch.empty(prep.num_atoms, 3, dtype=torch.float32, device=self.device)
        f2 = torch.empty_like(f1) if self.model.so3_denoising else None
        self.forward_prepared(prep, pos, f1, f2)
        try:
            self.check_flags()  # ValueError on an image without neighbours, like the reference
        except _lib.NumericRangeError:
            if not self.use_exact_f32():  # already exact: the inputs / weights themselves are not finite
                raise
            self.forward_prepared(prep, pos, f1, f2)
            self.check_flags()
        return f1, f2

    def forward_observe(self, data, upto: Optional[int] = None, with_heads: bool = False):
        """The full forward that also observes what a ``ScaleFactor`` fit reads (``adf_painn_forward_observe``): ->
        ``layer_var`` float64 ``[num_layers]`` on the device, entry l = ``torch.mean(torch.var(x, dim=0))`` of the node
        features after update layer l's scale multiply; entries after ``upto`` (default: the last layer) are NaN, their
        layers are not run.  ``with_heads`` (``upto`` the last layer only): -> ``(layer_var, f1, f2)`` with the heads'
        outputs as ``forward`` gives them.  Ends a static-atom promise.  Same error protocol as ``forward``."""
        L = int(self.model.num_layers)
        upto = L - 1 if upto is None else int(upto)
        prep = self.prepare(data)
        pos = data.pos.to(torch.float32).contiguous()
        layer_var = torch.full((L,), float("nan"), dtype=torch.float64, device=self.device)
        f1 = f2 = None
        if with_heads:
            f1 = torch.empty(prep.num_atoms, 3, dtype=torch.float32, device=self.device)
            f2 = torch.empty_like(f1) if self.num_heads == 2 else None
        self._moving_keepalive = None   # the library forgets the promise: so does its keeper
        self._moving_gen += 1
        desc = prep.desc(pos)

        def run():
            with torch.cuda.device(self.device):
                _lib.check(self.lib.adf_painn_forward_observe(self.handle, C.byref(desc), upto, layer_var.data_ptr(),
                                                              _ptr(f1), _ptr(f2), self._stream()))
        run()
        try:
            self.check_flags()
        except _lib.NumericRangeError:
            if not self.use_exact_f32():
                raise
            run()
            self.check_flags()
        return (layer_var, f1, f2) if with_heads else layer_var

    def forward_energy_prepared(self, prep: PreparedBatch, pos: torch.Tensor, energy: torch.Tensor,
                                forces: Optional[torch.Tensor]) -> None:
        """Enqueue one S2EF forward (``adf_painn_forward_energy``): energy [B], forces [N,3] (None without a force
        head); no host synchronisation."""
        desc = prep.desc(pos)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_painn_forward_energy(
                self.handle, C.byref(desc), energy.data_ptr(), forces.data_ptr() if forces is not None else None,
                self._stream()))

    def forward_energy(self, data):
        """S2EF forward of the model's energy head and (if it has one) its force head -> (energy [B], forces [N,3] | None).
        Same error protocol as ``forward``."""
        prep = self.prepare(data)
        pos = data.pos.to(torch.float32).contiguous()
        energy = torch.empty(prep.num_systems, dtype=torch.float32, device=self.device)
        forces = torch.empty(prep.num_atoms, 3, dtype=torch.float32, device=self.device) if self.num_heads else None
        self.forward_energy_prepared(prep, pos, energy, forces)
        try:
            self.check_flags()
        except _lib.NumericRangeError:
            if not self.use_exact_f32():
                raise
            self.forward_energy_prepared(prep, pos, energy, forces)
            self.check_flags()
        return energy, forces

    def forward_energy_gradient_prepared(self, prep: PreparedBatch, pos: torch.Tensor, energy: torch.Tensor,
                                         forces: torch.Tensor) -> None:
        """Enqueue one evaluation of the energy [B] and of forces [N,3] = -dE/dpos, the gradient of that energy with the
        edge set held fixed (``adf_painn_forward_energy_gradient``: what ``torch.autograd.grad(energy.sum(), pos)`` gives
        on the reference); no host synchronisation.  Works without a force head."""
        desc = prep.desc(pos)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_painn_forward_energy_gradient(
                self.handle, C.byref(desc), energy.data_ptr(), forces.data_ptr(), self._stream()))

    def forward_energy_gradient(self, data):
        """-> (energy [B], forces [N,3] = -dE/dpos).  Same error protocol as ``forward_energy``: a non-finite value in
        f16x3 arithmetic re-runs in exact f32, out of memory is a ``RuntimeError`` (``ml_relax`` then halves the batch)."""
        prep = self.prepare(data)
        pos = data.pos.to(torch.float32).contiguous()
        energy = torch.empty(prep.num_systems, dtype=torch.float32, device=self.device)
        forces = torch.empty(prep.num_atoms, 3, dtype=torch.float32, device=self.device)
        self.forward_energy_gradient_prepared(prep, pos, energy, forces)
        try:
            self.check_flags()
        except _lib.NumericRangeError:
            if not self.use_exact_f32():
                raise
            self.forward_energy_gradient_prepared(prep, pos, energy, forces)
            self.check_flags()
        return energy, forces

    def energy_gradient_workspace_bytes(self, num_atoms: int) -> int:
        """Device memory the library holds for ``forward_energy_gradient`` on a batch of ``num_atoms`` atoms."""
        n = C.c_int64(0)
        _lib.check(self.lib.adf_painn_energy_gradient_workspace(self.handle, int(num_atoms), C.byref(n)))
        return int(n.value)

    def get_tune(self) -> dict:
        """The kernel-selection switches this engine's handle read from the environment when it was created
        (adf_painn_get_tune): field name -> value.  The variants give the same bits, so only this shows the selection."""
        t = _lib.Tune()
        _lib.check(self.lib.adf_painn_get_tune(self.handle, C.byref(t)))
        return {name: int(getattr(t, name)) for name, _ in _lib.Tune._fields_}

    def build_graph(self, data, prep=None):
        """Graph only; returns the number of symmetrised edges.  ``prep``: an already prepared batch of ``data``."""
        if prep is None:
            prep = self.prepare(data)
        pos = data.pos.to(torch.float32).contiguous()
        desc = prep.desc(pos)
        n = C.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_graph_build(self.handle, C.byref(desc), self._stream(), C.byref(n)))
        self._last_graph_N = prep.num_atoms
        return int(n.value)

    def export_graph(self):
        """(nbr_count[N], nbr_src[N,K], nbr_shift[N,K,3], edge_src[E], edge_dst[E], dist[E], vec[E,3])."""
        N, K = self._last_graph_N, self.model.max_neighbors
        if N <= 0:
            raise RuntimeError("export_graph: call build_graph first")
        dev = self.device
        cnt = torch.empty(N, dtype=torch.int32, device=dev)
        src = torch.empty(N, K, dtype=torch.int32, device=dev)
        sh = torch.empty(N, K, 3, dtype=torch.int32, device=dev)
        cap = 2 * N * K
        es = torch.empty(cap, dtype=torch.int32, device=dev)
        ed = torch.empty(cap, dtype=torch.int32, device=dev)
        dist = torch.empty(cap, dtype=torch.float32, device=dev)
        vec = torch.empty(cap, 3, dtype=torch.float32, device=dev)
        n = C.c_int64(0)
        with torch.cuda.device(dev):
            _lib.check(self.lib.adf_graph_export(
                self.handle, cnt.data_ptr(), src.data_ptr(), sh.data_ptr(), cap, es.data_ptr(), ed.data_ptr(),
                dist.data_ptr(), vec.data_ptr(), C.byref(n), self._stream()))
        E = int(n.value)
        return cnt, src, sh, es[:E], ed[:E], dist[:E], vec[:E]

    def message_layer(self, layer: int, x: torch.Tensor, vec: torch.Tensor):
        x_out, vec_out = torch.empty_like(x), torch.empty_like(vec)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_painn_message_layer(
                self.handle, layer, x.shape[0], x.data_ptr(), vec.data_ptr(), x_out.data_ptr(), vec_out.data_ptr(),
                self._stream()))
        return x_out, vec_out

    def update_layer(self, layer: int, x: torch.Tensor, vec: torch.Tensor):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_painn_update_layer(
                self.handle, layer, x.shape[0], x.data_ptr(), vec.data_ptr(), self._stream()))
        return x, vec

    def _sde_entry(self, coef, coefs_dev, num_steps):
        """Two step entries here: adf_sde_step (host scalars) and adf_sde_step_scheduled (device table)."""
        if coef is not None:
            return self.lib.adf_sde_step, (C.byref(coef),)
        return self.lib.adf_sde_step_scheduled, (coefs_dev.data_ptr(), num_steps)

    def counters(self) -> _lib.Counters:
        c = _lib.Counters()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_get_counters(self.handle, C.byref(c), self._stream()))
        return c

    PROFILE_CATEGORIES = ("graph", "message", "node_dense", "heads", "stepper")

    def profile_read(self):
        """{category: (total_ms, groups)} since the last read (HIP events on the launch stream)."""
        ms = (C.c_float * 5)()
        cnt = (C.c_int64 * 5)()
        ksteps = C.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_profile_read(self.handle, ms, cnt, C.byref(ksteps), self._stream()))
        out = {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.PROFILE_CATEGORIES)}
        out["message_ksteps"] = int(ksteps.value)
        return out

    def measure_peaks(self):
        """On-box peaks for the roofline fractions: HBM stream copy (GB/s), f16 and f32 MFMA (TFLOP/s)."""
        out = (C.c_float * 3)()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.adf_measure_peaks(out, self._stream()))
        return {"hbm_copy_gbps": float(out[0]), "mfma_f16_tflops": float(out[1]), "mfma_f32_tflops": float(out[2])}
