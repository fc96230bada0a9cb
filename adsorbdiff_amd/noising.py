"""Forward noising of a training batch — mirror of ``tr_so3_schedule`` / ``pbc_correction``
(adsorbdiff/trainers/sde_denoising_trainer.py:45-135): per system a diffusion time t ~ U(0,1), a Gaussian in-plane
displacement of the adsorbate's centre of mass (minimum-image wrapped), an IGSO(3) rotation about it and the +1 A lift;
the batch gets ``tr_sigma, rot_sigma, tr_score, rot_score, ads_center_noise_vec`` attached and its adsorbate positions
overwritten, exactly like the reference's in-place version.  Host-side data preparation (B rows of 3-vectors per
batch); random streams are consumed in the reference's order (torch.rand, torch normal_, then numpy per system).

``ads_COM_gaussian_schedule`` mirrors the reference's noising of the translation-only (one-head) model (:138-177).

Device noising (opt-in, csrc/noising.hip): ``DeviceNoiser`` draws one row of eight numbers per system from a counter-based
generator keyed by ``(seed, step, noise_keys(batch))`` and noises the batch in one kernel, without a host read; a system
then receives the same noise alone, in any batch and on any rank.  ``tr_so3_schedule_from_draws`` and
``ads_COM_gaussian_schedule_from_draws`` are the host functions of the same row table (the arithmetic of the mirrors
above): the oracle of the kernels.  Row = ``(u_t, n0, n1, n2, n3, n4, n5, u_om)``: uniform of the diffusion time, COM
noise, rotation axis before normalisation, uniform of the rotation angle's CDF look-up.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import torch

from .so3_tables import Igso3Tables


def axis_angle_to_matrix(v: torch.Tensor) -> torch.Tensor:
    """[3] axis-angle -> [3,3] via the unit quaternion (adsorbdiff/utils/rot_utils.py:18-98, small-angle series below 1e-6)."""
    ang = torch.linalg.norm(v)
    half = 0.5 * ang
    k = 0.5 - ang * ang / 48 if float(ang.abs()) < 1e-6 else torch.sin(half) / ang
    qr, (qi, qj, qk) = torch.cos(half), v * k
    two_s = 2.0 / (qr * qr + qi * qi + qj * qj + qk * qk)
    return torch.stack([
        1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
        two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
        two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)]).reshape(3, 3)


def axis_angle_to_matrix_batch(v: np.ndarray) -> np.ndarray:
    """[B,3] float64 axis-angles -> [B,3,3] float64: the same formulas, all systems at once (the per-system torch version
    above costs ~20 small CPU tensor ops per system: 20 ms per 256-system batch)."""
    v = np.asarray(v, dtype=np.float64)
    ang = np.linalg.norm(v, axis=1)
    half = 0.5 * ang
    small = np.abs(ang) < 1e-6
    k = np.where(small, 0.5 - ang * ang / 48, np.sin(half) / np.where(small, 1.0, ang))
    qr = np.cos(half)
    qi, qj, qk = v[:, 0] * k, v[:, 1] * k, v[:, 2] * k
    two_s = 2.0 / (qr * qr + qi * qi + qj * qj + qk * qk)
    return np.stack([
        1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
        two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
        two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)], axis=1).reshape(-1, 3, 3)


@torch.no_grad()
def pbc_correction(noise_vec: torch.Tensor, cell: torch.Tensor) -> torch.Tensor:
    """[B,3] vectors wrapped to the minimum image of their system's cell: fractional coordinates by an fp64 solve with
    cell^T, into (-0.5, 0.5], back with the rows of cell."""
    frac = torch.linalg.solve(cell.transpose(1, 2).double(), noise_vec.double().unsqueeze(-1)).squeeze(-1)
    frac = frac % 1.0 % 1.0
    frac = torch.where(frac > 0.5, frac - 1, frac)
    return torch.einsum("bi,bij->bj", frac.float(), cell.float())


def _sigmas(t: torch.Tensor, lo, hi) -> torch.Tensor:
    return lo ** (1 - t) * hi**t


def _ads_center(batch, B: int):
    """(adsorbate mask, system of every adsorbate atom, centre of mass [B,3]); tag 2 marks the adsorbate."""
    dev = batch.pos.device
    ads = batch.tags == 2
    bidx = batch.batch[ads]
    cnt = torch.zeros(B, device=dev).index_add_(0, bidx, torch.ones(bidx.shape[0], device=dev))
    center = torch.zeros(B, 3, device=dev).index_add_(0, bidx, batch.pos[ads]) / cnt[:, None]
    return ads, bidx, center


def _tr_so3_apply(batch, B: int, tr_sigma, rot_sigma, normal, upds, rot_score):
    """``tr_so3_schedule`` after its draws: ``normal`` [B,3] float32 standard normals of the COM noise, ``upds`` /
    ``rot_score`` [B,3] float64 axis-angle updates and their scores (host)."""
    dev = batch.pos.device
    ads, bidx, center = _ads_center(batch, B)
    noise = normal * tr_sigma[:, None]
    noise = pbc_correction(noise, batch.cell.reshape(B, 3, 3))
    noise[:, -1] = 0
    R = torch.from_numpy(axis_angle_to_matrix_batch(upds).astype(np.float32)).to(dev)
    rel = batch.pos[ads] - center[bidx]
    new_ads = torch.einsum("nj,nij->ni", rel, R[bidx]) + noise[bidx] + center[bidx]
    new_ads[:, -1] += 1  # the reference lifts the noised adsorbate by 1 A
    batch.pos = batch.pos.clone()
    batch.pos[ads] = new_ads
    batch.tr_sigma, batch.rot_sigma = tr_sigma[:, None], rot_sigma[:, None]
    batch.rot_score = torch.from_numpy(rot_score.astype(np.float32)).to(dev)
    batch.ads_center_noise_vec = noise
    batch.tr_score = -noise / tr_sigma[:, None] ** 2
    return batch


@torch.no_grad()
def tr_so3_schedule(batch, denoise_pos_params: dict, tables: Igso3Tables = None):
    tables = tables or Igso3Tables.shared()
    dev = batch.pos.device
    B = int(batch.natoms.shape[0])
    t = torch.rand(size=(B,), device=dev)
    tr_sigma = _sigmas(t, denoise_pos_params["ads_std_low"], denoise_pos_params["ads_std_high"])
    rot_sigma = _sigmas(t, denoise_pos_params["rot_std_low"], denoise_pos_params["rot_std_high"])
    normal = torch.zeros(B, 3, device=dev).normal_()
    rot_sigma_h = rot_sigma.cpu().numpy()
    # the numpy stream is consumed system by system, as the reference does (sample_vec, then score_vec of every system);
    # the table look-ups of all systems run at once (10 -> 1.5 ms of host time per 256 systems and training step)
    upds, rot_score = tables.sample_and_score_vecs(rot_sigma_h.astype(np.float64))
    return _tr_so3_apply(batch, B, tr_sigma, rot_sigma, normal, upds, rot_score)


def _com_apply(batch, B: int, tr_sigma, normal):
    """``ads_COM_gaussian_schedule`` after its draws (``normal`` [B,3] float32 standard normals)."""
    ads, _, center = _ads_center(batch, B)
    noise = normal * tr_sigma[:, None]
    noise[:, -1] = 0  # noise only in x, y
    center = center + noise
    # the samplers' wrap: the COLUMNS of cell act as lattice vectors, all three components are wrapped
    cell = batch.cell.reshape(B, 3, 3).float()
    frac = torch.linalg.solve(cell, center)
    frac = frac % 1 % 1
    center = torch.einsum("bi,bij->bj", frac, cell.transpose(1, 2))
    center[:, -1] += 1  # the reference lifts the noised adsorbate by 1 A
    batch.pos = batch.pos.clone()
    batch.pos[ads] = center[batch.batch][ads]  # the adsorbate collapses to its noised centre, as in the reference
    batch.tr_sigma = tr_sigma[:, None]
    batch.ads_center_noise_vec = noise
    batch.tr_score = -noise / tr_sigma[:, None] ** 2
    return batch


@torch.no_grad()
def ads_COM_gaussian_schedule(batch, denoise_pos_params: dict):
    """Mirror of ``ads_COM_gaussian_schedule`` (sde_denoising_trainer.py:138-177), the noising of the one-head model:
    t ~ U(0,1) per system (``torch.rand`` on the batch's device), a Gaussian in-plane displacement of the adsorbate's centre
    (``normal_`` on a zero [B,3] tensor, z set to 0), the centre wrapped into the cell and lifted by 1 A, every adsorbate
    atom set to it.  Attaches ``tr_sigma [B,1], ads_center_noise_vec, tr_score``; ``batch.pos`` becomes a new tensor."""
    dev = batch.pos.device
    B = int(batch.natoms.shape[0])
    t = torch.rand(size=(B,), device=dev)
    tr_sigma = _sigmas(t, denoise_pos_params["ads_std_low"], denoise_pos_params["ads_std_high"])
    normal = torch.zeros(B, 3, device=dev).normal_()
    return _com_apply(batch, B, tr_sigma, normal)


# ---------------------------------------------------------------------------------------------------- keyed draws
def noise_key_source(batch) -> str:
    """Where ``noise_keys`` takes a batch's keys from: ``"noise_key"``, ``"sid"`` or ``"index"`` (the position in the batch:
    the only source that does not identify a system wherever it appears)."""
    B = int(batch.natoms.shape[0])
    if getattr(batch, "noise_key", None) is not None:
        return "noise_key"
    sid = getattr(batch, "sid", None)
    return "sid" if sid is not None and len(sid) == B else "index"


def noise_keys(batch) -> torch.Tensor:
    """int64 [B] keys of the systems for the counter-based draws, by preference: ``batch.noise_key`` (int64 [B]); the first
    8 bytes (little endian) of ``blake2b(str(sid))`` per system where ``batch.sid`` is present; the system's index in the
    batch otherwise.  The first two identify a system wherever it appears; the index fallback does NOT: with it the noise
    of a system still depends on its position in the batch."""
    B = int(batch.natoms.shape[0])
    source = noise_key_source(batch)
    if source == "noise_key":
        key = torch.as_tensor(batch.noise_key).reshape(-1)
        if key.dtype != torch.int64 or key.numel() != B:
            raise ValueError(f"batch.noise_key: int64 [{B}] expected, got {key.dtype} [{key.numel()}]")
        return key
    if source == "sid":
        return torch.tensor([int.from_bytes(hashlib.blake2b(str(s).encode("utf-8")).digest()[:8], "little", signed=True)
                             for s in batch.sid], dtype=torch.int64)
    return torch.arange(B, dtype=torch.int64)


def _draw_rows(draws, B: int) -> np.ndarray:
    d = draws.detach().cpu().numpy() if torch.is_tensor(draws) else np.asarray(draws)
    d = np.ascontiguousarray(d, dtype=np.float64)
    if d.shape != (B, 8):
        raise ValueError(f"draws: [{B}, 8] expected, got {list(d.shape)}")
    return d


@torch.no_grad()
def tr_so3_schedule_from_draws(batch, denoise_pos_params: dict, draws, tables: Igso3Tables = None):
    """``tr_so3_schedule`` with its random numbers read from ``draws`` [B,8] (float64 rows, layout in the module
    docstring) instead of the torch / numpy streams: the same arithmetic, on the batch's device."""
    tables = tables or Igso3Tables.shared()
    dev = batch.pos.device
    B = int(batch.natoms.shape[0])
    d = _draw_rows(draws, B)
    t = torch.from_numpy(d[:, 0].astype(np.float32)).to(dev)
    tr_sigma = _sigmas(t, denoise_pos_params["ads_std_low"], denoise_pos_params["ads_std_high"])
    rot_sigma = _sigmas(t, denoise_pos_params["rot_std_low"], denoise_pos_params["rot_std_high"])
    normal = torch.from_numpy(d[:, 1:4].astype(np.float32)).to(dev)
    upds, rot_score = tables.vecs_and_scores_from_draws(rot_sigma.cpu().numpy().astype(np.float64), d[:, 4:7], d[:, 7])
    return _tr_so3_apply(batch, B, tr_sigma, rot_sigma, normal, upds, rot_score)


@torch.no_grad()
def ads_COM_gaussian_schedule_from_draws(batch, denoise_pos_params: dict, draws):
    """``ads_COM_gaussian_schedule`` from ``(u_t, n0, n1)`` of the rows of ``draws`` [B,8]."""
    dev = batch.pos.device
    B = int(batch.natoms.shape[0])
    d = _draw_rows(draws, B)
    t = torch.from_numpy(d[:, 0].astype(np.float32)).to(dev)
    tr_sigma = _sigmas(t, denoise_pos_params["ads_std_low"], denoise_pos_params["ads_std_high"])
    normal = torch.from_numpy(d[:, 1:4].astype(np.float32)).to(dev)
    return _com_apply(batch, B, tr_sigma, normal)


class DeviceNoiser:
    """Noising on the device (csrc/noising.hip).  ``draws(step, keys)`` -> float64 [B,8] rows that depend on
    ``(seed, step, key)`` alone; ``tr_so3`` / ``com`` noise a batch from such rows (its own for ``step`` and
    ``noise_keys(batch)`` unless ``keys`` or ``draws`` are given; ``draws=`` overrides the generator, for tests and for
    replaying a recorded table).  Both return the batch with a new ``pos`` tensor and the attributes of the host
    functions; ``tr_so3`` also attaches ``rot_norm [B]``, the ``exp_score_norm`` look-up the loss divides by.  Nothing is
    read back to the host.  ``tables``: needed by ``tr_so3`` only (default: the shared tables, loaded on first use)."""

    def __init__(self, params: dict, tables: Igso3Tables = None, device="cuda:0", seed: int = 0) -> None:
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs a ROCm device (the HIP path has no CPU fallback)")
        from . import lib as _lib

        self._lib = _lib
        self.lib = _lib.load()
        self.params = dict(params)
        self.tables = tables
        self.seed = int(seed)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def draws(self, step: int, keys) -> torch.Tensor:
        keys = torch.as_tensor(keys).reshape(-1)
        if keys.dtype != torch.int64:
            raise ValueError(f"keys: int64 expected, got {keys.dtype}")
        keys = keys.to(self.dev).contiguous()
        B = int(keys.numel())
        out = torch.empty(B, 8, dtype=torch.float64, device=self.dev)
        seed = self.seed & 0xFFFFFFFFFFFFFFFF
        seed = seed - (1 << 64) if seed >= (1 << 63) else seed
        with torch.cuda.device(self.dev):
            self._lib.check(self.lib.adf_noise_draws(seed, int(step) & 0x7FFFFFFF, keys.data_ptr(), B, out.data_ptr(),
                                                     self._stream()))
        return out

    def _inputs(self, batch, step, keys, draws):
        from .evaluator import atom_offsets

        if getattr(batch, "tags", None) is None:
            raise ValueError("batch.tags is required (tag 2 marks the adsorbate)")
        B, N = int(batch.natoms.numel()), int(batch.pos.shape[0])
        if draws is None:
            if step is None:
                raise ValueError("step= or draws= is required")
            draws = self.draws(step, noise_keys(batch) if keys is None else keys)
        elif not torch.is_tensor(draws):
            draws = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float64))
        draws = draws.to(self.dev, torch.float64).contiguous()
        if tuple(draws.shape) != (B, 8):
            raise ValueError(f"draws: [{B}, 8] expected, got {list(draws.shape)}")
        pos = batch.pos.to(self.dev, torch.float32).contiguous()
        cell = batch.cell.to(self.dev, torch.float32).reshape(B, 9).contiguous()
        tags = batch.tags.to(self.dev, torch.int32).contiguous()
        return B, N, draws, pos, cell, tags, atom_offsets(batch.natoms, self.dev)

    @torch.no_grad()
    def tr_so3(self, batch, step: int = None, keys=None, draws=None):
        if self.tables is None:
            self.tables = Igso3Tables.shared()
        tb = self.tables.on_device(self.dev)
        if "cdf" not in tb or "score" not in tb:
            raise ValueError("DeviceNoiser.tr_so3 needs the full IGSO(3) tables (cdf and score)")
        B, N, draws, pos, cell, tags, off = self._inputs(batch, step, keys, draws)
        p = self.params
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = torch.empty(N, 3, **f32)
        per = torch.empty(3, B, **f32)       # tr_sigma, rot_sigma, rot_norm
        vecs = torch.empty(3, B, 3, **f32)   # tr_score, rot_score, ads_center_noise_vec
        with torch.cuda.device(self.dev):
            self._lib.check(self.lib.adf_noise_tr_so3(
                pos.data_ptr(), cell.data_ptr(), tags.data_ptr(), off.data_ptr(), B, N, draws.data_ptr(),
                C.c_float(p["ads_std_low"]), C.c_float(p["ads_std_high"]), C.c_float(p["rot_std_low"]),
                C.c_float(p["rot_std_high"]), tb["omegas"].data_ptr(), tb["cdf"].data_ptr(), tb["score"].data_ptr(),
                tb["exp_score_norm"].data_ptr(), int(tb["cdf"].shape[0]), int(tb["cdf"].shape[1]), out.data_ptr(),
                per[0].data_ptr(), per[1].data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(), vecs[2].data_ptr(),
                per[2].data_ptr(), self._stream()))
        batch.pos = out
        batch.tr_sigma, batch.rot_sigma, batch.rot_norm = per[0][:, None], per[1][:, None], per[2]
        batch.tr_score, batch.rot_score, batch.ads_center_noise_vec = vecs[0], vecs[1], vecs[2]
        return batch

    @torch.no_grad()
    def com(self, batch, step: int = None, keys=None, draws=None):
        B, N, draws, pos, cell, tags, off = self._inputs(batch, step, keys, draws)
        p = self.params
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = torch.empty(N, 3, **f32)
        tr_sigma = torch.empty(B, **f32)
        vecs = torch.empty(2, B, 3, **f32)   # tr_score, ads_center_noise_vec
        with torch.cuda.device(self.dev):
            self._lib.check(self.lib.adf_noise_com(
                pos.data_ptr(), cell.data_ptr(), tags.data_ptr(), off.data_ptr(), B, N, draws.data_ptr(),
                C.c_float(p["ads_std_low"]), C.c_float(p["ads_std_high"]), out.data_ptr(), tr_sigma.data_ptr(),
                vecs[0].data_ptr(), vecs[1].data_ptr(), self._stream()))
        batch.pos = out
        batch.tr_sigma = tr_sigma[:, None]
        batch.tr_score, batch.ads_center_noise_vec = vecs[0], vecs[1]
        return batch

    def score_norm(self, rot_sigma: torch.Tensor, tables: Igso3Tables = None) -> torch.Tensor:
        """``Igso3Tables.score_norm`` of device sigmas without a host read (for batches that arrive already noised)."""
        return device_score_norm(rot_sigma, tables or self.tables or Igso3Tables.shared(), self.dev)


def device_score_norm(rot_sigma: torch.Tensor, tables: Igso3Tables, device) -> torch.Tensor:
    """float32 [B]: ``tables.exp_score_norm[eps_index(rot_sigma)]`` looked up on the device (adf_igso3_score_norm)."""
    from . import lib as _lib

    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("device_score_norm needs a ROCm device (the HIP path has no CPU fallback)")
    lib = _lib.load()
    table = tables.on_device(device)["exp_score_norm"]
    sig = rot_sigma.detach().to(device, torch.float32).reshape(-1).contiguous()
    out = torch.empty(sig.numel(), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.adf_igso3_score_norm(sig.data_ptr(), table.data_ptr(), int(table.numel()), int(sig.numel()),
                                            out.data_ptr(), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    return out
