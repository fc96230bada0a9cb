"""Numpy restatement of the sampler's keyed draws (csrc/noising.hip: adf_sampler_draws; contract in
include/adsorbdiff_hip.h and DESIGN.md 4i) on top of tests/helpers_tr_only.philox4x32_10, and the literal re-enactment of
the reference's early-stop loop for one system (tests/test_sampler_per_system_host.py, tests/test_gpu_sampler_per_system.py).
"""
import numpy as np

from tests.helpers_tr_only import philox4x32_10

PLACE_ROW = 0xFFFFFFFF


def _words(seed: int, keys, site, t: int, j: int) -> np.ndarray:
    """uint32 [B,4]: Philox4x32-10, key (seed lo, seed hi), counter (key lo, key hi, t, 4 + 2 site + j)."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1).view(np.uint64)
    B = keys.shape[0]
    site = np.zeros(B, np.uint64) if site is None else np.asarray(site, dtype=np.int64).reshape(-1).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (B, 2))
    ctr = np.stack([keys & np.uint64(0xFFFFFFFF), keys >> np.uint64(32), np.full(B, int(t) & 0xFFFFFFFF, np.uint64),
                    np.uint64(4) + np.uint64(2) * site + np.uint64(j)], axis=-1)
    return philox4x32_10(ctr, key)


def place_draws(seed: int, keys, site=None) -> np.ndarray:
    """float32 [B,3]: (w_k >> 8) 2^-24 of the placement row (t = 0xFFFFFFFF, j = 0)."""
    w = _words(seed, keys, site, PLACE_ROW, 0)[:, :3]
    return ((w >> np.uint32(8)).astype(np.float64) * 2.0**-24).astype(np.float32)


def step_normals(seed: int, keys, site, T: int) -> np.ndarray:
    """float64 [T,B,6]: Box-Muller in double on (w0,w1), (w2,w3), (w4,w5) of every step row, BEFORE the cast to float32:
    z_a = float32(out[..., :3]), z_b = float32(out[..., 3:])."""
    B = np.asarray(keys).reshape(-1).shape[0]
    out = np.empty((T, B, 6))
    for t in range(T):
        w = np.concatenate([_words(seed, keys, site, t, 0), _words(seed, keys, site, t, 1)], axis=-1)
        u = (w.astype(np.float64) + 0.5) * 2.0**-32
        for p in range(3):
            r = np.sqrt(-2.0 * np.log(u[:, 2 * p]))
            ph = 2.0 * np.pi * u[:, 2 * p + 1]
            out[t, :, 2 * p], out[t, :, 2 * p + 1] = r * np.cos(ph), r * np.sin(ph)
    return out


def reference_loop_one_system(conv_column, count: int = 10):
    """The reference's loop (denoising_torch.py:296-356) for ONE system, step by step as it is written there: the
    cumulative counter, the ``break`` before the update, the update otherwise.  -> (steps_applied, stop_step)."""
    cvg_count, applied = 0, 0
    for t, conv in enumerate(conv_column):
        if conv:
            cvg_count += 1
            if count > 0 and cvg_count == count:
                return applied, t
        applied += 1
    return applied, -1
