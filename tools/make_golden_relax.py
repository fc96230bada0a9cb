"""TEST INFRASTRUCTURE - generate tests/golden/relax_*.npz by running the REAL reference S2EF PaiNN
(adsorbdiff/models/painn/painn.py) and L-BFGS (adsorbdiff/relaxation/optimizers/lbfgs_torch.py) on CPU.  Run in the build
container only (needs the reference sources on the import path, as oracle/make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_relax.py

Weights are NOT stored: both models are drawn from a seed (the mirror class draws the same weights, checked here and by
the tests through the recorded per-tensor sums).  Fixtures:

  relax_painn.npz     (a) energies and forces of the small model (H=128, 2 layers, the stepper fixtures' shape) and of
                          the OC20 width (H=512, 6 layers, 128 rbf, cutoff 12, K=50); the small batch holds one pair of
                          atoms 5e-4 A apart; the state_dict key list with shapes and per-tensor sums
  relax_teacher.npz   (b) reference LBFGS.step called directly on a scripted force sequence: memory 5 over 20 iterations
                          (the ring wraps), fixed atoms, a near-zero-force iteration that takes the skip path; the same
                          with early_stop_batch=True
  relax_harmonic.npz  (c) free-running reference relaxation with an analytic harmonic calculator F = -k (x - x*) in f32
  relax_run.npz       (d) free-running reference relaxation of 4 systems with the small S2EF PaiNN; fmax keeps a margin
                          of 1e-3 relative from every system's max force at every iteration (asserted)

(c) and (d) drive LBFGS.run through the reference's TorchCalc, exactly what ml_relax does for a batch that fits.  The
archives are written with fixed zip metadata, so two runs give identical bytes.
"""
from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

GOLD = ROOT / "tests" / "golden"
HP_SMALL = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES_SMALL = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
HP_FULL = dict(hidden_channels=512, num_layers=6, num_rbf=128, cutoff=12.0, max_neighbors=50)
SCALES_FULL = {f"upd_out_scalar_scale_{i}": 1.0 - 0.04 * i for i in range(6)}
SEED_SMALL, SEED_FULL = 3, 4


def write_npz(path: Path, arrays: dict) -> None:
    """np.savez_compressed with a fixed member timestamp (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            v = arrays[k]
            v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            np.lib.format.write_array(buf, v, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print("written", path, path.stat().st_size, "bytes")


def batch_arrays(b, prefix=""):
    return {prefix + k: getattr(b, k) for k in ("pos", "atomic_numbers", "tags", "fixed", "cell", "natoms", "batch")}


def close_pair_batch():
    """4 small systems; in system 1 the last adsorbate atom sits 5e-4 A from the one before it."""
    from adsorbdiff_amd.synthetic import make_batch

    b = make_batch(4, n_slab=36, n_ads=4, seed=71)
    a1 = int(b.natoms[:2].sum()) - 1
    b.pos[a1] = b.pos[a1 - 1] + torch.tensor([5e-4, 0.0, 0.0])
    return b


class Predictor:
    """What TorchCalc touches on a trainer: predict(batch) -> {"energy", "forces"}; logs every call's positions."""

    def __init__(self, fn, model=None):
        self.fn = fn
        self._unwrapped_model = model if model is not None else type("M", (), {"otf_graph": True})()
        self.pos_log = []

    @torch.no_grad()
    def predict(self, batch, per_image=False, disable_tqdm=True):
        self.pos_log.append(batch.pos.clone())
        e, f = self.fn(batch)
        return {"energy": e, "forces": f}


def seg_max_force(forces, batch, B):
    """check_convergence's per-system max |f| (lbfgs_torch.py:75-77), f64."""
    f = forces.to(torch.float64)
    n = (f ** 2).sum(axis=1).sqrt()
    return torch.zeros(B, dtype=torch.float64).scatter_reduce_(0, batch, n, "amax", include_self=False)


def main() -> None:
    from oracle import refshim

    refshim.install()
    import adsorbdiff.relaxation.optimizers.lbfgs_torch as ref_lb
    from adsorbdiff.models.painn.painn import PaiNN as RefS2EF

    from adsorbdiff_amd.painn import PaiNN as Mirror
    from adsorbdiff_amd.synthetic import make_batch

    torch.set_num_threads(8)

    # ------------------------------------------------------------------------------------------------ (a) model outputs
    fx = {}
    for tag, hp, sc, seed, bt in (("small", HP_SMALL, SCALES_SMALL, SEED_SMALL, close_pair_batch()),
                                  ("full", HP_FULL, SCALES_FULL, SEED_FULL, make_batch(2, n_slab=64, n_ads=4, seed=72))):
        torch.manual_seed(seed)
        ref = RefS2EF(None, 50, 1, scale_file=dict(sc), **hp).eval()
        torch.manual_seed(seed)
        mir = Mirror(None, 50, 1, scale_file=dict(sc), **hp)
        sd_r, sd_m = ref.state_dict(), mir.state_dict()
        assert list(sd_r) == list(sd_m), "key order"
        assert all(torch.equal(sd_r[k], sd_m[k]) for k in sd_r), "the mirror does not draw the reference's weights"
        with torch.no_grad():
            out = ref(bt.clone())
        fx.update({f"{tag}_energy": out["energy"], f"{tag}_forces": out["forces"], f"{tag}_seed": seed,
                   **batch_arrays(bt, f"{tag}_")})
        fx[f"{tag}_keys"] = np.array([k.encode() for k in sd_r], dtype="S")
        fx[f"{tag}_shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd_r.values()], dtype=np.int64)
        fx[f"{tag}_sums"] = np.array([float(v.double().sum()) for v in sd_r.values()], dtype=np.float64)
        print(f"[a:{tag}] energy {out['energy'].tolist()}  |f|max {float(out['forces'].abs().max()):.3e}")
        if tag == "small":
            model_small = ref
    write_npz(GOLD / "relax_painn.npz", fx)

    # ------------------------------------------------------------------------------------------------ (b) teacher-forced
    fx = {}
    for tag, early, K, skip_at in (("ring", False, 20, 12), ("early", True, 8, None)):
        bt = make_batch(3, n_slab=9, n_ads=3, seed=73)
        N, B = bt.pos.shape[0], 3
        g = torch.Generator().manual_seed(74 if tag == "ring" else 75)
        base = torch.randn(N, 3, generator=g)
        sys_scale = torch.tensor([1.0, 0.3, 0.06])[bt.batch].reshape(-1, 1)
        forces, fmax = [], 0.2
        for k in range(K):
            f = (base * 0.9 ** k + 0.3 * torch.randn(N, 3, generator=g)) * sys_scale
            if k == skip_at:
                f = f * 1e-12
            f[bt.fixed == 1] = 0
            forces.append(f.float())
        pred = Predictor(lambda b_: (torch.zeros(B), torch.zeros_like(b_.pos)))
        opt = ref_lb.LBFGS(bt, ref_lb.TorchCalc(pred), maxstep=0.04, memory=5, damping=1.0, alpha=70.0, device="cpu",
                           early_stop_batch=early)
        opt.fmax = fmax
        from collections import deque
        opt.s, opt.y, opt.rho = deque(maxlen=5), deque(maxlen=5), deque(maxlen=5)
        opt.r0 = opt.f0 = None
        pos_in = bt.pos.clone()
        pos_after, masks, skipped, mf = [], [], [], []
        for k in range(K):
            f64 = forces[k].to(torch.float64)
            mfk = seg_max_force(forces[k], bt.batch, B)
            margin = ((mfk - fmax).abs() / fmax).min()
            assert margin > 1e-3, (tag, k, margin)
            mask = mfk[bt.batch].ge(fmax)
            r0_before = None if opt.r0 is None else opt.r0.clone()
            p0 = bt.pos.clone()
            opt.step(k, f64, mask)
            skip = torch.equal(bt.pos, p0) and (r0_before is not None and torch.equal(opt.r0, r0_before))
            pos_after.append(bt.pos.clone())
            masks.append(mfk.ge(fmax))
            skipped.append(skip)
            mf.append(mfk)
        if skip_at is not None:
            assert skipped[skip_at] and sum(skipped) == 1, skipped
        assert any(not m.all() for m in masks) and any(m.any() for m in masks)
        print(f"[b:{tag}] skipped at {[i for i, s in enumerate(skipped) if s]}, masks {[m.int().tolist() for m in masks][:4]}...")
        fx.update({f"{tag}_pos_in": pos_in, f"{tag}_forces": torch.stack(forces), f"{tag}_pos_after": torch.stack(pos_after),
                   f"{tag}_masks": torch.stack(masks), f"{tag}_skipped": np.array(skipped), f"{tag}_max_force": torch.stack(mf),
                   f"{tag}_early": int(early), f"{tag}_fmax": fmax, f"{tag}_memory": 5, f"{tag}_maxstep": 0.04,
                   f"{tag}_damping": 1.0, f"{tag}_alpha": 70.0, **batch_arrays(bt, f"{tag}_")})
    write_npz(GOLD / "relax_teacher.npz", fx)

    # ------------------------------------------------------------------------------------------------ (c) harmonic
    bt = make_batch(3, n_slab=9, n_ads=3, seed=76)
    N, B = bt.pos.shape[0], 3
    g = torch.Generator().manual_seed(77)
    xstar = (bt.pos + 0.3 * torch.randn(N, 3, generator=g)).float()
    kk = torch.tensor([2.0, 5.0, 9.0])[bt.batch].reshape(-1, 1).float()

    def harmonic(b_):
        d = b_.pos - xstar
        f = -kk * d
        e = torch.zeros(B).index_add_(0, b_.batch, (0.5 * kk * d * d).sum(1))
        return e, f

    fmax_h, steps_h = 0.05, 60
    res = run_ref(ref_lb, bt, harmonic, fmax_h, steps_h, memory=10)
    assert res["margin"] > 1e-3, res["margin"]
    print(f"[c] iterations {res['iterations']}, final max forces {res['max_force'][-1].tolist()}")
    write_npz(GOLD / "relax_harmonic.npz", dict(xstar=xstar, k=torch.tensor([2.0, 5.0, 9.0]), fmax=fmax_h, steps=steps_h,
                                                memory=10, **{k: v for k, v in res.items() if k != "margin"},
                                                **batch_arrays(bt)))

    # ------------------------------------------------------------------------------------------------ (d) PaiNN run
    bt = make_batch(4, n_slab=20, n_ads=4, seed=78)

    def painn(b_):
        with torch.no_grad():
            o = model_small(b_.clone())
        return o["energy"], o["forces"]

    steps_d = 10
    # candidates between the systems' initial max forces (the random-init model's forces are ~1e-2 eV/A)
    mf0 = run_ref(ref_lb, bt.clone(), painn, 1e-12, 2, memory=50)["max_force"][0].sort().values.tolist()
    cands = [round(a + (b_ - a) * t, 6) for a, b_ in zip(mf0[:-1], mf0[1:]) for t in (0.5, 0.3, 0.7, 0.9)]
    for fmax_d in cands:
        res = run_ref(ref_lb, bt.clone(), painn, fmax_d, steps_d, memory=50)
        conv = res["masks"].logical_not().any()
        if res["margin"] > 1e-3 and conv and res["masks"][0].any():
            break
    else:
        raise SystemExit("no fmax with a margin found")
    print(f"[d] fmax {fmax_d}: iterations {res['iterations']}, margin {res['margin']:.3e}, "
          f"masks {res['masks'].int().tolist()}")
    write_npz(GOLD / "relax_run.npz", dict(fmax=fmax_d, steps=steps_d, memory=50, seed=SEED_SMALL,
                                           **{k: v for k, v in res.items() if k != "margin"}, **batch_arrays(bt)))


def run_ref(ref_lb, bt, fn, fmax, steps, memory):
    """Free-running reference LBFGS.run (what ml_relax runs for a batch that fits) with recording hooks."""
    pred = Predictor(fn)
    pos_in = bt.pos.clone()
    B = int(bt.natoms.shape[0])
    opt = ref_lb.LBFGS(bt, ref_lb.TorchCalc(pred), maxstep=0.04, memory=memory, damping=1.0, alpha=70.0, device="cpu")
    mf_log = []
    orig = opt.check_convergence

    def rec(iteration, forces=None, energy=None):
        m, e, f = orig(iteration, forces, energy)
        mf_log.append(seg_max_force(f, bt.batch, B))
        return m, e, f

    opt.check_convergence = rec
    out = opt.run(fmax=fmax, steps=steps)
    mf = torch.stack(mf_log)
    margin = float(((mf - fmax).abs() / fmax).min())
    return dict(pos_in=pos_in, pos_final=out.pos.clone(), y=out.y.clone(), force=out.force.clone(), max_force=mf,
                masks=mf.ge(fmax), iterations=len(mf_log), pos_log=torch.stack(pred.pos_log), margin=margin)


if __name__ == "__main__":
    main()
