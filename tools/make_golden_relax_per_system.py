"""TEST INFRASTRUCTURE - generate tests/golden/relax_per_system.npz: what the per-system L-BFGS mode must reproduce, recorded
by running the REAL reference L-BFGS (adsorbdiff/relaxation/optimizers/lbfgs_torch.py) on CPU on every system ALONE
(B = 1) over scripted forces.  Run in the build container only (needs the reference sources, as tools/make_golden_relax.py
does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_relax_per_system.py

A system's reference optimizer gets ``step(t_b, ...)`` only at the iterations where that system's update mask is set, with
its own step number t_b = 0, 1, 2, ...: a system whose mask is clear is left alone, as the per-system mode leaves it.
Cases (systems of 12, 7, 1 and 33 atoms, memory 5, 20 iterations, fixed atoms; the force recipe of make_golden_relax.py
(b) with per-system scales 1.0 / 0.3 / 1.0 / 0.12):

  ring   fmax 0.2: the rings wrap, one system converges early for good, one has its mask clear and then set again (all
         three asserted), every max force keeps a relative margin of 1e-3 from fmax (asserted)
  skip   fmax 1e-9, the forces of system 1 scaled by 1e-8 at iteration 12: exactly that system skips at that iteration
         while the others move in the same call (asserted) - what tells the per-system skip from the batch-global one

Recorded per case: inputs, forces [K, N, 3], positions after every iteration [K, N, 3], masks [K, B], the per-system skip
table [K, B], steps_taken [B].  Data only; written with fixed zip metadata, so two runs give identical bytes.
"""
from __future__ import annotations

import sys
from collections import deque
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from tools.make_golden_relax import GOLD, Predictor, batch_arrays, seg_max_force, write_npz  # noqa: E402

SIZES = ((9, 3), (5, 2), (0, 1), (29, 4))     # (slab, adsorbate) atoms: 12, 7, 1 and 33
SCALES = (1.0, 0.3, 1.0, 0.12)
MEMORY, K, SKIP_AT, SKIP_SYS = 5, 20, 12, 1
SEED_BATCH, SEED_FORCES = 81, {"ring": 82, "skip": 83}


def make_systems():
    from adsorbdiff_amd.data import Batch
    from adsorbdiff_amd.synthetic import make_system

    gen = torch.Generator().manual_seed(SEED_BATCH)
    return Batch.from_data_list([make_system(gen, ns, na, sid=str(i)) for i, (ns, na) in enumerate(SIZES)])


def scripted_forces(bt, tag):
    N = bt.pos.shape[0]
    g = torch.Generator().manual_seed(SEED_FORCES[tag])
    base = torch.randn(N, 3, generator=g)
    sys_scale = torch.tensor(SCALES)[bt.batch].reshape(-1, 1)
    forces = []
    for k in range(K):
        f = (base * 0.9 ** k + 0.3 * torch.randn(N, 3, generator=g)) * sys_scale
        if tag == "skip" and k == SKIP_AT:
            f = torch.where((bt.batch == SKIP_SYS).reshape(-1, 1), f * 1e-8, f)
        f[bt.fixed == 1] = 0
        forces.append(f.float())
    return forces


def main() -> None:
    from oracle import refshim

    refshim.install()
    import adsorbdiff.relaxation.optimizers.lbfgs_torch as ref_lb

    from adsorbdiff_amd.data import Batch

    torch.set_num_threads(8)
    fx = {}
    for tag, fmax in (("ring", 0.2), ("skip", 1e-9)):
        bt = make_systems()
        B = len(SIZES)
        forces = scripted_forces(bt, tag)
        offs = [0] + torch.cumsum(bt.natoms, 0).tolist()
        pos_in = bt.pos.clone()
        # one reference optimizer per system, each on a batch that holds that system alone
        singles, opts = [], []
        for d in bt.to_data_list():
            one = Batch.from_data_list([d])
            pred = Predictor(lambda b_: (torch.zeros(1), torch.zeros_like(b_.pos)))
            opt = ref_lb.LBFGS(one, ref_lb.TorchCalc(pred), maxstep=0.04, memory=MEMORY, damping=1.0, alpha=70.0,
                               device="cpu")
            opt.fmax = fmax
            opt.s, opt.y, opt.rho = deque(maxlen=MEMORY), deque(maxlen=MEMORY), deque(maxlen=MEMORY)
            opt.r0 = opt.f0 = None
            singles.append(one)
            opts.append(opt)
        t = [0] * B
        pos_after, masks, skipped, mf = [], [], [], []
        for k in range(K):
            mfk = seg_max_force(forces[k], bt.batch, B)
            margin = ((mfk - fmax).abs() / fmax).min()
            assert margin > 1e-3, (tag, k, float(margin))
            mk = mfk.ge(fmax)
            sk = [False] * B
            for b in range(B):
                if not bool(mk[b]):
                    continue
                one, opt = singles[b], opts[b]
                f64 = forces[k][offs[b]:offs[b + 1]].to(torch.float64)
                r0_before = None if opt.r0 is None else opt.r0.clone()
                p0 = one.pos.clone()
                opt.step(t[b], f64, torch.ones(one.pos.shape[0], dtype=torch.bool))
                t[b] += 1
                sk[b] = torch.equal(one.pos, p0) and r0_before is not None and torch.equal(opt.r0, r0_before)
            pos_after.append(torch.cat([one.pos for one in singles]).clone())
            masks.append(mk)
            skipped.append(sk)
            mf.append(mfk)
        masks_t, skipped_t = torch.stack(masks), torch.tensor(skipped)
        if tag == "ring":
            assert int(skipped_t.sum()) == 0, skipped_t.nonzero().tolist()
            assert max(t) >= MEMORY + 2, t                       # a ring wrapped: an entry was overwritten
            # set at first, and clear from some iteration of the first half through the end
            for_good = [b for b in range(B) if bool(masks_t[0, b]) and not bool(masks_t[K // 2:, b].any())]
            again = [b for b in range(B) if any((not bool(masks_t[k0, b])) and bool(masks_t[k0 + 1:, b].any())
                                                 for k0 in range(K - 1))]
            assert for_good, "no system converges early for good"
            assert again, "no system has its mask clear and then set again"
            print(f"[ring] steps_taken {t}; converged for good: {for_good}; clear then set again: {again}")
        else:
            assert skipped_t.nonzero().tolist() == [[SKIP_AT, SKIP_SYS]], skipped_t.nonzero().tolist()
            assert bool(masks_t.all())
            moved = [not torch.equal(pos_after[SKIP_AT][offs[b]:offs[b + 1]], pos_after[SKIP_AT - 1][offs[b]:offs[b + 1]])
                     for b in range(B)]
            assert moved == [b != SKIP_SYS for b in range(B)], moved
            print(f"[skip] steps_taken {t}; skipped {skipped_t.nonzero().tolist()}")
        bt.pos = pos_in
        fx.update({f"{tag}_pos_in": pos_in, f"{tag}_forces": torch.stack(forces), f"{tag}_pos_after": torch.stack(pos_after),
                   f"{tag}_masks": masks_t, f"{tag}_skipped": skipped_t, f"{tag}_max_force": torch.stack(mf),
                   f"{tag}_steps_taken": np.array(t, dtype=np.int32), f"{tag}_fmax": fmax, f"{tag}_memory": MEMORY,
                   f"{tag}_maxstep": 0.04, f"{tag}_damping": 1.0, f"{tag}_alpha": 70.0, **batch_arrays(bt, f"{tag}_")})
    write_npz(GOLD / "relax_per_system.npz", fx)


if __name__ == "__main__":
    main()
