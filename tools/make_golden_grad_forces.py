"""TEST INFRASTRUCTURE - generate tests/golden/grad_forces.npz and relax_grad_run.npz by running the REAL reference S2EF
PaiNN (adsorbdiff/models/painn/painn.py) on CPU and differentiating its energy with torch.autograd.  Run in the build
container only (needs the reference sources on the import path, as tools/make_golden_relax.py does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_grad_forces.py

The golden forces are F = -d(energy.sum())/d(pos) in FLOAT64 with the edge set held fixed.  The reference module does not
run in float64 as it stands (its graph code mixes dtypes); it does with torch.set_default_dtype(torch.float64),
model.double(), double pos / cell and the graph built once in float32 by the reference's own radius_graph_pbc and passed in
with otf_graph=False.  Every case also records what the reference's own float32 autograd gives against that (the floor of
the arithmetic: ``*_err32`` relative to max|F|, ``*_net32`` the largest net force of a system relative to max|F|).
Weights are NOT stored: models are drawn from a seed, the mirror class draws the same (checked by per-tensor sums).

  grad_forces.npz
    small_*   (a) H=128, 2 layers, 4 systems of 36+4 atoms; plus the reference's symmetrised edge list (tests pin the
                  float64 oracle of tests/helpers_grad_forces.py on it) and a float64 central difference along a random
                  direction at h = 1e-4 (asserted here to agree with the gradient to 1e-7: the golden is a true gradient)
    full_*    (b) the OC20 width (H=512, 6 layers, 128 rbf, cutoff 12, K=50), 2 systems of 64+4 atoms
    nohead_*  (c) a model built with regress_forces=False (no force head), another seed
    ragged_*  (d) systems of 36+4, 7+1 (a single adsorbate atom), 61+3, 20+2 atoms
    dir_*     (e) directional derivative at h = 1e-2 for a model whose max_neighbors never binds (asserted: the edge sets
                  at pos, pos + h v, pos - h v differ at most by edges within h of the cutoff, where the envelope and its
                  derivative vanish): the float64 central difference and the same difference from the float32 reference
  relax_grad_run.npz
    a free-running reference LBFGS.run of 4 small systems driven by the reference's float32 autograd forces, fmax chosen
    with the 1e-3 margin rule of relax_run.npz.  Fairness of the target (asserted): the same run from positions perturbed
    by 1e-6 A ends within 2.5e-5 A of it with equal masks.  FAIR_TRIES lists what is tried, in order; the first entry
    (the relax fixtures' max_neighbors = 20, up to 10 iterations, seed 78) passed: the perturbed run ends 1.9e-6 A away.
    The random-weight gradient forces are large (max|F| about 12), so the run converges in 3 iterations at fmax 7.26.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from tools.make_golden_relax import (GOLD, HP_FULL, HP_SMALL, SCALES_FULL, SCALES_SMALL, SEED_FULL, SEED_SMALL,  # noqa: E402
                                     batch_arrays, run_ref, write_npz)

SEED_NOHEAD = 5
RAGGED = ((36, 4), (7, 1), (61, 3), (20, 2))
DIR_K = 128          # the handle's largest max_neighbors; asserted below never to bind on the (e) batch
DIR_H = 1e-2
# relaxation target: what made the run a fair one (see the docstring); set by trying in this order
FAIR_TRIES = (dict(K=20, steps=10, seed=78), dict(K=20, steps=6, seed=78), dict(K=128, steps=10, seed=78),
              dict(K=128, steps=6, seed=78), dict(K=128, steps=6, seed=79))


def main() -> None:
    from oracle import refshim

    refshim.install()
    import adsorbdiff.relaxation.optimizers.lbfgs_torch as ref_lb
    from adsorbdiff.models.painn.painn import PaiNN as RefS2EF
    from adsorbdiff.utils.utils import radius_graph_pbc

    from adsorbdiff_amd.data import Batch
    from adsorbdiff_amd.painn import PaiNN as Mirror
    from adsorbdiff_amd.synthetic import make_batch, make_system

    torch.set_num_threads(8)

    def attach(b, bt, hp):
        """the float32 graph of ``bt`` (reference's own radius_graph_pbc) attached to ``b``"""
        dd = torch.get_default_dtype()
        torch.set_default_dtype(torch.float32)
        ei, co, nb = radius_graph_pbc(bt.clone(), hp["cutoff"], hp["max_neighbors"], True)
        torch.set_default_dtype(dd)
        b.edge_index, b.cell_offsets, b.neighbors = ei, co.to(b.pos.dtype), nb
        return ei, co

    def energy_grad(model, bt, hp, dtype, pos=None, graph_of=None, capture=None):
        """(energy, -dE/dpos) of the reference in ``dtype``; float64: fixed float32 graph of ``graph_of`` (default bt)"""
        b = bt.clone()
        if dtype == torch.float64:
            attach(b, graph_of if graph_of is not None else bt, hp)
            model.otf_graph = False
        else:
            model.otf_graph = True
        b.pos = (bt.pos if pos is None else pos).to(dtype).clone().requires_grad_(True)
        b.cell = b.cell.to(dtype)
        if capture is not None:
            orig = model.generate_graph_values

            def rec(data):
                out = orig(data)
                capture["edge_index"], capture["dist"], capture["unit"] = out[0].clone(), out[2].detach().clone(), out[3].detach().clone()
                return out

            model.generate_graph_values = rec
        try:
            with torch.enable_grad():
                e = model(b)["energy"]
                (g,) = torch.autograd.grad(e.sum(), b.pos)
        finally:
            if capture is not None:
                del model.generate_graph_values
        return e.detach(), -g.detach()

    def build(hp, scales, seed, **kw):
        torch.manual_seed(seed)
        ref = RefS2EF(None, 50, 1, scale_file=dict(scales), **hp, **kw).eval()
        torch.manual_seed(seed)
        mir = Mirror(None, 50, 1, scale_file=dict(scales), **hp, **kw)
        sd_r, sd_m = ref.state_dict(), mir.state_dict()
        assert list(sd_r) == list(sd_m) and all(torch.equal(sd_r[k], sd_m[k]) for k in sd_r), "the mirror draws other weights"
        return ref

    def case(tag, ref, bt, hp, seed, capture=None):
        B = int(bt.natoms.shape[0])
        e32, f32 = energy_grad(ref, bt, hp, torch.float32)
        sums = np.array([float(v.double().sum()) for v in ref.state_dict().values()], dtype=np.float64)
        torch.set_default_dtype(torch.float64)
        ref.double()
        try:
            e64, f64 = energy_grad(ref, bt, hp, torch.float64, capture=capture)
        finally:
            ref.float()
            torch.set_default_dtype(torch.float32)
        fmaxv = float(f64.abs().max())
        err32 = float((f32.double() - f64).abs().max()) / fmaxv
        net32 = float(torch.zeros(B, 3).index_add_(0, bt.batch, f32).abs().max()) / fmaxv
        net64 = float(torch.zeros(B, 3, dtype=torch.float64).index_add_(0, bt.batch, f64).abs().max()) / fmaxv
        print(f"[{tag}] E {e64.tolist()}  max|F| {fmaxv:.4f}  f32-vs-f64 {err32:.2e}  net32 {net32:.2e}  net64 {net64:.2e}")
        assert net64 < 1e-12 and err32 < 2e-5
        return {f"{tag}_energy": e64, f"{tag}_forces": f64, f"{tag}_err32": err32, f"{tag}_net32": net32,
                f"{tag}_energy32": e32, f"{tag}_seed": seed, f"{tag}_sums": sums, **batch_arrays(bt, f"{tag}_")}

    fx = {}
    # ------------------------------------------------------------------------------------------------ (a) small
    bt = make_batch(4, n_slab=36, n_ads=4, seed=71)
    ref = build(HP_SMALL, SCALES_SMALL, SEED_SMALL)
    cap = {}
    fx.update(case("small", ref, bt, HP_SMALL, SEED_SMALL, capture=cap))
    src, dst = cap["edge_index"]
    vec = cap["unit"] * cap["dist"][:, None]                       # float64, target -> source
    off = vec - (bt.pos.double()[src] - bt.pos.double()[dst])
    cell_e = bt.cell.double()[bt.batch[dst]]
    shifts = torch.linalg.solve(cell_e.transpose(1, 2), off.unsqueeze(-1)).squeeze(-1)
    assert float((shifts - shifts.round()).abs().max()) < 1e-6
    fx.update(small_edge_src=src.to(torch.int32), small_edge_dst=dst.to(torch.int32), small_edge_shift=shifts.round().to(torch.int8))
    # the golden is a true gradient: float64 central difference along a random unit direction
    g = torch.Generator().manual_seed(5)
    v = torch.randn(bt.pos.shape, generator=g, dtype=torch.float64)
    v /= v.norm()
    torch.set_default_dtype(torch.float64)
    ref.double()
    p0 = bt.pos.double()
    ep = energy_grad(ref, bt, HP_SMALL, torch.float64, pos=p0 + 1e-4 * v)[0].sum()
    em = energy_grad(ref, bt, HP_SMALL, torch.float64, pos=p0 - 1e-4 * v)[0].sum()
    ref.float()
    torch.set_default_dtype(torch.float32)
    fd = float((ep - em) / 2e-4)
    ana = float(-(torch.as_tensor(fx["small_forces"]) * v).sum())
    print(f"[small] central difference {fd:.10e}  -F.v {ana:.10e}  rel {abs(fd - ana) / abs(ana):.2e}")
    assert abs(fd - ana) / abs(ana) < 1e-7
    fx.update(small_fd_v=v, small_fd_h=1e-4, small_fd=fd)
    model_small = ref

    # ------------------------------------------------------------------------------------------------ (b) full width
    fx.update(case("full", build(HP_FULL, SCALES_FULL, SEED_FULL), make_batch(2, n_slab=64, n_ads=4, seed=72), HP_FULL, SEED_FULL))
    # ------------------------------------------------------------------------------------------------ (c) no force head
    fx.update(case("nohead", build(HP_SMALL, SCALES_SMALL, SEED_NOHEAD, regress_forces=False), bt, HP_SMALL, SEED_NOHEAD))
    # ------------------------------------------------------------------------------------------------ (d) ragged
    g = torch.Generator().manual_seed(4242)
    rag = Batch.from_data_list([make_system(g, ns, na, sid=str(i)) for i, (ns, na) in enumerate(RAGGED)])
    fx.update(case("ragged", model_small, rag, HP_SMALL, SEED_SMALL))

    # ------------------------------------------------------------------------------------------------ (e) directional
    hp_dir = dict(HP_SMALL, max_neighbors=DIR_K)
    ref = build(hp_dir, SCALES_SMALL, SEED_SMALL)
    p0 = bt.pos.double()
    sets, dists = [], []
    for sgn in (0, 1, -1):
        bb = bt.clone()
        bb.pos = (p0 + sgn * DIR_H * v).float()
        ei, co, nb = radius_graph_pbc(bb, hp_dir["cutoff"], DIR_K, True)
        assert int(torch.bincount(ei[1]).max()) < DIR_K, "max_neighbors binds: choose a larger one"
        sets.append(set(map(tuple, torch.cat([ei.t(), co.long()], 1).tolist())))
    cell_of = bt.cell.double()[bt.batch]
    for s_ in sets[1:]:
        for (j, i, a, b_, c) in sets[0] ^ s_:   # edges that appear / disappear: within h of the cutoff at the base positions
            d0 = float((p0[j] - p0[i] + torch.tensor([a, b_, c], dtype=torch.float64) @ cell_of[i]).norm())
            assert abs(d0 - hp_dir["cutoff"]) < 2.1 * DIR_H, d0
    print(f"[dir] edges {len(sets[0])}, changed +h {len(sets[0] ^ sets[1])}, -h {len(sets[0] ^ sets[2])} (all at the cutoff)")

    def e_sum(model, pos, dtype, graph_pos):
        gb = bt.clone()
        gb.pos = graph_pos.float()
        with torch.no_grad():
            b = bt.clone()
            if dtype == torch.float64:
                attach(b, gb, hp_dir)
                model.otf_graph = False
            else:
                model.otf_graph = True
            b.pos, b.cell = pos.to(dtype), b.cell.to(dtype)
            return model(b)["energy"].double().sum()

    fd32 = float((e_sum(ref, p0 + DIR_H * v, torch.float32, p0) - e_sum(ref, p0 - DIR_H * v, torch.float32, p0)) / (2 * DIR_H))   # (graph on the fly)
    torch.set_default_dtype(torch.float64)
    ref.double()
    # float64: each displaced evaluation on the float32 graph of its own displaced positions (what a forward there builds)
    fd64 = float((e_sum(ref, p0 + DIR_H * v, torch.float64, p0 + DIR_H * v) - e_sum(ref, p0 - DIR_H * v, torch.float64, p0 - DIR_H * v)) / (2 * DIR_H))
    _, f64 = energy_grad(ref, bt, hp_dir, torch.float64)
    ref.float()
    torch.set_default_dtype(torch.float32)
    ana = float(-(f64 * v).sum())
    dev32 = abs(fd32 - fd64) / abs(fd64)
    print(f"[dir] h {DIR_H}: fd64 {fd64:.8e}  fd32 {fd32:.8e} (dev {dev32:.2e})  -F64.v {ana:.8e} (truncation {abs(ana - fd64) / abs(fd64):.2e})")
    fx.update(dir_v=v, dir_h=DIR_H, dir_fd64=fd64, dir_fd32=fd32, dir_dev32=dev32, dir_ana64=ana, dir_max_neighbors=DIR_K,
              dir_seed=SEED_SMALL, **batch_arrays(bt, "dir_"))
    write_npz(GOLD / "grad_forces.npz", fx)

    # ------------------------------------------------------------------------------------------------ relaxation run
    for tri in FAIR_TRIES:
        hp_run = dict(HP_SMALL, max_neighbors=tri["K"])
        ref = build(hp_run, SCALES_SMALL, SEED_SMALL)
        ref.otf_graph = True
        btr = make_batch(4, n_slab=20, n_ads=4, seed=tri["seed"])

        def painn(b_):
            bb = b_.clone()
            bb.pos = b_.pos.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                e = ref(bb)["energy"]
                (gr,) = torch.autograd.grad(e.sum(), bb.pos)
            return e.detach(), -gr.detach()

        steps = tri["steps"]
        mf0 = run_ref(ref_lb, btr.clone(), painn, 1e-12, 2, memory=50)["max_force"][0].sort().values.tolist()
        cands = [round(a + (b_ - a) * t, 6) for a, b_ in zip(mf0[:-1], mf0[1:]) for t in (0.5, 0.3, 0.7, 0.9)]
        cands += [round(mf0[0] * t, 6) for t in (0.7, 0.5, 0.3)]
        chosen = None
        for fmax in cands:
            res = run_ref(ref_lb, btr.clone(), painn, fmax, steps, memory=50)
            if res["margin"] > 1e-3 and res["masks"][0].any():
                pert = btr.clone()
                gp = torch.Generator().manual_seed(80)
                pert.pos = pert.pos + 1e-6 * torch.nn.functional.normalize(torch.randn(pert.pos.shape, generator=gp), dim=1)
                pert.pos[btr.fixed == 1] = btr.pos[btr.fixed == 1]
                res2 = run_ref(ref_lb, pert, painn, fmax, steps, memory=50)
                dev = float((res2["pos_final"] - res["pos_final"]).abs().max())
                same = res2["masks"].shape == res["masks"].shape and bool(torch.equal(res2["masks"], res["masks"]))
                print(f"[run] {tri} fmax {fmax}: iterations {res['iterations']}, margin {res['margin']:.2e}, "
                      f"perturbed run deviates {dev:.2e} A, masks equal {same}")
                if dev < 2.5e-5 and same:
                    chosen = (fmax, res)
                    break
        if chosen:
            break
    else:
        raise SystemExit("no fair relaxation target found")
    fmax, res = chosen
    print(f"[run] kept {tri}: fmax {fmax}, masks {res['masks'].int().tolist()}")
    write_npz(GOLD / "relax_grad_run.npz", dict(fmax=fmax, steps=tri["steps"], memory=50, seed=SEED_SMALL,
                                                 max_neighbors=tri["K"],
                                                 **{k: v for k, v in res.items() if k not in ("margin", "pos_log")},
                                                 **batch_arrays(btr)))


if __name__ == "__main__":
    main()
