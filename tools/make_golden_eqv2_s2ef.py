"""TEST INFRASTRUCTURE - generate tests/golden/eqv2_s2ef.npz and tests/golden/relax_eqv2_run.npz by running the REAL
reference EquiformerV2 S2EF model (adsorbdiff/models/equiformer_v2/equiformer_v2_oc20.py, class EquiformerV2_OC20) and
the reference L-BFGS (adsorbdiff/relaxation/optimizers/lbfgs_torch.py) on CPU.  Run in the build container only (needs
the reference sources on the import path, as oracle/make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_eqv2_s2ef.py

No weights are stored.  The small model is drawn from a seed (the mirror class consumes the generator as the reference
does and draws the same weights: asserted here, and by the tests through the recorded per-tensor sums); the full-width
model is refilled by tests/helpers.py::refill_parameters_by_name.  Both then get, from tests/helpers_s2ef.py::
trained_like: atom edge embeddings lifted to trained-like magnitudes, seeded non-zero values for the energy head's two
biases (zero in the reference's initialisation, which would hide them) and a seeded non-zero ``energy_lin_ref``.

eqv2_s2ef.npz
  small_*  C = 32, 2 blocks, L = 4 / M = 2, cutoff 6, K = 20 on 2 x 19 atoms: the reference's edge list, energies
           (``use_energy_lin_ref`` off and on), per-atom energies, forces, node embeddings after the edge-degree embedding
           and after every block, the state_dict key list with shapes and per-tensor sums.
  full_*   CFG4_KW without FOR_denoising, lmax_list=[4], cutoff 12, K = 20 on 2 x 40 atoms: the same outputs with the
           block embeddings as a strided sample plus per-degree norms (as eqv2_conditional_l4.npz stores them).
  Asserted per system: |E| >= 0.1 sum_i |e_i| / avg_num_nodes, so a relative bound on E is not a bound on cancellation
  noise.

relax_eqv2_run.npz
  A free-running reference relaxation (reference LBFGS.run through its TorchCalc) of 4 systems with the small model at
  cutoff 5.0 / K = 64.  A free run cannot inject an edge list, so the inputs must never truncate: asserted at every
  iteration that every atom has fewer than 64 neighbours inside the cutoff; fmax keeps a relative margin of 1e-3 from
  every system's max force at every iteration (asserted).

The archives are written with fixed zip metadata, so two runs give identical bytes.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

GOLD = ROOT / "tests" / "golden"
ATOM_STRIDE, CH_STRIDE = 9, 32


def record(eq, b, L, nl):
    """One reference forward with hooks: outputs, per-atom energies, block embeddings [nl + 1, N, S, C]."""
    rec = {}
    hooks = [eq.blocks[0].register_forward_pre_hook(lambda m_, a_: rec.__setitem__("x0", a_[0].embedding.detach().clone())),
             eq.energy_block.register_forward_hook(lambda m_, i_, o_: rec.__setitem__("e", o_.embedding.detach()[:, 0, 0].clone()))]
    for bi_, blk_ in enumerate(eq.blocks):
        hooks.append(blk_.register_forward_hook(lambda m_, i_, o_, bi_=bi_: rec.__setitem__(bi_, o_.embedding.detach().clone())))
    torch.manual_seed(1)   # the reference's random edge gauge (edge_rot_mat.py:21; it moves the outputs by < 1e-6 relative)
    with torch.no_grad():
        out = eq(b.clone())
    for h_ in hooks:
        h_.remove()
    xb = torch.stack([rec["x0"]] + [rec[i] for i in range(nl)])
    assert bool(torch.isfinite(out["forces"]).all()) and bool(torch.isfinite(xb).all())
    return out, rec["e"], xb


def check_mirror(ref, mir):
    rp, mp = dict(ref.named_parameters()), dict(mir.named_parameters())
    assert list(rp) == list(mp), "mirror parameter order differs from the reference's"
    assert all(tuple(rp[k].shape) == tuple(mp[k].shape) for k in rp)
    bad = [k for k in rp if not torch.equal(rp[k], mp[k])]
    assert not bad, ("mirror weights differ from the reference's", bad[:5])
    extra = [k for k in ref.state_dict() if k not in rp and not k.endswith(type(mir)._CONST_BUFFER_SUFFIXES)]
    assert not extra, ("reference buffers the mirror's load_state_dict would reject", extra[:5])


def model_case(tag, ref, mir, b, kw, fx):
    from tests.helpers_s2ef import energy_formula, tensor_sum

    L, nl = kw["lmax_list"][0], kw["num_layers"]
    check_mirror(ref, mir)
    gq = ref.generate_graph(b.clone(), enforce_max_neighbors_strictly=True)
    ref.use_energy_lin_ref = False
    out, e_atom, xb = record(ref, b, L, nl)
    ref.use_energy_lin_ref = True
    out_ref, _, _ = record(ref, b, L, nl)
    assert torch.equal(out["forces"], out_ref["forces"]) and not torch.equal(out["energy"], out_ref["energy"])
    # the formula the library implements (only the gating scalars reach the energy), on the reference's final embedding
    with torch.no_grad():
        xn = ref.norm(xb[-1])
    e_formula = energy_formula(ref.state_dict(), xn[:, 0, :])
    assert float((e_formula - e_atom).abs().max()) <= 1e-5 * float(e_atom.abs().max()), "energy head formula"
    B = int(b.natoms.shape[0])
    tot = torch.zeros(B).index_add_(0, b.batch, e_atom.abs()) / ref.avg_num_nodes
    assert bool((out["energy"].abs() >= 0.1 * tot).all()), (tag, out["energy"].tolist(), tot.tolist())
    sd = ref.state_dict()
    pn = [k for k, _ in ref.named_parameters()]
    fx.update({f"{tag}_{k}": getattr(b, k) for k in ("pos", "atomic_numbers", "tags", "fixed", "cell", "natoms", "batch")})
    fx.update({f"{tag}_edge_index": gq[0].to(torch.int32), f"{tag}_edge_vec": gq[2], f"{tag}_energy": out["energy"],
               f"{tag}_energy_lin_ref": out_ref["energy"], f"{tag}_forces": out["forces"], f"{tag}_atom_energy": e_atom,
               f"{tag}_keys": np.array([k.encode() for k in pn], dtype="S"),
               f"{tag}_shapes": np.array([",".join(map(str, sd[k].shape)) for k in pn], dtype="S"),
               f"{tag}_sums": np.array([tensor_sum(sd[k]) for k in pn], dtype=np.float64),
               f"{tag}_n_params": sum(p.numel() for p in ref.parameters())})
    print(f"[{tag}] E {out['energy'].tolist()} (+lin_ref {out_ref['energy'].tolist()}) sum|e_i|/avg {tot.tolist()} "
          f"|f|max {float(out['forces'].abs().max()):.4e}")
    return xb


def main() -> None:
    from oracle import refshim

    refshim.install()
    from oracle.refshim import e3nn_standin as E3

    E3.install(sys.modules)
    import adsorbdiff.relaxation.optimizers.lbfgs_torch as ref_lb
    from adsorbdiff.models.equiformer_v2.equiformer_v2_oc20 import EquiformerV2_OC20 as RefS2EF

    from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20 as Mirror
    from adsorbdiff_amd.synthetic import make_batch
    from oracle import eqv2_oracle as Q
    from tests.helpers import CFG4_KW, refill_parameters_by_name
    from tests.helpers_s2ef import EMB_SCALE, FULL_KW, RELAX_KW, SEED_SMALL, SMALL_KW, trained_like
    from tools.make_golden_relax import run_ref, write_npz

    torch.set_num_threads(8)
    assert FULL_KW == {k: v for k, v in dict(CFG4_KW, lmax_list=[4], load_energy_lin_ref=True).items() if k != "FOR_denoising"}

    # ------------------------------------------------------------------------------------------------ model outputs
    fx = dict(emb_scale=EMB_SCALE, seed=SEED_SMALL, atom_stride=ATOM_STRIDE, channel_stride=CH_STRIDE)
    torch.manual_seed(SEED_SMALL)
    ref = RefS2EF(None, None, None, use_s2_act_attn=False, proj_drop=0.0, **SMALL_KW).eval()
    torch.manual_seed(SEED_SMALL)
    mir = Mirror(None, None, None, **SMALL_KW).eval()
    check_mirror(ref, mir)   # the seeded draws themselves
    trained_like(ref), trained_like(mir)
    xb = model_case("small", ref, mir, make_batch(2, n_slab=16, n_ads=3, seed=3), SMALL_KW, fx)
    fx["small_x_blocks"] = xb

    torch.manual_seed(0)
    ref = trained_like(refill_parameters_by_name(RefS2EF(None, None, None, use_s2_act_attn=False, proj_drop=0.0, **FULL_KW).eval(), EMB_SCALE), scale_emb=False)
    torch.manual_seed(0)
    mir = trained_like(refill_parameters_by_name(Mirror(None, None, None, **FULL_KW).eval(), EMB_SCALE), scale_emb=False)
    L = FULL_KW["lmax_list"][0]
    xb = model_case("full", ref, mir, make_batch(2, n_slab=36, n_ads=4, seed=9), FULL_KW, fx)
    fx["full_x_blocks_sample"] = xb[:, ::ATOM_STRIDE, :, ::CH_STRIDE].contiguous()
    fx["full_x_blocks_degree_norms"] = torch.stack([torch.stack([xb[k, :, l * l:(l + 1) ** 2].double().norm() for l in range(L + 1)])
                                                    for k in range(xb.shape[0])])
    write_npz(GOLD / "eqv2_s2ef.npz", fx)

    # ------------------------------------------------------------------------------------------------ relaxation run
    torch.manual_seed(SEED_SMALL)
    ref = trained_like(RefS2EF(None, None, None, use_s2_act_attn=False, proj_drop=0.0, **RELAX_KW).eval())
    torch.manual_seed(SEED_SMALL)
    check_mirror(ref, trained_like(Mirror(None, None, None, **RELAX_KW).eval()))
    bt = make_batch(4, n_slab=36, n_ads=4, seed=71)
    rc, K = RELAX_KW["max_radius"], RELAX_KW["max_neighbors"]

    def s2ef(b_):
        with torch.no_grad():
            o = ref(b_.clone())
        return o["energy"], o["forces"]

    def never_truncates(res):
        worst = 0
        for pos in res["pos_log"]:
            ei, _, _ = Q.radius_graph_pbc(pos, bt.cell, bt.natoms, rc, 100000)
            worst = max(worst, int(torch.bincount(ei[1], minlength=pos.shape[0]).max()))
        assert worst < K, f"an atom has {worst} neighbours inside {rc} A: the K = {K} cap would truncate"
        return worst

    steps = 10
    mf0 = run_ref(ref_lb, bt.clone(), s2ef, 1e-12, 2, memory=50)["max_force"][0].sort().values.tolist()
    cands = [round(a + (b_ - a) * t, 6) for a, b_ in zip(mf0[:-1], mf0[1:]) for t in (0.5, 0.3, 0.7, 0.9)]
    for fmax in cands:
        res = run_ref(ref_lb, bt.clone(), s2ef, fmax, steps, memory=50)
        if res["margin"] > 1e-3 and res["masks"].logical_not().any() and res["masks"][0].any():
            break
    else:
        raise SystemExit("no fmax with a margin found")
    worst = never_truncates(res)
    print(f"[relax] fmax {fmax}: iterations {res['iterations']}, margin {res['margin']:.3e}, most neighbours {worst}, "
          f"masks {res['masks'].int().tolist()}")
    write_npz(GOLD / "relax_eqv2_run.npz", dict(
        fmax=fmax, steps=steps, memory=50, seed=SEED_SMALL, max_neighbours_seen=worst,
        **{k: v for k, v in res.items() if k != "margin"},
        **{k: getattr(bt, k) for k in ("pos", "atomic_numbers", "tags", "fixed", "cell", "natoms", "batch")}))


if __name__ == "__main__":
    main()
