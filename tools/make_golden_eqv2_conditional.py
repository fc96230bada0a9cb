"""TEST INFRASTRUCTURE - generate tests/golden/eqv2_conditional_l4.npz by running the REAL conditional EquiformerV2
denoiser on CPU (the shipped configs/denoising/eqv2_conditional.yml shape: L = 4 / M = 2, C = 128, 8 blocks,
``energy_encoding: scalar``).  Run in the build container only (needs the reference sources on the import path, as
oracle/make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_eqv2_conditional.py

Recipe of oracle/make_golden.py::main_eqv2_cfg4: the 21 M weights are NOT stored; every parameter with two or more
dimensions is refilled by tests/helpers.py::refill_parameters_by_name and the generator asserts that the mirror class
holds the reference's values.  ``energy_embedding`` then gets seeded N(0, 1) weight and bias (stored: 2 x 128 values;
the reference initialises the bias to zero, which would hide the term in sampling mode), and that layer alone is cast
to fp16: the reference feeds ``node_wise_y.half()`` into it (equiformer_v2_denoising.py:258-264), which runs only under
autocast or with the layer in fp16 - every other layer stays fp32.

Two cases on one 2-system batch: ``sampling=True`` (zero energies) and ``sampling=False`` with per-system energies
-1.73 / 2.41 eV (not representable in fp16).  Stored per case (prefix ``samp_`` / ``cond_``): (f1, f2), the full l = 0
rows of the node embedding after the energy and edge-degree embeddings, and after the edge-degree embedding and after
every block a strided sample plus per-degree norms over all atoms.  Shared: inputs, the reference's edge list, its
parameter names, the energy layer's fp32 values.  The archive is written with fixed zip metadata, so two runs give
identical bytes.
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

OUT = ROOT / "tests" / "golden" / "eqv2_conditional_l4.npz"
ATOM_STRIDE, CH_STRIDE = 9, 32
N_SLAB, N_ADS = 36, 4     # two 40-atom systems: the fixture stays small (the edge list is stored, so ties do not matter)
ENERGIES = (-1.73, 2.41)
EE_SEED = 20240


def write_npz(path: Path, arrays: dict) -> None:
    """np.savez_compressed with a fixed member timestamp (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main() -> None:
    from oracle import refshim

    refshim.install()
    from oracle.refshim import e3nn_standin as E3

    E3.install(sys.modules)
    from adsorbdiff.models.equiformer_v2.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos as RefEqV2

    from adsorbdiff_amd.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos as MyEqV2
    from adsorbdiff_amd.synthetic import make_batch
    from tests.helpers import CFG4_KW, refill_parameters_by_name

    torch.set_num_threads(8)
    kw = dict(CFG4_KW, lmax_list=[4], energy_encoding="scalar")
    emb_scale = 300.0
    torch.manual_seed(0)
    eq = refill_parameters_by_name(RefEqV2(None, None, None, use_s2_act_attn=False, proj_drop=0.0, **kw).eval(), emb_scale)
    torch.manual_seed(0)
    mine = refill_parameters_by_name(MyEqV2(None, None, None, **kw).eval(), emb_scale)
    C = kw["sphere_channels"]
    g = torch.Generator().manual_seed(EE_SEED)
    ee_w = torch.randn(C, 1, generator=g)
    ee_b = torch.randn(C, generator=g)
    with torch.no_grad():
        for m in (eq, mine):
            m.energy_embedding.weight.copy_(ee_w)
            m.energy_embedding.bias.copy_(ee_b)
    rp, mp = dict(eq.named_parameters()), dict(mine.named_parameters())
    assert list(rp) == list(mp), "mirror parameter order differs from the reference's"
    assert all(tuple(rp[k].shape) == tuple(mp[k].shape) for k in rp)
    bad_names = [k for k in rp if k != "atom_radii" and not torch.equal(rp[k], mp[k])]
    assert not bad_names, ("mirror weights differ from the reference's", bad_names[:5])
    names = list(rp)
    nparams = sum(p.numel() for p in eq.parameters())
    eq.energy_embedding.half()   # the only fp16 layer (what autocast does to it; the rest stays fp32)

    b = make_batch(2, n_slab=N_SLAB, n_ads=N_ADS, seed=9)
    bad = set(torch.nonzero(torch.isnan(eq.atom_radii)).flatten().tolist())
    z = b.atomic_numbers.clone()
    for zb in bad:
        z[z == zb] = 47.0
    b.atomic_numbers = z
    b.energy = torch.tensor(ENERGIES, dtype=torch.float32)
    gq = eq.generate_graph(b.clone(), enforce_max_neighbors_strictly=True)
    L = kw["lmax_list"][0]
    fx = dict(edge_index=gq[0].to(torch.int32), edge_vec=gq[2], energy=b.energy.clone(), ee_weight=ee_w, ee_bias=ee_b,
              param_names=np.array(names, dtype="S"),
              param_shapes=np.array([",".join(map(str, rp[k].shape)) for k in names], dtype="S"),
              n_params=nparams, emb_scale=emb_scale, lmax=L, mmax=kw["mmax_list"][0], atom_stride=ATOM_STRIDE,
              channel_stride=CH_STRIDE, pos=b.pos, atomic_numbers=b.atomic_numbers, tags=b.tags, fixed=b.fixed,
              cell=b.cell, natoms=b.natoms, batch=b.batch)
    for case, sampling in (("samp", True), ("cond", False)):
        eq.sampling = sampling
        rec = {}
        hooks = [eq.blocks[0].register_forward_pre_hook(lambda m_, a_: rec.__setitem__("x0", a_[0].embedding.detach().clone()))]
        for bi_, blk_ in enumerate(eq.blocks):
            hooks.append(blk_.register_forward_hook(lambda m_, i_, o_, bi_=bi_: rec.__setitem__(bi_, o_.embedding.detach().clone())))
        with torch.no_grad():
            f1, f2 = eq(b.clone())
        for h_ in hooks:
            h_.remove()
        xb = torch.stack([rec["x0"]] + [rec[i] for i in range(kw["num_layers"])])   # [9, N, 25, 128]
        assert xb.dtype == torch.float32
        assert bool(torch.isfinite(f1).all()) and bool(torch.isfinite(xb).all())
        # the term the reference added, recomputed with the formula the kernel implements
        y = torch.zeros(len(ENERGIES)) if sampling else b.energy
        w16, b16 = ee_w.half().float().reshape(-1), ee_b.half().float()
        term = (y.half().float()[:, None] * w16[None, :] + b16[None, :]).half().float()
        with torch.no_grad():
            ref_term = eq.energy_embedding(y[:, None].half()).float()
        assert torch.equal(term, ref_term), "fp16 term formula"
        norms = torch.stack([torch.stack([xb[k, :, l * l:(l + 1) ** 2].double().norm() for l in range(L + 1)])
                             for k in range(xb.shape[0])])
        fx.update({f"{case}_f1": f1, f"{case}_f2": f2, f"{case}_x_l0": xb[0, :, 0, :].contiguous(),
                   f"{case}_term": term,
                   f"{case}_x_blocks_sample": xb[:, ::ATOM_STRIDE, :, ::CH_STRIDE].contiguous(),
                   f"{case}_x_blocks_degree_norms": norms})
        print(f"[eqv2 conditional] {case}: |f1|max={f1.abs().max():.4e} |f2|max={f2.abs().max():.4e}")
    assert not torch.equal(fx["samp_f1"], fx["cond_f1"])
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in fx.items()}
    write_npz(OUT, arrays)
    print("written", OUT)


if __name__ == "__main__":
    main()
