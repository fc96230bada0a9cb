"""TEST INFRASTRUCTURE - generate tests/golden/train_tr_only.npz by running the REAL reference on CPU: the training step of
the translation-only (one-head, ``so3_denoising=False``) PaiNN denoiser.  Run in the build container only (needs the
reference sources on the import path, as oracle/make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_tr_only.py

Recipe of oracle/make_golden.py sections 6 and 10: the reference's ``ads_COM_gaussian_schedule`` and
``DenoisingTrainer._compute_loss`` are executed from their source file (the functions only: importing the trainer module
drags in the whole training stack) on a batch of the train_small.npz shape (4 systems of 36 + 4 atoms; H = 128, 2 layers,
128 radial functions, 6 A / 20 neighbours), then torch.autograd through the reference's one-head PaiNN gives the gradients.
The weights are seed 0 + perturbed biases (seed 3) + the trained-like rescale of tests/helpers_train.py and are NOT stored:
the generator asserts that the mirror class reproduces them bit for bit.  Stored: the clean and the noised batch, the
scores, the model output, the loss, the parameter names and, for every gradient, its norm and a strided sample of 256
elements.  Before anything is written the host mirror ``adsorbdiff_amd.noising.ads_COM_gaussian_schedule`` must reproduce
the reference's noised batch under the same seeds.  Arrays and names only; the archive is written with fixed zip
metadata, so two runs give identical bytes.
"""
from __future__ import annotations

import ast
import io
import sys
import types
import zipfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

OUT = ROOT / "tests" / "golden" / "train_tr_only.npz"
HP = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
WEIGHT_SEED, BIAS_SEED, NOISE_SEED, BATCH_SEED = 0, 3, 2026, 71
TPARAMS = dict(ads_std_low=0.1, ads_std_high=10, num_steps=50)


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


def reference_functions(ref_root: Path):
    """ads_COM_gaussian_schedule and DenoisingTrainer._compute_loss compiled from the reference's source file."""
    import torch_scatter as _ts

    tree = ast.parse((ref_root / "adsorbdiff" / "trainers" / "sde_denoising_trainer.py").read_text())
    wanted = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == "ads_COM_gaussian_schedule":
            wanted[node.name] = node
        if isinstance(node, ast.ClassDef) and node.name == "DenoisingTrainer":
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == "_compute_loss":
                    wanted[sub.name] = sub
    assert set(wanted) == {"ads_COM_gaussian_schedule", "_compute_loss"}, set(wanted)
    # (rot_utils is only touched by the so3_denoising branch of the loss, which this fixture does not take: importing it
    # evaluates the IGSO(3) series for minutes)
    ns = {"torch": torch, "np": np, "scatter": _ts.scatter, "rot_utils": None}
    exec(compile(ast.Module(body=list(wanted.values()), type_ignores=[]), "<reference functions>", "exec"), ns)
    return ns["ads_COM_gaussian_schedule"], ns["_compute_loss"]


def prepare_weights_(model) -> None:
    """Biases and LayerNorm parameters off their constants (seed BIAS_SEED), then trained-like magnitudes."""
    from tests.helpers_train import trained_like_rescale_

    g = torch.Generator().manual_seed(BIAS_SEED)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if n_.endswith("bias") or "layernorm" in n_:
                p_.add_(0.1 * torch.randn(p_.shape, generator=g))
    trained_like_rescale_(model)


def main() -> None:
    from oracle import refshim

    refshim.install()
    import adsorbdiff
    from adsorbdiff.models.painn.painn_denoising import PaiNN as RefPaiNN

    from adsorbdiff_amd import noising
    from adsorbdiff_amd.painn_denoising import PaiNN as MyPaiNN
    from adsorbdiff_amd.synthetic import make_batch

    ref_schedule, ref_compute_loss = reference_functions(Path(list(adsorbdiff.__path__)[0]).resolve().parent)
    torch.set_num_threads(8)
    torch.manual_seed(WEIGHT_SEED)
    ref = RefPaiNN(None, 50, 1, scale_file=SCALES, so3_denoising=False, **HP)
    prepare_weights_(ref)
    torch.manual_seed(WEIGHT_SEED)
    mine = MyPaiNN(None, 50, 1, scale_file=SCALES, so3_denoising=False, **HP)
    prepare_weights_(mine)
    sd_r, sd_m = ref.state_dict(), mine.state_dict()
    assert [k for k, _ in ref.named_parameters()] == [k for k, _ in mine.named_parameters()]
    assert all(torch.equal(sd_r[k], sd_m[k]) for k in sd_r if k != "atom_radii"), "mirror weights differ from the reference's"
    assert not any(k.startswith("out_forces2.") for k in sd_r)

    bt = make_batch(4, n_slab=36, n_ads=4, seed=BATCH_SEED)
    bt.fixed = bt.fixed.clone()
    pos_clean = bt.pos.clone()
    torch.manual_seed(NOISE_SEED)
    nb = ref_schedule(bt.clone(), TPARAMS)
    # the host mirror, same random stream
    torch.manual_seed(NOISE_SEED)
    mb = noising.ads_COM_gaussian_schedule(bt.clone(), TPARAMS)
    for key in ("pos", "tr_sigma", "tr_score", "ads_center_noise_vec"):
        a, r = getattr(mb, key), getattr(nb, key)
        assert a.shape == r.shape, key
        dv = (a - r).abs().max().item()
        assert dv <= 1e-6 * max(1.0, r.abs().max().item()), (key, dv)
    ads = bt.tags == 2
    assert torch.equal(nb.pos[~ads], pos_clean[~ads])
    for b in range(4):   # the adsorbate has collapsed to one point
        rows = nb.pos[ads & (bt.batch == b)]
        assert bool((rows == rows[0]).all())

    ref.train()
    ref.zero_grad()
    o1 = ref(nb.clone())
    assert torch.is_tensor(o1) and bool(torch.isfinite(o1).all())
    fake_self = types.SimpleNamespace(config={"optim": {}, "model_attributes": {"so3_denoising": False}}, device="cpu")
    out1 = o1.detach().clone()
    loss_r = ref_compute_loss(fake_self, {"positions": o1}, nb)
    loss_r.backward()
    names, norms, samples = [], [], {}
    for k, p in ref.named_parameters():
        names.append(k)
        if p.grad is None:
            norms.append(0.0)
            continue
        g = p.grad.reshape(-1)
        assert bool(torch.isfinite(g).all()), k
        norms.append(float(g.double().norm()))
        idx = torch.linspace(0, g.numel() - 1, min(256, g.numel())).round().long()
        samples["gidx::" + k] = idx
        samples["gval::" + k] = g[idx].clone()
    trainable = {k for k, p in ref.named_parameters() if p.requires_grad}
    without = [k for k, v in zip(names, norms) if v == 0.0 and k in trainable]
    assert without and all(k.startswith("out_energy.") for k in without), without
    print(f"[train tr-only] loss {loss_r.item():.8f}; {sum(1 for v in norms if v > 0)} of {len(names)} parameters with "
          f"gradient; |g| from {min(v for v in norms if v > 0):.3e} to {max(norms):.3e}")
    fx = dict(pos_clean=pos_clean, pos_noised=nb.pos, tr_sigma=nb.tr_sigma, tr_score=nb.tr_score,
              ads_center_noise_vec=nb.ads_center_noise_vec, out1=out1, loss=loss_r.detach(), weight_seed=WEIGHT_SEED,
              bias_seed=BIAS_SEED, noise_seed=NOISE_SEED, grad_names=np.array(names, dtype="S"), grad_norms=np.array(norms),
              atomic_numbers=bt.atomic_numbers, tags=bt.tags, fixed=bt.fixed, cell=bt.cell, natoms=bt.natoms, batch=bt.batch,
              scale_factors=np.array([SCALES["upd_out_scalar_scale_0"], SCALES["upd_out_scalar_scale_1"]]))
    for k, v in HP.items():
        fx["hp_" + k] = v
    for k, v in TPARAMS.items():
        fx["tp_" + k] = v
    fx.update(samples)
    write_npz(OUT, {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in fx.items()})
    print("written", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
