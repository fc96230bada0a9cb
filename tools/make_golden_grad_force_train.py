"""TEST INFRASTRUCTURE - generate tests/golden/grad_force_train.npz: the S2EF objective with ENERGY-GRADIENT forces in the loss
and the gradient of every parameter, from the REAL reference force field (adsorbdiff/models/painn/painn.py,
``regress_forces=False``) under the REAL reference loss.  Run in the build container only (needs the reference sources on
the import path, as tools/make_golden_grad_forces.py and tools/make_golden_s2ef_train.py do):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_grad_force_train.py            # writes the fixture
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_grad_force_train.py --check    # regenerates it and compares the bytes

What runs, in FLOAT64 on a frozen graph (built once in float32 by the reference's radius_graph_pbc and passed in with
``otf_graph=False``, as in tools/make_golden_grad_forces.py): ``out = model(batch)``, ``forces =
-torch.autograd.grad(out["energy"].sum(), pos, create_graph=True)``, then the reference's ``OCPTrainer._compute_loss`` (DDPLoss
over nn.L1Loss for the energy, over L2MAELoss for the forces) on a stand-in object, as tools/make_golden_s2ef_train.py calls it,
and ``torch.autograd.grad`` of the loss over the parameters: a second-order backward through the reference's own module.  The
reference's ``direct_forces=False`` branch is NOT used: it differentiates the node features, not the energy.

The predicted forces are the gradient of the model's normalised energy, so the force targets are normalised with mean 0 and
the ENERGY normaliser's stdev: the stand-in's ``normalizers["forces"]`` is that pair.

Weights are not stored (drawn from SEED, moved off their constants by ``perturb_``; per-tensor sums are recorded).  Gradients
of large tensors are stored as their float64 norm plus sampled entries, as in s2ef_train.npz.  The reference's symmetrised
edge list is stored too, so that the float64 oracle of tests/helpers_grad_force_train.py can be pinned on the same graph.
Asserted here: residuals stay away from the kinks of the objective, and every gradient is non-zero.
"""
from __future__ import annotations

import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from tools.make_golden_relax import GOLD, batch_arrays, write_npz  # noqa: E402
from tools.make_golden_s2ef_train import RESIDUAL_FLOOR, perturb_, sample_indices  # noqa: E402

FIXTURE = GOLD / "grad_force_train.npz"
HP = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
SEED, SEED_PERTURB, SEED_BATCH, SEED_TARGETS = 31, 32, 4343, 33
SYSTEMS = ((36, 4), (7, 1), (61, 3), (20, 2))          # slab + adsorbate atoms; the lower half of each slab is fixed
NORM_ENERGY = {"mean": -1.5, "stdev": 2.3}
ENERGY_COEFFICIENT, FORCE_COEFFICIENT = 2.0, 100.0


def make_inputs():
    from adsorbdiff_amd.data import Batch
    from adsorbdiff_amd.synthetic import make_system

    g = torch.Generator().manual_seed(SEED_BATCH)
    bt = Batch.from_data_list([make_system(g, ns, na, sid=str(i)) for i, (ns, na) in enumerate(SYSTEMS)])
    g = torch.Generator().manual_seed(SEED_TARGETS)
    B, N = int(bt.natoms.shape[0]), int(bt.pos.shape[0])
    bt.energy = (NORM_ENERGY["mean"] + NORM_ENERGY["stdev"] * torch.randn(B, generator=g)).float()
    bt.forces = (NORM_ENERGY["stdev"] * torch.randn(N, 3, generator=g)).float()
    return bt


def generate() -> dict:
    from oracle import refshim

    refshim.install()
    if "adsorbdiff.utils.rot_utils" not in sys.modules:   # not used by the S2EF trainer (see make_golden_s2ef_train.py)
        stub = types.ModuleType("adsorbdiff.utils.rot_utils")
        stub.axis_angle_to_matrix = None
        sys.modules["adsorbdiff.utils.rot_utils"] = stub
    from adsorbdiff.models.painn.painn import PaiNN as RefS2EF
    from adsorbdiff.modules.loss import DDPLoss
    from adsorbdiff.modules.normalizer import Normalizer as RefNormalizer
    from adsorbdiff.trainers.ocp_trainer import OCPTrainer
    from adsorbdiff.utils.utils import get_loss_module, radius_graph_pbc
    from torch import nn

    from adsorbdiff_amd.data import Batch
    from adsorbdiff_amd.painn import PaiNN as Mirror

    torch.set_num_threads(8)

    class IndexableBatch(Batch):   # the reference reads batch[target_name]
        def __getitem__(self, key):
            return getattr(self, key)

    torch.manual_seed(SEED)
    ref = perturb_(RefS2EF(None, 50, 1, scale_file=dict(SCALES), regress_forces=False, **HP).eval(), SEED_PERTURB)
    torch.manual_seed(SEED)
    mir = perturb_(Mirror(None, 50, 1, scale_file=dict(SCALES), regress_forces=False, **HP), SEED_PERTURB)
    sd_r, sd_m = ref.state_dict(), mir.state_dict()
    assert list(sd_r) == list(sd_m) and all(torch.equal(sd_r[k], sd_m[k]) for k in sd_r), "the mirror draws other weights"
    sums = np.array([float(v.double().sum()) for v in sd_r.values()], dtype=np.float64)
    names = [k for k, p in ref.named_parameters() if p.requires_grad]

    bt = make_inputs()
    B, N = int(bt.natoms.shape[0]), int(bt.pos.shape[0])
    dtype = torch.float64
    normalizers = {"energy": (NORM_ENERGY["mean"], NORM_ENERGY["stdev"]), "forces": (0.0, NORM_ENERGY["stdev"])}

    so = types.SimpleNamespace()
    cfg = [{"energy": {"fn": "mae", "coefficient": ENERGY_COEFFICIENT}}, {"forces": {"fn": "l2mae", "coefficient": FORCE_COEFFICIENT}}]
    so.loss_fns = []
    for loss in cfg:
        for target in loss:
            loss_name = loss[target].get("fn", "mae")
            loss_fn = getattr(nn, loss_name)() if hasattr(nn, loss_name) else get_loss_module(loss_name)
            so.loss_fns.append((target, {"fn": DDPLoss(loss_fn, loss_name, loss[target].get("reduction", "mean")),
                                         "coefficient": loss[target].get("coefficient", 1)}))
    so.output_targets = {"energy": {"level": "system"}, "forces": {"level": "atom", "train_on_free_atoms": True,
                                                                   "eval_on_free_atoms": True}}
    so.normalizers = {}
    for key, (mean, std) in normalizers.items():
        so.normalizers[key] = RefNormalizer(mean=mean, std=std)
        so.normalizers[key].mean = torch.as_tensor(mean, dtype=dtype)
        so.normalizers[key].std = torch.as_tensor(std, dtype=dtype)

    ei, co, nb = radius_graph_pbc(bt.clone(), HP["cutoff"], HP["max_neighbors"], True)   # float32 graph, built once
    cap = {}
    torch.set_default_dtype(torch.float64)
    ref.double()
    ref.otf_graph = False
    orig = ref.generate_graph_values

    def rec(data):
        out = orig(data)
        cap["edge_index"], cap["dist"], cap["unit"] = out[0].clone(), out[2].detach().clone(), out[3].detach().clone()
        return out

    ref.generate_graph_values = rec
    try:
        b = IndexableBatch()
        b.__dict__.update(bt.clone().__dict__)
        b.edge_index, b.cell_offsets, b.neighbors = ei, co.to(dtype), nb
        b.pos = bt.pos.to(dtype).clone().requires_grad_(True)
        b.cell = bt.cell.to(dtype)
        b.energy, b.forces = bt.energy.to(dtype), bt.forces.to(dtype)
        with torch.enable_grad():
            energy = ref(b)["energy"]
            (gpos,) = torch.autograd.grad(energy.sum(), b.pos, create_graph=True)
            forces = -gpos
            out = {"energy": energy.view(B, -1), "forces": forces.view(N, -1)}   # OCPTrainer._forward
            loss = OCPTrainer._compute_loss(so, out, b)
            terms = []
            for target, info in so.loss_fns:
                only = types.SimpleNamespace(loss_fns=[(target, info)], output_targets=so.output_targets, normalizers=so.normalizers)
                terms.append(OCPTrainer._compute_loss(only, out, b).detach())
            params = dict(ref.named_parameters())
            grads = torch.autograd.grad(loss, [params[k] for k in names])
        r = {"loss": loss.detach().double(), "terms": torch.stack(terms).double(), "energy": energy.detach().double().reshape(-1),
             "forces": forces.detach().double().reshape(N, 3), "grads": {k: g.detach().double() for k, g in zip(names, grads)}}
    finally:
        del ref.generate_graph_values
        ref.float()
        torch.set_default_dtype(torch.float32)

    # the reference's symmetrised edge list with integer shifts (as grad_forces.npz stores it)
    src, dst = cap["edge_index"]
    vec = cap["unit"] * cap["dist"][:, None]
    off = vec - (bt.pos.double()[src] - bt.pos.double()[dst])
    cell_e = bt.cell.double()[bt.batch[dst]]
    shifts = torch.linalg.solve(cell_e.transpose(1, 2), off.unsqueeze(-1)).squeeze(-1)
    assert float((shifts - shifts.round()).abs().max()) < 1e-6

    e_res = r["energy"] - (bt.energy.double() - NORM_ENERGY["mean"]) / NORM_ENERGY["stdev"]
    f_res = (r["forces"] - bt.forces.double() / NORM_ENERGY["stdev"]).norm(dim=1)
    free = bt.fixed == 0
    print(f"loss {float(r['loss']):.10f} terms {r['terms'].tolist()}; residual floors: energy {float(e_res.abs().min()):.3e}, "
          f"free-atom force norm {float(f_res[free].min()):.3e}; free atoms {int(free.sum())} of {N}; edges {int(src.numel())}")
    assert float(e_res.abs().min()) >= RESIDUAL_FLOOR and float(f_res[free].min()) >= RESIDUAL_FLOOR
    assert 0 < int(free.sum()) < N
    assert abs(float(r["terms"].sum()) - float(r["loss"])) < 1e-12 * abs(float(r["loss"]))
    for k in names:
        assert float(r["grads"][k].norm()) > 0.0, k

    fx = dict(batch_arrays(bt), energy_target=bt.energy, forces_target=bt.forces, seed=SEED, seed_perturb=SEED_PERTURB,
              state_sums=sums, energy_coefficient=ENERGY_COEFFICIENT, force_coefficient=FORCE_COEFFICIENT,
              train_on_free_atoms=True, scale_factors=np.array([SCALES[f"upd_out_scalar_scale_{i}"] for i in range(HP["num_layers"])]),
              norm_energy=np.array([NORM_ENERGY["mean"], NORM_ENERGY["stdev"]]),
              loss=r["loss"], loss_terms=r["terms"], energy_pred=r["energy"], forces_pred=r["forces"],
              edge_src=src.to(torch.int32), edge_dst=dst.to(torch.int32), edge_shift=shifts.round().to(torch.int8),
              grad_names=np.array(names), grad_norms=np.array([float(r["grads"][k].norm()) for k in names], dtype=np.float64),
              **{"hp_" + k: v for k, v in HP.items()})
    for k in names:
        g = r["grads"][k].reshape(-1)
        idx = sample_indices(k, g.numel())
        fx["grad::" + k] = (g if idx is None else g[idx]).double()
    return fx


def main() -> None:
    check = "--check" in sys.argv[1:]
    fx = generate()
    if not check:
        write_npz(FIXTURE, fx)
        return
    with tempfile.TemporaryDirectory() as tmp:
        again = Path(tmp) / FIXTURE.name
        write_npz(again, fx)
        same = again.read_bytes() == FIXTURE.read_bytes()
    print("fixture regenerated byte-identically" if same else "the regenerated fixture DIFFERS from the committed one")
    raise SystemExit(0 if same else 1)


if __name__ == "__main__":
    main()
