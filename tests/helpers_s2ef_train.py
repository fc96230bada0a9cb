"""Float64 oracle of the S2EF training step of the force field (adsorbdiff_amd.train_step.PaiNNS2EFTrainStep): the
objective restated in plain torch (``s2ef_loss``), the model forward from the pieces of oracle/painn_oracle.py with the energy
head of tests/helpers_grad_forces.py (``forward``), torch.autograd for the gradient of every parameter, and what the CPU
and GPU tests share: the fixture's model and batch, the ragged configurations, the figures and their bounds.

The graph is given (the fixture's, rebuilt by the oracle, or the engine's export) and held fixed: positions carry no
gradient, as in the HIP step.  tests/test_s2ef_train_host.py pins this oracle to the reference's own loss and autograd
(tests/golden/s2ef_train.npz, tools/make_golden_s2ef_train.py)."""
import math

import torch

from adsorbdiff_amd.painn import PaiNN
from oracle import painn_oracle as O
from tests import helpers_grad_forces as GF
from tests import helpers_train as HT
from tests.helpers import batch_from_fixture, load_npz, rel_err
from tools.make_golden_s2ef_train import perturb_, sample_indices

F = torch.nn.functional

# the ragged configurations of tests/helpers_train.CONFIGS that apply to this model: every one but ragged_bare, which differs from
# "ragged" only by the denoiser's trained-like rescale and so repeats it here
CONFIG_NAMES = [k for k in HT.CONFIGS if k != "ragged_bare"]
NORMALIZERS = {"energy": {"mean": -0.7, "stdev": 1.9}, "forces": {"mean": 0.0, "stdev": 2.1}}
COEFFICIENTS = dict(energy_coefficient=1.0, force_coefficient=100.0)   # the shipped YAMLs


# ------------------------------------------------------------------------------------------------ the objective
def s2ef_loss(e_pred, f_pred, e_tgt, f_tgt, fixed, norm_energy=(0.0, 1.0), norm_forces=(0.0, 1.0), energy_coefficient=1.0,
              force_coefficient=30.0, train_on_free_atoms=True, counts=None):
    """(loss, energy term, force term) of OCPTrainer._compute_loss with DDPLoss over L1 / L2MAE (ocp_trainer.py:308-356,
    modules/loss.py:48-102).  ``counts`` = (B_glob, M_glob, W) of a multi-rank step; ``f_pred`` None: the energy term alone."""
    B = e_pred.shape[0]
    W = 1 if counts is None else counts[2]
    re = e_pred - (e_tgt - norm_energy[0]) / norm_energy[1]
    le = energy_coefficient * W / (B if counts is None else counts[0]) * re.abs().sum()
    if f_pred is None:
        return le, le, torch.zeros_like(le)
    in_s = (fixed == 0) if (train_on_free_atoms and fixed is not None) else torch.ones(f_pred.shape[0], dtype=torch.bool)
    rf = (f_pred - (f_tgt - norm_forces[0]) / norm_forces[1])[in_s]
    M = int(in_s.sum()) if counts is None else counts[1]
    if M == 0:   # no sample: DDPLoss's loss * world_size / num_samples is 0 * W / 0 = NaN
        return le + float("nan"), le, torch.norm(rf, p=2, dim=-1).sum() * float("nan")
    lf = force_coefficient * W / M * torch.norm(rf, p=2, dim=-1).sum()
    return le + lf, le, lf


def metrics(e_pred, f_pred, e_tgt, f_tgt, fixed, norm_energy=(0.0, 1.0), norm_forces=(0.0, 1.0)):
    """energy_mae, forces_mae of _compute_metrics after denorm (ocp_trainer.py:358-402): per system, and per component over
    the atoms with fixed == 0."""
    e_mae = (e_pred * norm_energy[1] + norm_energy[0] - e_tgt).abs().mean()
    if f_pred is None:
        return e_mae, torch.zeros_like(e_mae)
    free = (fixed == 0) if fixed is not None else torch.ones(f_pred.shape[0], dtype=torch.bool)
    return e_mae, (f_pred * norm_forces[1] + norm_forces[0] - f_tgt)[free].abs().mean()


# ------------------------------------------------------------------------------------------------ the model
def forward(sd, atomic_numbers, batch, num_systems, edge_index, dist, unit, *, hidden_channels, num_layers, cutoff,
            scale_factors, regress_forces=True, **_):
    """(energy [B], forces [N,3] or None) of the S2EF PaiNN (models/painn/painn.py:380-419) in the dtype of ``sd``, on a
    fixed graph: messages flow edge_index[0] -> edge_index[1]."""
    H = hidden_channels
    rbf = GF.radial_basis(dist, cutoff, sd["radial_basis.rbf.offset"])
    x = sd["atom_emb.embeddings.weight"][atomic_numbers.long() - 1]
    vec = torch.zeros(x.shape[0], 3, H, dtype=x.dtype)
    for i in range(num_layers):
        dx, dvec = O.message_layer(sd, "message_layers.%d." % i, x, vec, edge_index, rbf, unit, H)
        x = (x + dx) * (1 / math.sqrt(2.0))
        vec = vec + dvec
        dx, dvec = O.update_layer(sd, "update_layers.%d." % i, x, vec, H)
        x = (x + dx) * float(scale_factors[i])
        vec = vec + dvec
    per_atom = F.linear(O.ssilu(F.linear(x, sd["out_energy.0.weight"], sd["out_energy.0.bias"])),
                        sd["out_energy.2.weight"], sd["out_energy.2.bias"]).squeeze(1)
    energy = torch.zeros(num_systems, dtype=x.dtype).index_add_(0, batch.long(), per_atom)
    forces = O.output_head(sd, "out_forces.", x, vec, H).reshape(-1, 3) if regress_forces else None
    return energy, forces


def hyper(model):
    return dict(hidden_channels=model.hidden_channels, num_layers=model.num_layers, num_rbf=model.num_rbf,
                cutoff=float(model.cutoff), scale_factors=model.scale_factors(), regress_forces=bool(model.regress_forces))


def oracle_loss_and_grads(model, batch, graph, normalizers=None, energy_coefficient=1.0, force_coefficient=30.0,
                          train_on_free_atoms=True, counts=None, dtype=torch.float64):
    """loss, its terms, the predictions, the two metrics and {parameter name: gradient} in ``dtype``; ``graph`` =
    (edge_index [2, E], dist [E], unit [E, 3]); targets batch.energy, batch.forces, batch.fixed."""
    ei, dist, unit = graph
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    sd = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in model.state_dict().items()}
    leaves = {k: sd[k].clone().requires_grad_(True) for k in names}
    sd.update(leaves)
    e, f = forward(sd, batch.atomic_numbers.cpu(), batch.batch.cpu(), int(batch.natoms.shape[0]), ei.cpu().long(),
                   dist.cpu().to(dtype), unit.cpu().to(dtype), **hyper(model))
    nz = normalizers or {}
    ne = (nz["energy"]["mean"], nz["energy"]["stdev"]) if "energy" in nz else (0.0, 1.0)
    nf = (nz["forces"]["mean"], nz["forces"]["stdev"]) if "forces" in nz else (0.0, 1.0)
    fixed = batch.fixed.cpu() if getattr(batch, "fixed", None) is not None else None
    e_t = batch.energy.cpu().to(dtype)
    f_t = batch.forces.cpu().to(dtype) if f is not None else None
    loss, le, lf = s2ef_loss(e, f, e_t, f_t, fixed, ne, nf, energy_coefficient, force_coefficient, train_on_free_atoms, counts)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    mt = metrics(e.detach(), None if f is None else f.detach(), e_t, f_t, fixed, ne, nf)
    return {"loss": loss.detach(), "terms": torch.stack([le.detach(), lf.detach()]), "energy": e.detach(),
            "forces": None if f is None else f.detach(), "metrics": torch.stack(list(mt)), "grads": dict(zip(names, grads))}


def oracle_graph(model, batch):
    """(edge_index, dist, unit) by the oracle's graph builder in float32 (the S2EF model's 1e-6 distance floor is never
    reached by the synthetic systems)."""
    ei, _, dist, unit = HT.oracle_graph(model, batch)
    return ei, dist, unit


def engine_graph(model, batch_on_device):
    eng = model.engine(batch_on_device.pos.device)
    eng.build_graph(batch_on_device)
    ei, _, dist, unit = HT.graph_from_export(eng)
    return ei, dist, unit


# ------------------------------------------------------------------------------------------------ the fixture
def fixture_case():
    """(fixture, mirror model on the CPU with the fixture's weights, batch with targets, step keywords)."""
    fx = load_npz("s2ef_train.npz")
    L = int(fx["hp_num_layers"])
    scales = {f"upd_out_scalar_scale_{i}": float(fx["scale_factors"][i]) for i in range(L)}
    torch.manual_seed(int(fx["seed"]))
    m = PaiNN(None, 50, 1, hidden_channels=int(fx["hp_hidden_channels"]), num_layers=L, num_rbf=int(fx["hp_num_rbf"]),
              cutoff=float(fx["hp_cutoff"]), max_neighbors=int(fx["hp_max_neighbors"]), scale_file=scales)
    perturb_(m, int(fx["seed_perturb"]))
    sums = [float(v.double().sum()) for v in m.state_dict().values()]
    assert len(sums) == len(fx["state_sums"]) and all(a == b for a, b in zip(sums, fx["state_sums"])), "other weights than the fixture's"
    b = batch_from_fixture(fx)
    b.energy, b.forces = torch.from_numpy(fx["energy_target"]).float(), torch.from_numpy(fx["forces_target"]).float()
    kw = dict(normalizers={"energy": {"mean": float(fx["norm_energy"][0]), "stdev": float(fx["norm_energy"][1])},
                           "forces": {"mean": float(fx["norm_forces"][0]), "stdev": float(fx["norm_forces"][1])}},
              energy_coefficient=float(fx["energy_coefficient"]), force_coefficient=float(fx["force_coefficient"]),
              train_on_free_atoms=bool(fx["train_on_free_atoms"]))
    return fx, m, b, kw


def fixture_gradient_errors(fx, grads):
    """{name: relative error} of ``grads`` against the fixture: the stored entries (all of a small tensor, seeded positions
    of a large one) and the norm of the whole tensor, whichever is worse."""
    out = {}
    for name, norm in zip(fx["grad_names"], fx["grad_norms"]):
        name = str(name)
        g = torch.as_tensor(grads[name]).detach().double().cpu().reshape(-1)
        idx = sample_indices(name, g.numel())
        e = rel_err(g if idx is None else g[idx], fx["grad::" + name])
        out[name] = max(e, abs(float(g.norm()) - float(norm)) / float(norm))
    return out


# ------------------------------------------------------------------------------------------------ ragged configurations
def make_config_model(name):
    """The mirror S2EF PaiNN of a configuration of tests/helpers_train.CONFIGS on the CPU: seeded initialisers, biases and
    LayerNorm gains moved off their constants, scale factors that differ from 1."""
    cfg = HT.CONFIGS[name]
    torch.manual_seed(7)
    m = PaiNN(None, 50, 1, hidden_channels=cfg["H"], num_layers=cfg["L"], num_rbf=cfg["R"], cutoff=cfg["cutoff"],
              max_neighbors=cfg["K"], scale_file={"upd_out_scalar_scale_%d" % i: HT.SCALE_FACTORS[i] for i in range(cfg["L"])})
    return perturb_(m, 8)


def make_config_batch(name, seed=31):
    """The configuration's batch with random targets of the normalizers' magnitude."""
    b = HT.make_config_batch(name)
    g = torch.Generator().manual_seed(seed)
    B, N = int(b.natoms.shape[0]), int(b.pos.shape[0])
    b.energy = (NORMALIZERS["energy"]["mean"] + NORMALIZERS["energy"]["stdev"] * torch.randn(B, generator=g)).float()
    b.forces = (NORMALIZERS["forces"]["mean"] + NORMALIZERS["forces"]["stdev"] * torch.randn(N, 3, generator=g)).float()
    return b


def measure_step(m, bd, ref, step_kw, dev="cuda:0"):
    """PaiNNS2EFTrainStep.loss_and_grad on the device against ``ref`` (oracle_loss_and_grads or the fixture's figures as
    {"loss", "terms", "energy", "forces", "grads" or "fixture"}): a dict of plain figures."""
    from adsorbdiff_amd.train_step import PaiNNS2EFTrainStep

    step = PaiNNS2EFTrainStep(m, dev, **step_kw)
    step.zero_grad()
    loss = step.loss_and_grad(bd).double().cpu()
    figs = {"grads": {}, "missing": []}
    figs["loss"] = abs(float(loss[0]) - float(ref["loss"])) / abs(float(ref["loss"]))
    terms = torch.as_tensor(ref["terms"]).double()
    live = terms != 0
    figs["terms"] = float(((loss[1:] - terms).abs()[live] / terms.abs()[live]).max())
    figs["dead_terms_zero"] = bool((loss[1:][~live] == 0).all())
    figs["energy"] = rel_err(step.last_outputs[0].cpu(), ref["energy"])
    figs["forces"] = rel_err(step.last_outputs[1].cpu(), ref["forces"]) if ref["forces"] is not None else 0.0
    first = {}
    for k, p in m.named_parameters():
        if p.requires_grad:
            if p.grad is None:
                figs["missing"].append(k)
            else:
                first[k] = p.grad.clone()
    if "fixture" in ref:
        figs["grads"] = fixture_gradient_errors(ref["fixture"], first)
    else:
        figs["grads"] = {k: rel_err(first[k].cpu(), g) for k, g in ref["grads"].items()}
    if "metrics" in ref:
        figs["metrics"] = float(((step.metrics.double().cpu() - ref["metrics"]).abs() / ref["metrics"].abs().clamp(min=1e-30)).max())
    absent = HT.absent_embedding_rows(m, bd)
    figs["absent_rows"] = int(absent.sum())
    figs["absent_embedding_max"] = float(first["atom_emb.embeddings.weight"].cpu()[absent].abs().max())
    step.loss_and_grad(bd)   # no zero_grad: every gradient doubles
    figs["doubling"] = max(rel_err(dict(m.named_parameters())[k].grad, 2 * g1) for k, g1 in first.items())
    figs["worst_grad"], figs["worst_grad_name"] = max((e, k) for k, e in figs["grads"].items())
    return figs


def assert_step(figs, label=""):
    """The bounds of tests/helpers_train.assert_configuration for this step: loss, its terms and both outputs 1e-5; every
    gradient 1e-4 relative (the training budget); no parameter without a gradient; rows of absent elements exactly zero;
    doubling to 1e-6."""
    assert figs["loss"] < 1e-5 and figs["terms"] < 1e-5 and figs["dead_terms_zero"], (label, figs["loss"], figs["terms"])
    assert figs["energy"] < 1e-5 and figs["forces"] < 1e-5, (label, figs["energy"], figs["forces"])
    assert not figs["missing"], (label, figs["missing"])
    bad = {k: e for k, e in figs["grads"].items() if not e < 1e-4}
    assert not bad, (label, bad)
    assert figs.get("metrics", 0.0) < 1e-5, (label, figs.get("metrics"))
    assert figs["absent_rows"] > 0 and figs["absent_embedding_max"] == 0.0, (label, figs["absent_embedding_max"])
    assert figs["doubling"] < 1e-6, (label, figs["doubling"])


def describe(figs, label=""):
    return (f"{label}: loss {figs['loss']:.1e} terms {figs['terms']:.1e} energy {figs['energy']:.1e} forces {figs['forces']:.1e} "
            f"worst gradient {figs['worst_grad']:.2e} ({figs['worst_grad_name']}) doubling {figs['doubling']:.1e}")


def measure_fixture(dev="cuda:0"):
    fx, m, b, kw = fixture_case()
    m = m.to(dev)
    ref = {"loss": fx["loss"], "terms": fx["loss_terms"], "energy": fx["energy_pred"], "forces": fx["forces_pred"], "fixture": fx}
    return measure_step(m, b.clone().to(dev), ref, kw, dev)


def measure_configuration(name, dev="cuda:0", regress_forces=True):
    """A ragged configuration against the float64 oracle on the engine's exported graph."""
    m = make_config_model(name) if regress_forces else make_energy_only_model(name)
    m = m.to(dev)
    b = make_config_batch(name)
    bd = b.clone().to(dev)
    kw = dict(normalizers=NORMALIZERS, **COEFFICIENTS)
    ref = oracle_loss_and_grads(m, b, engine_graph(m, bd), **kw)
    figs = measure_step(m, bd, ref, kw, dev)
    figs["name"] = name
    return figs


def make_energy_only_model(name):
    cfg = HT.CONFIGS[name]
    torch.manual_seed(7)
    m = PaiNN(None, 50, 1, hidden_channels=cfg["H"], num_layers=cfg["L"], num_rbf=cfg["R"], cutoff=cfg["cutoff"],
              max_neighbors=cfg["K"], regress_forces=False,
              scale_file={"upd_out_scalar_scale_%d" % i: HT.SCALE_FACTORS[i] for i in range(cfg["L"])})
    return perturb_(m, 8)
