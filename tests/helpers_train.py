"""Float64 gradient oracle of the score-matching training step, and the table of adversarial configurations that the CPU
test (tests/test_train_oracle.py) and the GPU tests (tests/test_gpu_training.py) share.

The oracle is torch.autograd through oracle/painn_oracle.py::painn_forward and oracle/train_oracle.py::score_matching_loss
(plain PyTorch, pinned to the reference function by function) in float64.  The graph is built once in float32 (by the oracle
or exported by the engine), its distances and unit vectors are cast and held fixed: positions carry no gradient, as in the
HIP step."""
import math

import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.so3_tables import Igso3Tables
from adsorbdiff_amd.synthetic import make_system
from oracle import painn_oracle as O
from oracle import train_oracle as TO
from tests.helpers import load_npz

TARGET_KEYS = ("tr_sigma", "rot_sigma", "tr_score", "rot_score")

# name -> H, L, R, cutoff, K, systems (slab + adsorbate atoms); what each one reaches is in the comment
CONFIGS = {
    # unequal segments, a 1-atom adsorbate, self-image edges (source == target with a non-zero shift)
    "ragged": dict(H=128, L=2, R=128, cutoff=6.0, K=20, systems=((36, 4), (7, 1), (61, 3), (20, 2))),
    # the same batch at the bare initialisers (no trained-like rescale)
    "ragged_bare": dict(H=128, L=2, R=128, cutoff=6.0, K=20, systems=((36, 4), (7, 1), (61, 3), (20, 2)), bare=True),
    # B = 1, and the only layer is the vec_is_zero one
    "single": dict(H=128, L=1, R=128, cutoff=6.0, K=20, systems=((36, 4),)),
    # zero-padded basis staging of message_bwd.hip / rbf_wgrad.hip
    "narrow_basis": dict(H=128, L=2, R=32, cutoff=6.0, K=20, systems=((36, 4), (7, 1), (61, 3), (20, 2))),
    # generic weight-gradient kernel with partial 64-wide tiles, 3 channel slices
    "odd_width": dict(H=192, L=3, R=96, cutoff=6.0, K=12, systems=((50, 4), (9, 2), (130, 5))),
    # a system above 256 atoms next to small ones: both graph paths feed one backward
    "mixed_csr": dict(H=128, L=2, R=128, cutoff=12.0, K=50, systems=((300, 4), (12, 1), (36, 4))),
    # the last adsorbate atom of the 61+3 system lifted to z = 28: an empty CSR segment
    "isolated": dict(H=128, L=2, R=128, cutoff=6.0, K=20, systems=((36, 4), (7, 1), (61, 3), (20, 2)), lift=(2, 28.0)),
    # 70 adsorbate atoms: the loss kernel's lane loop
    "big_adsorbate": dict(H=128, L=2, R=128, cutoff=6.0, K=20, systems=((40, 70), (36, 4))),
    # the 900-atom hub of test_hub_atom_with_many_incoming_edges, some atoms tagged 2: in-degree > 256 in the backward
    "hub": dict(H=128, L=2, R=128, cutoff=12.0, K=120, systems="hub"),
    # the shipped width, ragged
    "full_width": dict(H=512, L=2, R=128, cutoff=12.0, K=50, systems=((196, 4), (30, 2))),
}
SCALE_FACTORS = (1.05, 0.9, 1.1, 0.95, 1.02, 0.97)   # differ from 1: the step and the oracle must both apply them


def igso3_tables():
    """(tables for PaiNNTrainStep, look-ups for the oracle's loss) from tests/golden/igso3_tables.npz."""
    tb = load_npz("igso3_tables.npz")
    step_tables = Igso3Tables(tb["omegas"], None, None, tb["exp_score_norm"])
    oracle_tables = TO.Igso3({"_omegas_array": tb["omegas"], "_cdf_vals": None, "_score_norms": None,
                              "_exp_score_norms": tb["exp_score_norm"]})
    return step_tables, oracle_tables


def hub_batch():
    """900 atoms at log-uniform radii around atom 0 (272 incoming edges at K = 120, cutoff 12), as in
    tests/test_gpu_parity.py::test_hub_atom_with_many_incoming_edges; a few atoms are tagged as adsorbate."""
    torch.manual_seed(11)
    n = 900
    r = torch.exp(torch.rand(n - 1) * math.log(11.0 / 0.02)) * 0.02
    pos = torch.zeros(n, 3)
    pos[1:] = torch.nn.functional.normalize(torch.randn(n - 1, 3), dim=1) * r[:, None]
    b = Batch()
    b.pos = (pos + 50.0).float()
    b.atomic_numbers = torch.randint(1, 80, (n,)).float()
    b.tags = torch.ones(n, dtype=torch.long)
    b.tags[[0, 3, 200, 450, 899]] = 2
    b.fixed = torch.zeros(n, dtype=torch.long)
    b.cell = (torch.eye(3) * 100.0).reshape(1, 3, 3)
    b.natoms = torch.tensor([n])
    b.batch = torch.zeros(n, dtype=torch.long)
    b.sid = ["hub"]
    return b


def _cfg(name_or_cfg):
    return name_or_cfg if isinstance(name_or_cfg, dict) else CONFIGS[name_or_cfg]


def make_config_batch(name):
    """``name``: a key of CONFIGS, or a dict of the same form."""
    cfg = _cfg(name)
    if cfg["systems"] == "hub":
        return hub_batch()
    g = torch.Generator().manual_seed(4242)
    systems = []
    for i, (n_slab, n_ads) in enumerate(cfg["systems"]):
        d = make_system(g, n_slab, n_ads, sid=str(i))
        if n_ads > 8:   # the generator draws the adsorbate within 0.7 A of one point: spread a large one to atomic distances
            centre = d.pos[n_slab:].mean(0, keepdim=True)
            d.pos[n_slab:] = centre + (d.pos[n_slab:] - centre) * (n_ads / 4.0) ** (1.0 / 3.0)
        systems.append(d)
    if "lift" in cfg:
        which, z = cfg["lift"]
        systems[which].pos[-1, 2] = z
    return Batch.from_data_list(systems)


def trained_like_rescale_(model):
    """The rule of names of test_config5_width_loss_and_gradients_vs_reference_autograd, for any width."""
    H = model.hidden_channels
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if "x_layernorm" in n_:
                p_.mul_(0.05)
            if n_.endswith("x_proj.2.weight") or n_.endswith("x_proj.2.bias"):
                p_[2 * H:].mul_(1e-2)
            if n_.endswith("xvec_proj.2.weight") or n_.endswith("xvec_proj.2.bias"):
                p_.mul_(0.3)
            if n_.endswith("output_network.1.vec2_proj.weight"):
                p_.mul_(2e-4)


def make_config_model(name):
    """The mirror PaiNN of a configuration on the CPU: seeded initialisers, biases and LayerNorm parameters moved off their
    constants, then rescaled to trained-like magnitudes (not for a `bare` configuration)."""
    cfg = _cfg(name)
    torch.manual_seed(7)
    m = PaiNN(None, 50, 1, hidden_channels=cfg["H"], num_layers=cfg["L"], num_rbf=cfg["R"], cutoff=cfg["cutoff"],
              max_neighbors=cfg["K"], so3_denoising=True,
              scale_file={"upd_out_scalar_scale_%d" % i: SCALE_FACTORS[i] for i in range(cfg["L"])})
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if n_.endswith("bias") or "layernorm" in n_:
                p_.add_(0.1 * torch.randn(p_.shape, generator=g))
    if not cfg.get("bare"):
        trained_like_rescale_(m)
    assert all(abs(s - 1.0) > 1e-3 for s in m.scale_factors())
    return m


def make_targets(num_systems, seed=5):
    """Random targets with the magnitudes tr_so3_schedule gives: sigmas log-uniform over the schedule's range, scores of
    order 1 / sigma, no z component in the translation score."""
    g = torch.Generator().manual_seed(seed)
    B = num_systems
    tr_sigma = 0.1 * (10.0 / 0.1) ** torch.rand(B, 1, generator=g)
    rot_sigma = 0.01 * (1.55 / 0.01) ** torch.rand(B, 1, generator=g)
    tr_score = torch.randn(B, 3, generator=g) / tr_sigma
    tr_score[:, 2] = 0.0
    rot_score = torch.randn(B, 3, generator=g) / rot_sigma
    return {"tr_sigma": tr_sigma, "rot_sigma": rot_sigma, "tr_score": tr_score, "rot_score": rot_score}


def oracle_graph(model, batch):
    """(edge_index [2, E], neighbors [B], dist [E], unit_vec [E, 3]) by the oracle, float32."""
    return O.generate_graph_values(batch.pos.cpu().float(), batch.cell.cpu().float().reshape(-1, 3, 3), batch.natoms.cpu(),
                                   float(model.cutoff), int(model.max_neighbors))


def graph_from_export(engine):
    """The engine's current graph (Engine.export_graph) in the oracle's form: rows in the device's CSR order."""
    _, _, _, es, ed, dist, vec = engine.export_graph()
    ei = torch.stack([es.long().cpu(), ed.long().cpu()])
    return ei, None, dist.cpu().float(), vec.cpu().float()


def oracle_loss_and_grads(model, batch, targets, oracle_tables, graph=None, dtype=torch.float64):
    """loss, its two terms, both heads' outputs and {parameter name: gradient} of the score-matching step in ``dtype`` by
    torch.autograd through the oracle.  Parameters without a path to the loss (out_energy.*) map to None."""
    ei, nb, dist, unit = graph if graph is not None else oracle_graph(model, batch)
    g = (ei, nb, dist.to(dtype), unit.to(dtype))
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    sd = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in model.state_dict().items()}
    leaves = {k: sd[k].clone().requires_grad_(True) for k in names}
    sd.update(leaves)
    f1, f2 = O.painn_forward(sd, batch.pos.cpu().to(dtype), batch.atomic_numbers.cpu(), batch.cell.cpu().to(dtype),
                             batch.natoms.cpu(), hidden_channels=model.hidden_channels, num_layers=model.num_layers,
                             num_rbf=model.num_rbf, cutoff=float(model.cutoff), max_neighbors=int(model.max_neighbors),
                             scale_factors=model.scale_factors(), graph=g)
    f1, f2 = f1.reshape(-1, 3), f2.reshape(-1, 3)
    noised = {k: targets[k].cpu().float().to(dtype) for k in TARGET_KEYS}
    loss, terms = TO.score_matching_loss(f1, f2, batch.tags.cpu().long(), batch.batch.cpu().long(), noised, oracle_tables)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return {"loss": loss.detach(), "terms": torch.stack([t.detach() for t in terms]), "out1": f1.detach(),
            "out2": f2.detach(), "grads": dict(zip(names, grads))}


def absent_embedding_rows(model, batch):
    """Rows of atom_emb.embeddings.weight that no atom of the batch selects."""
    rows = torch.ones(model.atom_emb.embeddings.weight.shape[0], dtype=torch.bool)
    rows[batch.atomic_numbers.cpu().long() - 1] = False
    return rows


# ------------------------------------------------------------------------------------------------ the step on the device
_DEVICE_CASES = {}


def device_case(name, dev):
    """(model on ``dev``, batch on ``dev``, targets, float64 reference, tables) of a configuration; the reference's graph is
    the engine's own export (cast to float64), so that the comparison is about the step and not about ties in the K-th
    neighbour.  Cached per process: the three backward forms share one reference.  Asserts the structural property the
    configuration exists for, on the graph the device built."""
    if name in _DEVICE_CASES:
        return _DEVICE_CASES[name]
    m = make_config_model(name).to(dev)
    b = make_config_batch(name)
    targets = make_targets(int(b.natoms.shape[0]))
    step_tables, oracle_tables = igso3_tables()
    bd = b.clone().to(dev)
    eng = m.engine(dev)
    eng.build_graph(bd)
    graph = graph_from_export(eng)
    ei = graph[0]
    indeg = torch.bincount(ei[1], minlength=b.pos.shape[0])
    if name in ("ragged", "ragged_bare", "narrow_basis", "isolated"):
        assert int((ei[0] == ei[1]).sum()) > 0, "no self-image edge"
    if name == "isolated":
        assert int(indeg[int(b.natoms[:3].sum()) - 1]) == 0, "the lifted atom still has edges"
    if name == "hub":
        assert int(indeg.max()) > 256, int(indeg.max())
    if name == "mixed_csr":
        assert int(b.natoms.max()) > 256 and int(b.natoms.min()) < 64
    if name == "big_adsorbate":
        assert int((b.tags[: int(b.natoms[0])] == 2).sum()) > 64
    ref = oracle_loss_and_grads(m, b, targets, oracle_tables, graph=graph)
    _DEVICE_CASES[name] = (m, bd, targets, ref, step_tables)
    return _DEVICE_CASES[name]


def measure_configuration(name, dev="cuda:0"):
    """PaiNNTrainStep.loss_and_grad of a configuration against the float64 oracle: a dict of plain figures (relative errors
    of loss, terms, both outputs, every gradient; what must be exactly zero; the error of the doubled gradients after a
    second accumulating call).  The step reads its ADF_TRAIN_* switches at construction."""
    from adsorbdiff_amd.train_step import PaiNNTrainStep
    from tests.helpers import rel_err

    m, bd, targets, ref, step_tables = device_case(name, dev)
    step = PaiNNTrainStep(m, dev, igso3=step_tables)
    step.zero_grad()
    loss = step.loss_and_grad(bd, targets).double().cpu()
    figs = {"name": name, "grads": {}, "unused_with_grad": [], "missing": []}
    figs["loss"] = abs(float(loss[0]) - float(ref["loss"])) / abs(float(ref["loss"]))
    figs["terms"] = float(((loss[1:] - ref["terms"]).abs() / ref["terms"].abs()).max())
    figs["out1"] = rel_err(step.last_outputs[0].cpu(), ref["out1"])
    figs["out2"] = rel_err(step.last_outputs[1].cpu(), ref["out2"])
    first = {}
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        g = ref["grads"][k]
        if g is None:
            if p.grad is not None:
                figs["unused_with_grad"].append(k)
            continue
        if p.grad is None:
            figs["missing"].append(k)
            continue
        first[k] = p.grad.clone()
        figs["grads"][k] = rel_err(p.grad.cpu(), g)
    absent = absent_embedding_rows(m, bd)
    figs["absent_rows"] = int(absent.sum())
    figs["absent_embedding_max"] = float(first["atom_emb.embeddings.weight"].cpu()[absent].abs().max())
    step.loss_and_grad(bd, targets)   # no zero_grad: every gradient doubles
    figs["doubling"] = max(rel_err(dict(m.named_parameters())[k].grad, 2 * g1) for k, g1 in first.items())
    figs["worst_grad"], figs["worst_grad_name"] = max((e, k) for k, e in figs["grads"].items())
    return figs


def assert_configuration(figs, label=""):
    """The bounds of the fixture tests: loss, its terms and both outputs 1e-5; every gradient 1e-4 relative (the parity
    budget); out_energy.* without a gradient, rows of absent elements exactly zero; doubling to 1e-6."""
    tag = (figs["name"], label)
    assert figs["loss"] < 1e-5 and figs["terms"] < 1e-5, (tag, figs["loss"], figs["terms"])
    assert figs["out1"] < 1e-5 and figs["out2"] < 1e-5, (tag, figs["out1"], figs["out2"])
    assert not figs["unused_with_grad"] and not figs["missing"], (tag, figs["unused_with_grad"], figs["missing"])
    bad = {k: e for k, e in figs["grads"].items() if not e < 1e-4}
    assert not bad, (tag, bad)
    assert figs["absent_rows"] > 0 and figs["absent_embedding_max"] == 0.0, (tag, figs["absent_embedding_max"])
    assert figs["doubling"] < 1e-6, (tag, figs["doubling"])


def describe(figs, label=""):
    return (f"{figs['name']} [{label}]: loss {figs['loss']:.1e} terms {figs['terms']:.1e} out1 {figs['out1']:.1e} "
            f"out2 {figs['out2']:.1e} worst gradient {figs['worst_grad']:.2e} ({figs['worst_grad_name']}) "
            f"doubling {figs['doubling']:.1e}")
