"""``EqV2S2EFTrainStep.loss_and_grad`` as a whole against float64 autograd through the pieces of oracle/eqv2_oracle.py
(tests/helpers_eqv2_s2ef_train.reference_step) on a fixed edge list: loss, its terms, energies, forces and metrics to 1e-5;
gradients per group under REL_TOL and per parameter under max(REL_TOL, TIGHT_FACTOR x the float32 oracle's own distance),
printed; the None / zero pattern of the float64 autograd; what is trained is what ``model(batch)`` infers; reproducibility;
the order of ``grads_ready``."""
import pytest
import torch

from tests import helpers_eqv2_s2ef_train as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}
KW = dict(normalizers=S.NORMALIZERS, **S.COEFFICIENTS)

# name -> (graph, model keywords, step keywords, masks?, counts)
CASES = {
    "fixture": ("fixture", {}, {}, False, None),
    "ragged": ("ragged", {}, {}, False, None),
    "energy-only": ("fixture", dict(regress_forces=False), {}, False, None),
    "all-atoms": ("fixture", {}, dict(train_on_free_atoms=False), False, None),
    "lin-ref": ("fixture", dict(use_energy_lin_ref=True), {}, False, None),
    "masks": ("fixture", dict(alpha_drop=0.1, drop_path_rate=0.1), {}, True, None),
    "counts": ("fixture", {}, {}, False, (5, 61, 2)),
}


def setup(name):
    """-> (model on the device, batch on the device, batch, graph (cpu), step, step keywords, masks (cpu), counts)."""
    from adsorbdiff_amd.eqv2_train_step import EqV2S2EFTrainStep

    kind, mkw, skw, masked, counts = CASES[name]
    if kind == "ragged":
        m = S.ragged_model(**mkw)
        b, ei, vec = S.ragged_case()
    else:
        m = S.small_train_model(**mkw)
        b, ei, vec, _ = S.fixture_case()
    m = m.to(DEV)
    bd = b.clone().to(DEV)
    eng = m.engine(DEV)
    eng.set_edges(ei, vec)
    _, src, dst, v, _ = eng.export_graph(bd)
    graph = (torch.stack([src.long().cpu(), dst.long().cpu()]), v.cpu())
    assert torch.equal(graph[0], ei) and torch.equal(graph[1], vec)
    masks = None
    if masked:
        E, B = ei.shape[1], int(b.natoms.numel())
        gen = torch.Generator().manual_seed(77)
        masks = {"alpha": [(torch.rand(E, m.num_heads, generator=gen) >= 0.1).float() for _ in range(m.num_layers)],
                 "path": torch.tensor([[[1.0, 0.0], [1.0, 1.0]], [[0.0, 1.0], [1.0, 1.0]]])[: m.num_layers, :, :B]}
        assert all(float(a.min()) == 0.0 for a in masks["alpha"])
    kw = dict(KW, **skw)
    return m, bd, b, graph, EqV2S2EFTrainStep(m, DEV, **kw), kw, masks, counts


def references(name, m, b, graph, kw, masks, counts):
    if name not in _REF:
        _REF[name] = tuple(S.reference_step(m, b, graph, dt, masks=masks, counts=counts, **kw) for dt in (torch.float64, torch.float32))
    return _REF[name]


def run(step, m, bd, masks, counts, grads_ready=None):
    dmasks = None if masks is None else {"alpha": [a.to(DEV) for a in masks["alpha"]], "path": masks["path"].to(DEV)}
    dcounts = None if counts is None else torch.tensor(counts, dtype=torch.int64, device=DEV)
    step.zero_grad()
    loss = step.loss_and_grad(bd, grads_ready=grads_ready, counts=dcounts, masks=dmasks)
    return loss, {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("name", list(CASES))
def test_whole_step_against_float64_autograd(name):
    m, bd, b, graph, step, kw, masks, counts = setup(name)
    ref64, ref32 = references(name, m, b, graph, kw, masks, counts)
    if name == "masks":
        plain = S.reference_step(m, b, graph, **kw)
        # (the loss is dominated by the seeded noise of the targets: the predictions show what the masks do)
        assert S.frob(ref64["forces"], plain["forces"]) > 1e-2 and S.frob(ref64["energy"], plain["energy"]) > 1e-4, "the masks change nothing"
    if name == "counts":
        own = S.reference_step(m, b, graph, **kw)
        assert abs(float(ref64["loss"][0] - own["loss"][0])) > 1e-2 * abs(float(own["loss"][0])), "the divisors change nothing"
    seen = []
    loss, grads = run(step, m, bd, masks, counts, grads_ready=seen.extend)
    assert step.norm == {"energy": (-0.7, 1.9), "forces": (0.15, 2.1)}   # normalizers that are not (0, 1)
    S.check_step(name, grads, loss, step.last_outputs, step.metrics, ref64, ref32, m)
    # every trainable parameter is announced exactly once: heads and final norm, blocks last to first, embeddings
    assert sorted(seen) == sorted(grads) and len(set(seen)) == len(seen)
    order = [S.group_of(n) for n in seen]
    first = {g_: order.index(g_) for g_ in set(order)}
    last = {g_: len(order) - 1 - order[::-1].index(g_) for g_ in set(order)}
    heads = [g_ for g_ in ("force_block.", "energy_block.", "norm.") if g_ in first]
    assert ("force_block." in first) == bool(m.regress_forces)
    assert max(last[g_] for g_ in heads) < first[f"blocks.{m.num_layers - 1}."]
    assert last[f"blocks.{m.num_layers - 1}."] < first["blocks.0."] <= last["blocks.0."] < min(first["sphere_embedding."], first["edge_degree_embedding."])
    # rows of the embedding tables for elements the batch does not hold: exactly zero
    absent = torch.ones(m.max_num_elements, dtype=torch.bool)
    absent[bd.atomic_numbers.cpu().long()] = False
    for k, g in grads.items():
        if k.endswith("embedding.weight") and g.shape[0] == m.max_num_elements:
            assert float(g.cpu()[absent].abs().max()) == 0.0, k
    # a second accumulating call doubles every gradient
    dmasks = None if masks is None else {"alpha": [a.to(DEV) for a in masks["alpha"]], "path": masks["path"].to(DEV)}
    step.loss_and_grad(bd, counts=None if counts is None else torch.tensor(counts, dtype=torch.int64, device=DEV), masks=dmasks)
    for k, p in m.named_parameters():
        if p.requires_grad and float(grads[k].norm()) > 0.0:
            assert S.frob(p.grad, 2 * grads[k]) < 1e-6, k


def test_what_is_trained_is_what_is_inferred():
    """eval(): the step's outputs against ``model(batch)`` in exact-f32 arithmetic on the same edge list."""
    for name in ("fixture", "ragged"):
        m, bd, b, graph, step, kw, _, _ = setup(name)
        m.eval()
        step.zero_grad()
        step.loss_and_grad(bd)
        e_t, f_t = step.last_outputs
        eng = m.engine(DEV)
        eng.set_arithmetic(True)
        eng.set_edges(*graph)
        out = m(bd)
        fe, ff = S.frob(e_t, out["energy"]), S.frob(f_t, out["forces"])
        worst = float((f_t - out["forces"]).abs().max() / out["forces"].norm(dim=1).max())
        print(f"{name}: training forward against the inference forward: energy {fe:.2e} forces {ff:.2e} worst atom {worst:.2e}")
        assert fe < S.REL_TOL and ff < S.REL_TOL and worst < S.REL_TOL


def test_two_calls_give_the_same_bits():
    m, bd, b, graph, step, kw, masks, counts = setup("masks")
    runs = [run(step, m, bd, masks, counts) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    # drawn masks: a function of (seed, step) alone
    drawn = []
    for s_ in (5, 5, 6):
        step.mask_seed, step.mask_step = 3, s_
        step.zero_grad()
        drawn.append((step.loss_and_grad(bd).clone(), step.last_masks))
    assert torch.equal(drawn[0][0], drawn[1][0]) and not torch.equal(drawn[0][0], drawn[2][0])
    assert all(torch.equal(a, b_) for a, b_ in zip(drawn[0][1]["alpha"], drawn[1][1]["alpha"])) and step.mask_step == 7


def test_refusals():
    from adsorbdiff_amd.eqv2_train_step import EqV2S2EFTrainStep

    m = S.small_train_model().to(DEV)
    m.proj_drop = 0.1
    with pytest.raises(NotImplementedError, match="proj_drop"):
        EqV2S2EFTrainStep(m, DEV)
    m.proj_drop = 0.0
    step = EqV2S2EFTrainStep(m, DEV)
    b, ei, vec, _ = S.fixture_case()
    with pytest.raises(RuntimeError, match="zero_grad"):
        step.loss_and_grad(b.clone().to(DEV))
    step.zero_grad()
    nob = b.clone().to(DEV)
    del nob.forces
    with pytest.raises(ValueError, match="batch.forces is required"):
        step.loss_and_grad(nob)
