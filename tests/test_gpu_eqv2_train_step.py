"""``EqV2TrainStep.loss_and_grad`` as a whole against float64 autograd through oracle/eqv2_oracle.py on the device's exported
edge list: loss, terms and outputs to 1e-5; gradients per group under 1e-4 and per parameter under max(1e-4, 10 x the
float32 oracle's own distance), printed; unused parameters without a gradient; rows of absent elements exactly zero;
doubling; reproducibility; the order of ``grads_ready``; dropout / drop-path masks."""
import pytest
import torch

from tests import helpers_eqv2_train as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def setup(key):
    """key -> (model on the device, batch on the device, targets, exported graph (cpu), step)."""
    from adsorbdiff_amd.eqv2_train_step import EqV2TrainStep

    name, graph_kind, two_heads, conditional = key
    step_tables, _ = T.igso3_tables()
    if graph_kind == "ragged":
        m = T.train_model(name, two_heads, conditional)
        b, ei, vec = T.ragged_case()
    else:
        m = T.train_model(name, two_heads, conditional, cutoff=T.SPARSE_CUTOFF)
        b, _ = T.sparse_batch()
        b = T.tagged(b)
        ei = vec = None
    if conditional:
        b.energy = torch.tensor([-1.25, 0.5, 2.0][: int(b.natoms.numel())])
    m = m.to(DEV)
    bd = b.clone().to(DEV)
    eng = m.engine(DEV)
    eng.set_edges(ei, vec)
    _, src, dst, v, _ = eng.export_graph(bd)
    graph = (torch.stack([src.long().cpu(), dst.long().cpu()]), v.cpu())
    targets = T.make_targets(int(b.natoms.numel()))
    return m, bd, b, targets, graph, EqV2TrainStep(m, DEV, igso3=step_tables)


def references(key, m, b, targets, graph, masks=None):
    k = (key, masks is not None)
    if k not in _REF:
        _REF[k] = (T.reference_step(m, b, targets, graph, torch.float64, masks), T.reference_step(m, b, targets, graph, torch.float32, masks))
    return _REF[k]


CASES = [("small", "sparse", True, False), ("small", "ragged", True, False), ("mfma", "ragged", True, False),
         ("small", "ragged", False, False), ("small", "sparse", True, True)]


@pytest.mark.parametrize("key", CASES, ids=lambda k: f"{k[0]}-{k[1]}-{'two' if k[2] else 'one'}{'-conditional' if k[3] else ''}")
def test_whole_step_against_float64_autograd(key):
    m, bd, b, targets, graph, step = setup(key)
    ref64, ref32 = references(key, m, b, targets, graph)
    step.zero_grad()
    seen = []
    loss = step.loss_and_grad(bd, targets, grads_ready=seen.extend)
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters() if p.requires_grad}
    label = "-".join(str(x) for x in key)
    T.check_step(label, grads, loss, step.last_outputs + ((None,) if not key[2] else ()), ref64, ref32, m)
    # every trainable parameter with a path to the loss is announced exactly once
    live = sorted(k for k, g in ref64["grads"].items() if g is not None)
    assert sorted(seen) == live and len(set(seen)) == len(seen)
    order = [T.group_of(n) for n in seen]
    first = {g_: order.index(g_) for g_ in set(order)}
    assert first["force_block."] < first[f"blocks.{m.num_layers - 1}."] < first["blocks.0."] < first["sphere_embedding."]
    if key[3]:
        assert float(grads["energy_embedding.weight"].abs().max()) > 0.0
    # rows of the embedding tables for elements the batch does not hold: exactly zero
    Z = bd.atomic_numbers.cpu().long()
    absent = torch.ones(m.max_num_elements, dtype=torch.bool)
    absent[Z] = False
    for k, g in grads.items():
        if g is not None and k.endswith("embedding.weight") and g.shape[0] == m.max_num_elements:
            assert float(g.cpu()[absent].abs().max()) == 0.0, k
    # a second accumulating call doubles every gradient
    step.loss_and_grad(bd, targets)
    for k, p in m.named_parameters():
        if p.requires_grad and grads[k] is not None and float(grads[k].norm()) > 0.0:
            assert T.frob(p.grad, 2 * grads[k]) < 1e-6, k


def test_two_calls_give_the_same_bits():
    key = ("mfma", "ragged", True, False)
    m, bd, b, targets, graph, step = setup(key)
    runs = []
    for _ in range(2):
        step.zero_grad()
        loss = step.loss_and_grad(bd, targets)
        runs.append((loss.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_conditional_model_needs_the_energies():
    key = ("small", "sparse", True, True)
    m, bd, b, targets, graph, step = setup(key)
    del bd.energy
    step.zero_grad()
    with pytest.raises(ValueError, match="data.energy"):
        step.loss_and_grad(bd, targets)


def test_masks():
    """alpha_drop = drop_path_rate = 0.1 with supplied masks against the masked float64 reference; eval() ignores the rates;
    the same (seed, step) draws the same masks."""
    key = ("small", "sparse", True, False)
    m, bd, b, targets, graph, step = setup(key)
    m.alpha_drop, m.drop_path_rate = 0.1, 0.1
    E, B = graph[0].shape[1], int(b.natoms.numel())
    gen = torch.Generator().manual_seed(77)
    masks = {"alpha": [(torch.rand(E, m.num_heads, generator=gen) >= 0.1).float() for _ in range(m.num_layers)],
             "path": torch.tensor([[[1.0, 0.0, 1.0], [1.0, 1.0, 0.0]], [[0.0, 1.0, 1.0], [1.0, 1.0, 1.0]]])[: m.num_layers, :, :B]}
    assert all(float(a.min()) == 0.0 for a in masks["alpha"])
    ref64, ref32 = references(key, m, b, targets, graph, masks)
    plain64, _ = references(key, m, b, targets, graph)
    assert abs(float(ref64["loss"][0] - plain64["loss"][0])) > 1e-3 * abs(float(plain64["loss"][0])), "the masks change nothing"
    dmasks = {"alpha": [a.to(DEV) for a in masks["alpha"]], "path": masks["path"].to(DEV)}
    m.train()
    step.zero_grad()
    loss = step.loss_and_grad(bd, targets, masks=dmasks)
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters() if p.requires_grad}
    T.check_step("masks", grads, loss, step.last_outputs, ref64, ref32, m)
    # eval(): the rates are ignored
    m.eval()
    step.zero_grad()
    loss_eval = step.loss_and_grad(bd, targets)
    assert abs(float(loss_eval[0].cpu()) - float(plain64["loss"][0])) < 1e-5 * abs(float(plain64["loss"][0]))
    assert step.last_masks is None
    # drawn masks: a function of (seed, step) alone; another step draws others
    m.train()
    drawn = []
    for s in (5, 5, 6):
        step.mask_seed, step.mask_step = 3, s
        step.zero_grad()
        drawn.append((step.loss_and_grad(bd, targets).clone(), step.last_masks))
    assert torch.equal(drawn[0][0], drawn[1][0]) and not torch.equal(drawn[0][0], drawn[2][0])
    assert all(torch.equal(a, b_) for a, b_ in zip(drawn[0][1]["alpha"], drawn[1][1]["alpha"]))
    assert torch.equal(drawn[0][1]["path"], drawn[1][1]["path"])
    assert step.mask_step == 7
    keep = torch.cat([a.reshape(-1) for a in drawn[0][1]["alpha"]]).mean()
    assert 0.8 < float(keep) < 0.97


def test_proj_drop_is_refused():
    from adsorbdiff_amd.eqv2_train_step import EqV2TrainStep

    m = T.train_model("small").to(DEV)
    m.proj_drop = 0.1
    with pytest.raises(NotImplementedError, match="proj_drop"):
        EqV2TrainStep(m, DEV)
