"""The S2EF training step of the force field on the device: the two new kernels on their own against float64 torch (the
4 * e32 rule and the sentinel frames of tests/test_gpu_train_ops.py), the whole step against the reference's loss and autograd
(tests/golden/s2ef_train.npz) and against the float64 oracle at ragged shapes (tests/helpers_s2ef_train.py) in both
arithmetic modes, the energy-only model, ``ForcesTrainer.train_step`` against torch's AdamW / clip / EMA, and two ranks."""
import ctypes
import json
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_s2ef_train as HS
from tests.helpers import rel_err
from tests.test_gpu_train_ops import Guarded, check, dev, gen, ok, ops, s

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
F = torch.nn.functional


# ------------------------------------------------------------------------------------------------ the loss kernel alone
def _loss_case(name):
    """Inputs of a case: predictions, targets, fixed (or None), system sizes, normalizers, coefficients, counts."""
    g = gen(41, len(name), sum(map(ord, name)))
    sizes = {"ragged": (40, 8, 64, 22, 130), "single": (37,), "all_fixed_system": (12, 30, 7), "fixed_absent": (40, 8, 64),
             "forces_absent": (40, 8, 64), "zero_residual": (9, 70, 3), "counts": (40, 8, 64, 22), "all_atoms": (40, 8, 64)}[name]
    B, N = len(sizes), sum(sizes)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    c = dict(sizes=sizes, batch=batch, free_only=1, counts=None, ne=(-1.5, 2.3), nf=(0.25, 1.7), ce=2.0, cf=100.0)
    c["e_pred"], c["f_pred"] = torch.randn(B, generator=g) * 3.0, torch.randn(N, 3, generator=g)
    c["e_tgt"], c["f_tgt"] = torch.randn(B, generator=g) * 5.0, torch.randn(N, 3, generator=g) * 2.0
    c["fixed"] = (torch.rand(N, generator=g) < 0.4).long()
    if name == "all_fixed_system":
        c["fixed"][batch == 1] = 1
    if name == "fixed_absent":
        c["fixed"] = None
    if name == "all_atoms":
        c["free_only"] = 0
    if name == "forces_absent":
        c["f_pred"] = None
    if name == "counts":
        c["counts"] = (11, 301, 2)
    if name == "zero_residual":
        # mean 0.5, std 2 and predictions on a 1/1024 grid: target = mean + std * prediction is exact in float32, and so
        # is the zero residual of system 1 and of three atoms (one of them fixed)
        c["ne"], c["nf"] = (0.5, 2.0), (0.5, 2.0)
        c["e_pred"], c["f_pred"] = (c["e_pred"] * 1024).round() / 1024, (c["f_pred"] * 1024).round() / 1024
        c["e_tgt"][1] = 0.5 + 2.0 * c["e_pred"][1]
        rows = torch.tensor([0, 20, 81])
        c["fixed"][rows] = torch.tensor([0, 1, 0])
        c["fixed"][1] = 0
        c["f_tgt"][rows] = 0.5 + 2.0 * c["f_pred"][rows]
    return c


def _run_loss_kernel(c, rows=None):
    """adf_op_s2ef_loss on a case (``rows``: only that system, alone) -> loss [3], dE, dF (or None), metrics [2] in frames."""
    sizes = c["sizes"] if rows is None else (c["sizes"][rows],)
    sel = slice(None) if rows is None else (c["batch"] == rows)
    bsel = slice(None) if rows is None else slice(rows, rows + 1)
    B, N = len(sizes), sum(sizes)
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(sizes), 0).to(torch.int32)
    ep, et, offd = dev(c["e_pred"][bsel]), dev(c["e_tgt"][bsel]), dev(off, torch.int32)
    fp = dev(c["f_pred"][sel]) if c["f_pred"] is not None else None
    ft = dev(c["f_tgt"][sel])
    fx = dev(c["fixed"][sel], torch.int32) if c["fixed"] is not None else None
    cnt = torch.tensor(c["counts"], dtype=torch.int64, device=DEV) if c["counts"] is not None else None
    loss, dE, dF, met = Guarded(1, 3), Guarded(B, 1), Guarded(N, 3), Guarded(1, 2)
    lib = ops().lib
    cf = ctypes.c_float
    ok(lib.adf_op_s2ef_loss(ep.data_ptr(), fp.data_ptr() if fp is not None else None, et.data_ptr(), ft.data_ptr(),
                            fx.data_ptr() if fx is not None else None, offd.data_ptr(), B, c["free_only"], cf(c["ne"][0]),
                            cf(c["ne"][1]), cf(c["nf"][0]), cf(c["nf"][1]), cf(c["ce"]), cf(c["cf"]),
                            cnt.data_ptr() if cnt is not None else None, loss.ptr, dE.ptr, dF.ptr if fp is not None else None,
                            met.ptr, ops().scratch(int(lib.adf_op_s2ef_loss_scratch(B))).data_ptr(), s()))
    torch.cuda.synchronize()
    got_dF = dF.result() if fp is not None else None
    if fp is None:
        assert bool(torch.isnan(dF.view).all()), "dF must stay untouched without force predictions"
    return loss.result().reshape(3), dE.result().reshape(B), got_dF, met.result().reshape(2)


LOSS_CASES = ["ragged", "single", "all_fixed_system", "fixed_absent", "forces_absent", "zero_residual", "counts", "all_atoms"]


@pytest.mark.parametrize("name", LOSS_CASES)
def test_s2ef_loss_kernel_vs_float64_torch(name):
    """loss, its terms, dE, dF and the two metrics against the float64 restatement (tests/helpers_s2ef_train.s2ef_loss and
    torch.autograd): at most 4 * e32, e32 the error of the same expression in float32 torch; exact where e32 is 0 (the
    zero gradients at a zero residual and outside S).  Two runs are bit-equal."""
    c = _loss_case(name)
    loss, dE, dF, met = _run_loss_kernel(c)
    again = _run_loss_kernel(c)
    assert torch.equal(loss, again[0]) and torch.equal(dE, again[1]) and torch.equal(met, again[3])
    assert dF is None or torch.equal(dF, again[2])
    out = []
    for dt in (torch.float64, torch.float32):
        ep = c["e_pred"].to(dt).requires_grad_(True)
        fp = c["f_pred"].to(dt).requires_grad_(True) if c["f_pred"] is not None else None
        et, ft = c["e_tgt"].to(dt), c["f_tgt"].to(dt)
        l, le, lf = HS.s2ef_loss(ep, fp, et, ft, c["fixed"], c["ne"], c["nf"], c["ce"], c["cf"], bool(c["free_only"]), c["counts"])
        grads = torch.autograd.grad(l, [ep] + ([fp] if fp is not None else []))
        mt = HS.metrics(ep.detach(), None if fp is None else fp.detach(), et, ft, c["fixed"], c["ne"], c["nf"])
        out.append((torch.stack([l.detach(), le.detach(), lf.detach()]).reshape(3, 1), grads[0].reshape(-1, 1),
                    grads[1] if fp is not None else None, torch.stack(list(mt)).reshape(2, 1)))
    B, N = len(c["sizes"]), sum(c["sizes"])
    shape = (name, B, N)
    check("s2ef_loss", shape, loss.reshape(3, 1), out[0][0], out[1][0], terms=B + N)
    check("s2ef_loss_dE", shape, dE.reshape(-1, 1), out[0][1], out[1][1])
    check("s2ef_loss_metrics", shape, met.reshape(2, 1), out[0][3], out[1][3], terms=3 * N)
    if dF is not None:
        check("s2ef_loss_dF", shape, dF, out[0][2], out[1][2])
        if c["fixed"] is not None and c["free_only"]:
            assert float(dF[c["fixed"] == 1].abs().max()) == 0.0
    else:
        assert float(loss[2]) == 0.0 and float(loss[0]) == float(loss[1]) and float(met[1]) == 0.0
    if name == "zero_residual":
        assert float(dE[1]) == 0.0 and float(dF[[0, 20, 81]].abs().max()) == 0.0 and float(dF[1].abs().max()) > 0.0
    if name == "all_fixed_system":
        assert float(dF[c["batch"] == 1].abs().max()) == 0.0 and float(dE[1]) != 0.0


def test_s2ef_loss_with_every_atom_of_the_batch_fixed_is_nan_like_the_reference():
    """No atom in S and no counts supplied: M = 0, the force term is 0 * W / 0 = NaN as DDPLoss's
    loss * world_size / num_samples is (float64 torch gives the same), the energy term and dE stay finite; the trainer
    skips such a step."""
    c = _loss_case("fixed_absent")
    c["fixed"] = torch.ones(sum(c["sizes"]), dtype=torch.long)
    loss, dE, dF, met = _run_loss_kernel(c)
    l, le, lf = HS.s2ef_loss(c["e_pred"].double(), c["f_pred"].double(), c["e_tgt"].double(), c["f_tgt"].double(), c["fixed"],
                             c["ne"], c["nf"], c["ce"], c["cf"], True, None)
    assert bool(torch.isnan(l)) and bool(torch.isnan(lf)) and bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[2]))
    assert abs(float(loss[1]) - float(le)) < 1e-6 * float(le) and bool(torch.isfinite(dE).all()) and float(met[1]) == 0.0
    assert not bool(torch.isfinite(dF).all()) or float(dF.abs().max()) == 0.0


def test_s2ef_loss_rows_of_a_system_do_not_depend_on_its_batch():
    """With the divisors supplied, a system's dE / dF are bit-equal when it is alone and when it sits inside a batch."""
    c = _loss_case("ragged")
    c["counts"] = (len(c["sizes"]), int((c["fixed"] == 0).sum()), 1)
    _, dE, dF, _ = _run_loss_kernel(c)
    own = _run_loss_kernel(dict(c, counts=None))
    assert torch.equal(dE, own[1]) and torch.equal(dF, own[2])      # the supplied divisors are the batch's own
    for b in range(len(c["sizes"])):
        _, dE1, dF1, _ = _run_loss_kernel(c, rows=b)
        assert torch.equal(dE1, dE[b:b + 1]) and torch.equal(dF1, dF[c["batch"] == b]), b


# ------------------------------------------------------------------------------------------------ the energy head backward
@pytest.mark.parametrize("N,H2", [(1, 64), (3, 96), (63, 64), (64, 256), (65, 96), (257, 256), (4099, 64), (4099, 256), (1000, 96)])
def test_energy_head_backward_vs_float64_autograd(N, H2):
    """adf_op_energy_head_bwd (+ adf_op_linear_bwd for out_energy.0) against float64 autograd of Linear -> ScaledSiLU ->
    Linear -> per-system sum with an upstream dE [B]: d(he0), dW2, db2 by the 4 * e32 rule, out_energy.0's gradients at the
    products' 1e-5.  Row counts around the 64-row chunk (below one chunk, one row over), column counts that are not a
    multiple of the 64-column tile; accumulating and overwriting; two runs bit-equal; the dE == 1 data-gradient-only form."""
    from oracle import painn_oracle as O

    g = gen(43, N, H2)
    H = 2 * H2
    B = max(1, min(7, N // 3))
    batch = torch.sort(torch.randint(0, B, (N,), generator=g)).values
    x = torch.randn(N, H, generator=g)
    W0, b0 = torch.randn(H2, H, generator=g) / math.sqrt(H), torch.randn(H2, generator=g) * 0.3
    w2, b2 = torch.randn(1, H2, generator=g) / math.sqrt(H2), torch.randn(1, generator=g)
    dE = torch.randn(B, generator=g) * 2.0
    xd, W0d, b0d, w2d, dEd, bd = dev(x), dev(W0), dev(b0), dev(w2), dev(dE), dev(batch, torch.int32)
    he0 = ops().linear(xd, W0d, b0d, N, H2, H)
    torch.cuda.synchronize()
    he0_c = he0.cpu()
    lib = ops().lib

    def run(acc, init_w=None, init_b=None, with_dE=True, params=True):
        dhe = Guarded(N, H2)
        dW2 = Guarded(1, H2, init=init_w) if params else None
        db2 = Guarded(1, 1, init=init_b) if params else None
        ok(lib.adf_op_energy_head_bwd(he0.data_ptr(), w2d.data_ptr(), dEd.data_ptr() if with_dE else None,
                                      bd.data_ptr() if with_dE else None, dhe.ptr, dW2.ptr if params else None,
                                      db2.ptr if params else None, 1 if acc else 0, N, H2,
                                      ops().scratch(int(lib.adf_op_energy_head_bwd_scratch(N, H2))).data_ptr() if params else None,
                                      s()))
        return dhe.result(), (dW2.result().reshape(-1) if params else None), (db2.result().reshape(-1) if params else None)

    def fn(h, w, b):
        per_atom = F.linear(O.ssilu(h), w, b).squeeze(1)
        return torch.zeros(B, dtype=h.dtype).index_add_(0, batch, per_atom)

    res = []
    for dt in (torch.float64, torch.float32):
        xs = [he0_c.to(dt).requires_grad_(True), w2.to(dt).requires_grad_(True), b2.to(dt).requires_grad_(True)]
        res.append(torch.autograd.grad(fn(*xs), xs, dE.to(dt)))
    dhe, dW2, db2 = run(False)
    again = run(False)
    assert torch.equal(dhe, again[0]) and torch.equal(dW2, again[1]) and torch.equal(db2, again[2])
    shape = (N, H2, B)
    check("energy_head_bwd_dhe0", shape, dhe, res[0][0], res[1][0])
    check("energy_head_bwd_dW2", shape, dW2, res[0][1], res[1][1], vector=True)
    check("energy_head_bwd_db2", shape, db2.reshape(1, 1), res[0][2].reshape(1, 1), res[1][2].reshape(1, 1), terms=N)
    # accumulating into what is there
    iw, ib = torch.randn(H2, generator=g), torch.randn(1, generator=g)
    _, aW2, ab2 = run(True, iw, ib)
    assert torch.equal(aW2, iw + dW2) and torch.equal(ab2, ib + db2)
    # dE == 1, data gradient only: the seed of the energy-gradient forces
    seed, _, _ = run(False, with_dE=False, params=False)
    r = []
    for dt in (torch.float64, torch.float32):
        h = he0_c.to(dt).requires_grad_(True)
        r.append(torch.autograd.grad(fn(h, w2.to(dt), b2.to(dt)).sum(), h)[0])
    check("energy_head_bwd_seed", shape, seed, r[0], r[1])
    # out_energy.0 through the existing product backward, data gradient accumulated into dx
    dx0 = torch.randn(N, H, generator=g)
    dxd, dW0, db0 = dev(dx0), torch.zeros(H2, H, device=DEV), torch.zeros(H2, device=DEV)
    ops().linear_bwd(xd, W0d, dev(dhe), N, H2, H, dW0, db0, dA=dxd, acc_dA=True)
    torch.cuda.synchronize()
    x64, W64, b64 = (t.double().requires_grad_(True) for t in (x, W0, b0))
    gx, gW, gb = torch.autograd.grad(fn(F.linear(x64, W64, b64), w2.double(), b2.double()), [x64, W64, b64], dE.double())
    for got, ref, what in ((dxd.cpu() - dx0, gx, "dx"), (dW0.cpu(), gW, "dW0"), (db0.cpu(), gb, "db0")):
        e = rel_err(got, ref)
        print(f"energy_head out_energy.0 {what} {shape}: {e:.2e}")
        assert e < 1e-5, (what, shape, e)


# ------------------------------------------------------------------------------------------------ the whole step
def test_step_vs_reference_loss_and_autograd():
    """tests/golden/s2ef_train.npz (the reference's DDPLoss / _compute_loss and float64 autograd): loss, terms and outputs
    1e-5, every parameter's gradient within the 1e-4 training budget (tests/helpers_train.assert_configuration)."""
    figs = HS.measure_fixture(DEV)
    print("S2EF " + HS.describe(figs, "fixture [default]"))
    HS.assert_step(figs, "fixture")


@pytest.mark.parametrize("name", HS.CONFIG_NAMES)
def test_step_at_ragged_shapes_vs_float64_oracle(name):
    """The ragged configurations of tests/helpers_train.CONFIGS with S2EF targets, against the float64 oracle on the
    engine's exported graph: same budget."""
    figs = HS.measure_configuration(name, DEV)
    print("S2EF " + HS.describe(figs, f"{name} [default]"))
    HS.assert_step(figs, name)


_EXACT_F32_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, {root!r})
from tests import helpers_s2ef_train as HS
figs = HS.measure_fixture("cuda:0"); figs["name"] = "fixture"
print("FIGS " + json.dumps(figs), flush=True)
for name in HS.CONFIG_NAMES:
    print("FIGS " + json.dumps(HS.measure_configuration(name, "cuda:0")), flush=True)
"""


def test_step_with_the_exact_f32_products():
    """The fixture and the ragged table once more under ADF_TRAIN_GEMM=f32 and ADF_WGRAD=f32, the second arithmetic mode
    the denoiser's step is tested in (both switches are read once per process, hence the child)."""
    env = dict(os.environ, ADF_TRAIN_GEMM="f32", ADF_WGRAD="f32")
    for k in ("ADF_TRAIN_RBF_WGRAD", "ADF_TRAIN_MSG_BWD", "ADF_TRAIN_MSG"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-c", _EXACT_F32_SCRIPT.format(root=str(ROOT))], env=env, capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    seen = []
    for line in res.stdout.splitlines():
        if line.startswith("FIGS "):
            figs = json.loads(line[5:])
            print("S2EF " + HS.describe(figs, f"{figs['name']} [exact f32 products]"))
            HS.assert_step(figs, figs["name"])
            seen.append(figs["name"])
    assert seen == ["fixture"] + HS.CONFIG_NAMES


def test_energy_only_model():
    """regress_forces=False: the loss is the energy term alone, the gradients match the oracle, and no out_forces key
    appears."""
    figs = HS.measure_configuration("ragged", DEV, regress_forces=False)
    print("S2EF " + HS.describe(figs, "ragged, energy only"))
    HS.assert_step(figs, "energy only")
    assert figs["grads"] and not any(k.startswith("out_forces") for k in figs["grads"])
    m = HS.make_energy_only_model("ragged").to(DEV)
    assert not any(k.startswith("out_forces") for k, _ in m.named_parameters())
    assert set(m(HS.make_config_batch("ragged").to(DEV))) == {"energy"}


# ------------------------------------------------------------------------------------------------ ForcesTrainer.train_step
def _trainer(lr, **kw):
    fx, m, b, step_kw = HS.fixture_case()
    tr = ForcesTrainer(m, device=DEV, normalizers=step_kw["normalizers"])
    tr.setup_training(lr, energy_coefficient=step_kw["energy_coefficient"], force_coefficient=step_kw["force_coefficient"], **kw)
    return fx, tr, b.to(DEV), step_kw


def test_ten_training_steps_match_torch_adamw_clip_ema_on_oracle_gradients():
    """Ten steps on the fixture batch; parameters, EMA shadow and the gradient norm against torch.optim.AdamW +
    clip_grad_norm_ + the EMA mirror driven by the float64 oracle's gradients.  Tolerance of
    test_fused_adamw_matches_torch_adamw_clip_ema: 2e-6 on the parameters, 1e-5 on the gradient norm.

    The learning rate is 1e-6, by this reasoning: an AdamW update is lr * m / sqrt(v), sign-like in the gradient, so an
    element whose gradient is smaller than the step's error moves by up to 2 lr per step in the wrong direction whatever the
    error's size.  Within the 1e-4 gradient budget a fraction of about 1e-4 of the elements may do so; over ten steps that
    is a parameter error of sqrt(1e-4) * 2 lr * 10 = 0.2 lr against parameters of magnitude 0.1, i.e. 2 lr relative:
    2e-6 at lr = 1e-6.  Ten such steps move the parameters by 1e-4 relative, fifty times the tolerance."""
    from adsorbdiff_amd.exponential_moving_average import ExponentialMovingAverage

    lr, wd, clip, decay = 1e-6, 0.001, 10.0, 0.999
    fx, tr, bd, kw = _trainer(lr, weight_decay=wd, clip_grad_norm=clip, ema_decay=decay)
    m = tr._unwrapped_model
    _, ref, b, _ = HS.fixture_case()
    graph = HS.engine_graph(m, bd)
    no_decay = set(ref.no_weight_decay())
    groups = [{"params": [p for n, p in ref.named_parameters() if p.requires_grad and n in no_decay], "weight_decay": 0.0},
              {"params": [p for n, p in ref.named_parameters() if p.requires_grad and n not in no_decay], "weight_decay": wd}]
    topt = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    ema_ref = ExponentialMovingAverage(ref.parameters(), decay)
    start = {k: p.detach().clone() for k, p in m.named_parameters()}
    losses = []
    for it in range(10):
        out = tr.train_step(bd)
        assert not out["skipped"] and not out["stop"] and out["metrics"].shape == (2,)
        losses.append(float(out["loss"][0]))
        r = HS.oracle_loss_and_grads(ref, b, graph, **kw)
        for n, q in ref.named_parameters():
            q.grad = r["grads"][n].float() if q.requires_grad else None
        gn_ref = torch.nn.utils.clip_grad_norm_([q for q in ref.parameters() if q.grad is not None], max_norm=clip)
        topt.step()
        ema_ref.update()
        assert abs(float(out["grad_norm"]) - float(gn_ref)) < 1e-5 * float(gn_ref), (it, float(out["grad_norm"]), float(gn_ref))
        assert abs(losses[-1] - float(r["loss"])) < 1e-5 * float(r["loss"])
    worst = max((rel_err(p.detach().cpu(), q.detach()), n) for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()))
    moved = max(rel_err(p.detach(), start[n]) for n, p in m.named_parameters() if p.requires_grad)
    worst_ema = max(rel_err(s1.cpu(), s2) for s1, s2 in zip(tr.ema.shadow_params, ema_ref.shadow_params))
    print(f"S2EF ten steps at lr {lr}: gradient norm {float(gn_ref):.4g} (clip {clip}), parameters moved up to {moved:.1e}, "
          f"worst parameter error {worst[0]:.2e} ({worst[1]}), worst EMA error {worst_ema:.2e}, loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert float(gn_ref) > clip, "the clip is not active: choose a smaller clip_grad_norm"
    assert worst[0] < 2e-6 and worst_ema < 2e-6, (worst, worst_ema)
    assert tr.step == 10


def test_training_lowers_the_loss_and_predict_sees_the_trained_weights():
    """Ten steps at lr = 1e-3 on the fixture batch: the loss after them is lower than at step 0; ``predict`` differs from
    before and equals, bit for bit, a fresh model's output with the same (EMA) weights."""
    fx, tr, bd, kw = _trainer(1e-3)
    before = tr.predict(bd.clone())
    loss0 = float(tr.train_step(bd)["loss"][0])
    for _ in range(9):
        tr.train_step(bd)
    tr.train_engine.zero_grad()
    after_loss = float(tr.train_engine.loss_and_grad(bd)[0])
    print(f"S2EF loss at step 0 {loss0:.4f}, after ten steps {after_loss:.4f}")
    assert after_loss < loss0
    after = tr.predict(bd.clone())
    assert not torch.equal(after["energy"], before["energy"]) and not torch.equal(after["forces"], before["forces"])
    _, fresh, _, _ = HS.fixture_case()
    fresh = fresh.to(DEV)
    with torch.no_grad():
        for p, sh in zip([p for p in fresh.parameters() if p.requires_grad], tr.ema.shadow_params):
            p.copy_(sh)
    want = ForcesTrainer(fresh, device=DEV, normalizers=kw["normalizers"]).predict(bd.clone())
    assert torch.equal(after["energy"], want["energy"]) and torch.equal(after["forces"], want["forces"])


def test_non_finite_loss_skips_the_update():
    """A NaN target makes the loss NaN: the step is skipped, parameters, moments and EMA shadow bit-unchanged; the next
    good batch trains."""
    fx, tr, bd, kw = _trainer(1e-3)
    tr.train_step(bd)
    m = tr._unwrapped_model
    snap = [p.detach().clone() for p in m.parameters()]
    shadow = [t.clone() for t in tr.ema.shadow_params]
    moments = [(e[2].clone(), e[3].clone()) for e in tr.optimizer.entries]
    bad = bd.clone()
    bad.energy[1] = float("nan")
    out = tr.train_step(bad)
    assert out["skipped"] and not out["stop"] and out["grad_norm"] is None and bool(torch.isnan(out["loss"][0]))
    assert all(torch.equal(a, p.detach()) for a, p in zip(snap, m.parameters()))
    assert all(torch.equal(a, t) for a, t in zip(shadow, tr.ema.shadow_params))
    assert all(torch.equal(a, e[2]) and torch.equal(b, e[3]) for (a, b), e in zip(moments, tr.optimizer.entries))
    assert tr.step == 1
    out = tr.train_step(bd)
    assert not out["skipped"] and tr.step == 2 and not all(torch.equal(a, p.detach()) for a, p in zip(snap, m.parameters()))


# ------------------------------------------------------------------------------------------------ two ranks
WORKER = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_s2ef_train as HS

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
fx, m, full, kw = HS.fixture_case()
tr = ForcesTrainer(m, device="cuda:0", normalizers=kw["normalizers"])
tr.setup_training(0.0, weight_decay=0.0, clip_grad_norm=0.0, ema_decay=0.0, energy_coefficient=kw["energy_coefficient"],
                  force_coefficient=kw["force_coefficient"])
data = full.to_data_list()
lo, hi = (0, 1) if rank == 0 else (1, len(data))          # one system on rank 0, three on rank 1
mine = Batch.from_data_list(data[lo:hi])
a0, a1 = int(full.natoms[:lo].sum()), int(full.natoms[:hi].sum())
mine.energy, mine.forces = full.energy[lo:hi].clone(), full.forces[a0:a1].clone()
out = tr.train_step(mine)                                 # lr = 0: only the averaged gradients matter
if rank == 0:
    torch.save({"grads": {k: p.grad.cpu() for k, p in m.named_parameters() if p.requires_grad},
                "systems": int(mine.natoms.numel()), "free": int((mine.fixed == 0).sum())}, sys.argv[2])
dist.barrier()
dist.destroy_process_group()
"""


def run_two_ranks(tmp_path, worker=WORKER):
    script = tmp_path / "worker.py"
    script.write_text(worker)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), str(ROOT), str(tmp_path / "g.pt")], env=env))
    assert [p.wait(timeout=600) for p in procs] == [0, 0]
    return torch.load(tmp_path / "g.pt")


def two_rank_errors(got):
    """(worst error against the fixture's full-batch reference gradients, worst against a single-process full-batch step)"""
    fx, m, b, kw = HS.fixture_case()
    from adsorbdiff_amd.train_step import PaiNNS2EFTrainStep

    m = m.to(DEV)
    step = PaiNNS2EFTrainStep(m, DEV, **kw)
    step.zero_grad()
    step.loss_and_grad(b.to(DEV))
    single = max(rel_err(got["grads"][k], p.grad.cpu()) for k, p in m.named_parameters() if p.requires_grad)
    return max(HS.fixture_gradient_errors(fx, got["grads"]).values()), single


def test_two_rank_training_step_equals_full_batch(tmp_path):
    """DDP semantics with a ragged split: rank 0 holds one system, rank 1 the other three (other system counts and other
    free-atom counts), sharing cuda:0 under gloo.  After the all-reduce of the counts and the bucketed all-reduce of the
    gradients every rank holds the gradient of the full-batch loss: the reference's autograd gradients and the
    single-process step's, within the 1e-4 of the denoiser's two-rank test.  With local counts in place of the all-reduced
    ones the energy term would be weighted 4 / (2 * 1) and 4 / (2 * 3) per rank instead of 1."""
    got = run_two_ranks(tmp_path)
    fx = HS.fixture_case()[0]
    free = fx["fixed"] == 0
    assert got["systems"] == 1 and got["free"] not in (int(free.sum()) - got["free"], 0)
    vs_fixture, vs_single = two_rank_errors(got)
    print(f"S2EF two ranks: worst gradient error against the fixture {vs_fixture:.2e}, against the single-process step {vs_single:.2e}")
    assert vs_fixture < 1e-4 and vs_single < 1e-4
