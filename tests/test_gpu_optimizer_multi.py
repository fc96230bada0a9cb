"""csrc/optimizer.hip on the device: MultiTensorAdamW against torch.optim.AdamW + clip_grad_norm_ + the EMA mirror in float64,
the ordered gradient norm, the non-finite guard, the state-dict round trip through torch, and the ordered embedding backward."""
import copy
import ctypes as C

import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.exponential_moving_average import ExponentialMovingAverage
from adsorbdiff_amd.train_step import MultiTensorAdamW, reference_param_groups
from tests import helpers_train_loop as H
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _chunk():
    return int(L.load().adf_op_optimizer_chunk())


def _optimizer(module, max_norm, lr=1e-2, weight_decay=0.01, ema_decay=0.99, use_num_updates=False):
    ema = ExponentialMovingAverage(module.parameters(), ema_decay, use_num_updates=use_num_updates) if ema_decay else None
    return MultiTensorAdamW(module, lr=lr, weight_decay=weight_decay, max_grad_norm=max_norm, ema=ema), ema


def _snapshot(module, opt, ema):
    return ([p.detach().clone() for p in module.parameters()], [m.clone() for m in opt.exp_avg],
            [v.clone() for v in opt.exp_avg_sq], [s.clone() for s in ema.shadow_params])


# ------------------------------------------------------------------------------------------------ against the float64 oracle
@pytest.mark.parametrize("max_norm", [5.0, 1e6], ids=["clip_active", "clip_inactive"])
def test_multi_tensor_adamw_matches_torch_adamw_clip_ema_in_float64(max_norm):
    mod = H.Synthetic(_chunk(), DEV)
    opt, ema = _optimizer(mod, max_norm)
    ref = H.Float64Mirror(mod, lr=1e-2, weight_decay=0.01, max_norm=max_norm, ema_decay=0.99)
    assert [len(g["params"]) for g in opt.param_groups] == [1, 8] and opt.param_groups[0]["weight_decay"] == 0
    for it in range(5):
        mod.set_grads(100 + it)
        gn_ref = float(ref.step(mod))
        gn = float(opt.step())
        assert (gn_ref > max_norm) == (max_norm == 5.0)   # clipping is active in one case and not in the other
        assert abs(gn - gn_ref) < 1e-5 * gn_ref, (it, gn, gn_ref)
    for (n, p), q in zip(mod.named_parameters(), ref.params):
        assert rel_err(p.detach().cpu().double(), q.detach()) < 2e-6, n
    for (n, _), s, s_ref in zip(mod.named_parameters(), ema.shadow_params, ref.ema.shadow_params):
        assert rel_err(s.cpu().double(), s_ref) < 2e-6, n
    # the tensor without a gradient did not move (no weight decay either), and has no state
    assert torch.equal(mod.p257.detach().cpu().double(), ref.params[4].detach())
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3, 5, 6, 7, 8]   # p257 is index 4 of (p63 | p1, p64, p65, p257, ...)
    assert opt.counters() == {"applied": 5, "skipped": 0}


def test_ema_decay_warms_up_with_the_device_counter():
    mod = H.Synthetic(_chunk(), DEV)
    opt, ema = _optimizer(mod, 5.0, ema_decay=0.999, use_num_updates=True)
    ref = H.Float64Mirror(mod, lr=1e-2, weight_decay=0.01, max_norm=5.0, ema_decay=0.999)
    ref.ema.num_updates = 0
    for it in range(3):
        mod.set_grads(300 + it)
        ref.step(mod)
        opt.step()
    for s, s_ref in zip(ema.shadow_params, ref.ema.shadow_params):
        assert rel_err(s.cpu().double(), s_ref) < 2e-6
    assert ema.num_updates == 0   # the host count is refreshed at state_dict() only
    opt.state_dict()
    assert ema.num_updates == 3 == ref.ema.num_updates


# ------------------------------------------------------------------------------------------------ the norm
def test_gradient_norm_is_reproducible_and_independent_of_the_launch():
    Lc = _chunk()
    mod = H.Synthetic(Lc, DEV)
    mod.set_grads(7)
    opt, _ = _optimizer(mod, None, lr=0.0, weight_decay=0.0)
    a = opt.step().clone()
    b = opt.step().clone()
    assert torch.equal(a, b)
    # the same tensors in a launch with more chunks: tensors without a gradient appended
    more = H.Synthetic(Lc, DEV, extra=3)
    more.set_grads(7)
    for n, p in mod.named_parameters():
        q = dict(more.named_parameters())[n]
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), n
    opt2, _ = _optimizer(more, None, lr=0.0, weight_decay=0.0)
    assert opt2.nchunks == opt.nchunks + 3
    assert torch.equal(opt2.step(), a)
    want = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in mod.parameters() if p.grad is not None))
    assert abs(float(a) - float(want)) <= 1e-6 * float(want), (float(a), float(want))
    # 16-byte loads or scalar loads: the same elements in the same order, so the same bits wherever the gradients sit
    for misalign in ((), ("p65", "pLm1", "pL", "pLp1", "p2Lp3")):
        moved = H.Synthetic(Lc, DEV)
        moved.set_grads(7, misalign=misalign)
        assert all((p.grad.data_ptr() % 16 != 0) == (n in misalign) for n, p in moved.named_parameters() if p.grad is not None)
        opt3, _ = _optimizer(moved, None, lr=0.0, weight_decay=0.0)
        assert torch.equal(opt3.step(), a), misalign


def test_gradient_norm_over_more_chunks_than_one_tile_of_the_second_stage():
    mod = H.ManySmall(600, DEV)
    opt = MultiTensorAdamW(mod, lr=0.0, weight_decay=0.0, max_grad_norm=None, ema=None)
    assert opt.nchunks == 600
    a = opt.step().clone()
    assert torch.equal(opt.step(), a)
    want = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in mod.parameters()))
    assert abs(float(a) - float(want)) <= 1e-6 * float(want), (float(a), float(want))


# ------------------------------------------------------------------------------------------------ non-finite gradients
def test_a_nan_gradient_changes_nothing_but_the_skip_count():
    mod = H.Synthetic(_chunk(), DEV)
    opt, ema = _optimizer(mod, 5.0, use_num_updates=True)
    mod.set_grads(1)
    opt.step()
    before = _snapshot(module=mod, opt=opt, ema=ema)
    state = copy.deepcopy(opt.state_dict())
    ema_state = copy.deepcopy(ema.state_dict())
    mod.set_grads(2)
    mod.pL.grad[12345] = float("nan")
    norm = opt.step()
    assert not bool(torch.isfinite(norm))
    for was, now in zip(before, _snapshot(module=mod, opt=opt, ema=ema)):
        for x, y in zip(was, now):
            assert torch.equal(x, y)
    assert opt.counters() == {"applied": 1, "skipped": 1}
    # the next clean step is step 2 of an optimizer that never saw the NaN
    fresh_mod = H.Synthetic(_chunk(), DEV)
    with torch.no_grad():
        for p, x in zip(fresh_mod.parameters(), before[0]):
            p.copy_(x)
    fresh, fresh_ema = _optimizer(fresh_mod, 5.0, use_num_updates=True)
    fresh_ema.load_state_dict(ema_state)
    fresh.load_state_dict(state)
    for m_, o_ in ((mod, opt), (fresh_mod, fresh)):
        m_.set_grads(3)
        o_.step()
    for was, now in zip(_snapshot(fresh_mod, fresh, fresh_ema), _snapshot(mod, opt, ema)):
        for x, y in zip(was, now):
            assert torch.equal(x, y)
    assert opt.counters() == {"applied": 2, "skipped": 1} and fresh.counters() == {"applied": 2, "skipped": 0}


# ------------------------------------------------------------------------------------------------ torch's state layout
def test_state_dict_round_trip_through_torch_adamw():
    Lc = _chunk()
    mod = H.Synthetic(Lc, DEV)
    opt, _ = _optimizer(mod, None, ema_decay=None)
    twin = H.Synthetic(Lc, DEV)
    topt = torch.optim.AdamW(reference_param_groups(twin, 0.01), lr=1e-2)
    for it in range(2):
        twin.set_grads(40 + it)
        topt.step()
    # torch -> here: step 3 of both agree
    with torch.no_grad():
        for p, q in zip(mod.parameters(), twin.parameters()):
            p.copy_(q)
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    assert opt.counters() == {"applied": 2, "skipped": 0}
    for m_, o_ in ((twin, topt), (mod, opt)):
        m_.set_grads(42)
        o_.step()
    for (n, p), q in zip(mod.named_parameters(), twin.parameters()):
        assert rel_err(p.detach(), q.detach()) < 2e-6, n
    # here -> torch: what we write is what torch.optim.AdamW loads, and its next step agrees with ours
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 3.0 and 4 not in sd["state"]
    assert set(sd["param_groups"][0]) == set(topt.state_dict()["param_groups"][0])
    third = H.Synthetic(Lc, DEV)
    with torch.no_grad():
        for p, q in zip(third.parameters(), mod.parameters()):
            p.copy_(q)
    topt3 = torch.optim.AdamW(reference_param_groups(third, 0.01), lr=1e-2)
    topt3.load_state_dict(copy.deepcopy(sd))
    for m_, o_ in ((third, topt3), (mod, opt)):
        m_.set_grads(43)
        o_.step()
    for (n, p), q in zip(mod.named_parameters(), third.parameters()):
        assert rel_err(p.detach(), q.detach()) < 2e-6, n
    # one counter: unequal steps are refused
    bad = copy.deepcopy(sd)
    bad["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="one counter"):
        opt.load_state_dict(bad)


def test_torch_schedulers_accept_the_optimizer():
    mod = H.Synthetic(_chunk(), DEV)
    opt, _ = _optimizer(mod, None, lr=1e-2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 ** s)
    before = mod.p64.detach().clone()
    mod.set_grads(9)
    opt.step()
    sched.step()
    assert opt.param_groups[0]["lr"] == 0.5e-2 and not torch.equal(before, mod.p64.detach())
    torch.optim.lr_scheduler.ReduceLROnPlateau(opt)


# ------------------------------------------------------------------------------------------------ ordered embedding backward
@pytest.mark.parametrize("N", [1, 64, 65, 777])
def test_ordered_embedding_backward(N):
    lib = L.load()
    H_, rows = 96, 12
    g = torch.Generator().manual_seed(N)
    Z = torch.full((N,), 3, dtype=torch.int32)
    if N > 2:
        Z[torch.rand(N, generator=g) < 0.5] = 7
        Z[N // 2] = 11          # present once; 5 and every other row are absent
    assert N < 3 or (int((Z == 11).sum()) == 1 and int((Z == 7).sum()) > 0 and int((Z == 3).sum()) > 0)
    dx = torch.randn(N, H_, generator=g)
    base = torch.randn(rows, H_, generator=g)
    want = base.double().index_add(0, Z.long() - 1, dx.double())
    Zd, dxd = Z.to(DEV), dx.to(DEV)
    scratch = torch.empty(int(lib.adf_op_embed_bwd_ordered_scratch(N, H_, rows)), device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for _ in range(2):
        demb = base.to(DEV)
        L.check(lib.adf_op_embed_bwd_ordered(dxd.data_ptr(), Zd.data_ptr(), demb.data_ptr(), N, H_, rows, scratch.data_ptr(),
                                             stream))
        outs.append(demb.cpu())
    assert torch.equal(outs[0], outs[1])
    present = torch.zeros(rows, dtype=torch.bool)
    present[Z.long() - 1] = True
    assert torch.equal(outs[0][~present], base[~present])          # untouched, not rewritten with + 0
    err = (outs[0].double() - want).abs().amax(dim=1)
    assert bool((err[present] <= 1e-6 * want.abs().amax(dim=1)[present]).all()), err


def test_ordered_embedding_backward_over_more_segments_than_one_tile():
    """257 segments: stage 2 stages its slot table in tiles of 256 segments.  The bound is the worst case of float32
    summation: an element passes through at most 64 (its segment) + 257 (the segments) + 1 (the row) additions, each
    rounding by 2^-24 relative to a partial sum that the sum of magnitudes bounds."""
    lib = L.load()
    N, H_, rows = 64 * 256 + 1, 96, 12
    g = torch.Generator().manual_seed(5)
    Z = torch.where(torch.rand(N, generator=g) < 0.5, 3, 7).to(torch.int32)
    Z[N - 1] = 11   # alone in the last, one-atom segment
    dx = torch.randn(N, H_, generator=g)
    base = torch.randn(rows, H_, generator=g)
    idx = Z.long() - 1
    want = base.double().index_add(0, idx, dx.double())
    magnitude = base.double().abs().index_add(0, idx, dx.double().abs())
    Zd, dxd = Z.to(DEV), dx.to(DEV)
    scratch = torch.empty(int(lib.adf_op_embed_bwd_ordered_scratch(N, H_, rows)), device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for _ in range(2):
        demb = base.to(DEV)
        L.check(lib.adf_op_embed_bwd_ordered(dxd.data_ptr(), Zd.data_ptr(), demb.data_ptr(), N, H_, rows, scratch.data_ptr(),
                                             stream))
        outs.append(demb.cpu())
    assert torch.equal(outs[0], outs[1])
    present = torch.zeros(rows, dtype=torch.bool)
    present[idx] = True
    assert int(present.sum()) == 3 and torch.equal(outs[0][~present], base[~present])
    bound = (64 + 257 + 1) * 2.0 ** -24 * magnitude
    assert bool(((outs[0].double() - want).abs() <= bound)[present].all())
    assert torch.equal(outs[0][10], base[10] + dx[N - 1])   # one atom: one addition
