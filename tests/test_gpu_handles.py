"""Life-cycle of the two handles (adf_painn, adf_eqv2): workspaces that grow after they have been used, with and without
live incremental state; the subset buffers; state that is set once being set again; the HIP-event profiler; and device
memory coming back when a handle is destroyed.  Both models' forwards are run-to-run bit-identical and independent of the
batch a system sits in (test_forward_is_run_to_run_deterministic, test_eqv2_forward_is_run_to_run_and_batch_independent), so
every comparison here is ``torch.equal``."""
import ctypes as C
import functools
import gc

import pytest
import torch

from adsorbdiff_amd import lib as _lib
from adsorbdiff_amd import so3_math
from adsorbdiff_amd.engine import PaiNNEngine
from adsorbdiff_amd.eqv2_engine import EqV2Engine
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.synthetic import make_batch
from tests.helpers_grad_forces import make_config_batch, make_config_model
from tests.test_gpu_eqv2 import make_model, safe_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("painn", "eqv2")
SENTINEL = 7.0
MB = 1 << 20


def new_model(kind):
    if kind == "painn":   # the model of test_incremental_layers_survive_foreign_builds_and_weight_updates
        torch.manual_seed(9)
        return PaiNN(None, 50, 1, hidden_channels=128, num_layers=3, num_rbf=32, cutoff=3.6, max_neighbors=12,
                     so3_denoising=True, scale_file={f"upd_out_scalar_scale_{i}": 1.0 for i in range(3)}).to(DEV).eval()
    return make_model(6, 2, C=32, hidden=64, heads=2, alpha=16, value=16, ffn=32, ec=32, layers=2, cutoff=12.0).to(DEV)


def new_engine(model):
    """A fresh handle on the module's weights (``model.engine()`` would hand out the module's cached one)."""
    return (EqV2Engine if hasattr(model, "sphere_channels") else PaiNNEngine)(model, torch.device(DEV))


@functools.lru_cache(maxsize=None)
def batch(kind, name):
    if kind == "painn":
        b = make_batch(2, n_slab=40, n_ads=3, seed=1) if name == "S" else make_batch(5, n_slab=100, n_ads=4, seed=2)
    else:
        b = safe_batch(1, 20, seed=3) if name == "S" else safe_batch(3, 36, seed=17)
    return b.to(DEV)


def forward(eng, b, pos=None, idx=None, prep=None):
    """(f1, f2) of one forward; rows the forward does not write keep SENTINEL.  check_flags waits for the stream and
    raises what the kernels flagged."""
    prep = prep if prep is not None else eng.prepare(b)
    f1 = torch.full((prep.num_atoms, 3), SENTINEL, device=DEV)
    f2 = torch.full((prep.num_atoms, 3), SENTINEL, device=DEV)
    eng.forward_prepared(prep, b.pos if pos is None else pos, f1, f2, idx)
    eng.check_flags()
    return f1, f2


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    """The batch alone on a fresh engine: computed once, shared, never written."""
    eng = new_engine(new_model(kind))
    out = forward(eng, batch(kind, name))
    eng.close()
    return out


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("kind", KINDS)
def test_workspaces_regrow_under_use(kind):
    """S, L, S on one engine: L grows capN, capB and capE after the buffers have been used; every output equals the one a
    fresh engine gives on that batch alone."""
    eng = new_engine(new_model(kind))
    for k, name in enumerate("SLS"):
        assert same(forward(eng, batch(kind, name)), reference(kind, name)), (k, name)
    eng.close()


def _incremental_sequence(kind, incremental):
    S, L = batch(kind, "S"), batch(kind, "L")
    eng = new_engine(new_model(kind))
    eng.set_incremental(incremental)
    prep = eng.prepare(S)
    ads = S.tags == 2
    g = torch.Generator().manual_seed(21)
    pos = [S.pos.clone()]
    for _ in range(4):   # the adsorbate moves by 0.1 A per coordinate at the most
        p = pos[-1].clone()
        p[ads] = p[ads] + (torch.rand(int(ads.sum()), 3, generator=g).to(DEV) - 0.5) * 0.2
        pos.append(p)
    outs = []
    eng.set_moving_atoms(prep, ads)
    outs += [forward(eng, S, pos[0], prep=prep), forward(eng, S, pos[1], prep=prep)]   # the kept state is live
    eng.set_moving_atoms(None, None)
    outs.append(forward(eng, L))                                                       # the workspaces grow under it
    eng.set_moving_atoms(prep, ads)
    outs += [forward(eng, S, pos[2], prep=prep), forward(eng, S, pos[3], prep=prep)]
    # PaiNN's host sees a forward's list lengths one forward late, so a promise's second forward still takes the all-rows
    # form (measured: inc_rows == inc_rows_full == 1032 after the two forwards above, before and after this file's
    # change); the third is the first that can run on the lists
    outs.append(forward(eng, S, pos[4], prep=prep))
    counters = eng.counters()
    eng.set_moving_atoms(None, None)
    eng.close()
    return outs, counters


@pytest.mark.parametrize("kind", KINDS)
def test_regrow_with_live_incremental_state(kind):
    """Two forwards of S under a static-atom promise, a forward of L without one, S promised again and three more
    forwards: every output equals the same sequence with incremental layers / blocks switched off, and (PaiNN) the row
    counters show that the incremental path ran after the regrow."""
    ref, _ = _incremental_sequence(kind, False)
    got, c = _incremental_sequence(kind, True)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert same(a, b), k
    print(kind, "inc_rows", c.inc_rows, "inc_rows_full", c.inc_rows_full)
    assert c.inc_rows_full > 0
    if kind == "painn":
        assert c.inc_rows < c.inc_rows_full, (c.inc_rows, c.inc_rows_full)


@pytest.mark.parametrize("kind", KINDS)
def test_subset_buffers_grow(kind):
    """forward_prepared(out_idx=...) with 3, then 40 rows of L: the listed rows equal the full forward's, the others keep
    the sentinel.  The buffers are sized n + n / 4 + 64 rows, so 3 rows leave room for 40; a third call with 100 rows is
    what makes them grow."""
    L = batch(kind, "L")
    N = L.pos.shape[0]
    full = reference(kind, "L")
    eng = new_engine(new_model(kind))
    prep = eng.prepare(L)
    last = int(prep.atom_offset[-2])   # first atom of the last system
    for n in (3, 40, 100):
        idx = torch.unique(torch.linspace(0, N - 1, n).round().long())
        assert idx.numel() == n and int(idx[-1]) >= last
        sub = forward(eng, L, idx=idx.to(DEV, torch.int32).contiguous(), prep=prep)
        rest = torch.ones(N, dtype=torch.bool, device=DEV)
        rest[idx.to(DEV)] = False
        for s, f in zip(sub, full):
            assert torch.equal(s[idx.to(DEV)], f[idx.to(DEV)]), n
            assert bool((s[rest] == SENTINEL).all()), n
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_set_once_state_survives_being_set_twice(kind):
    """Binding the weights a second time, and (EquiformerV2) handing over the constant tables a second time the way the
    engine's constructor does, leaves the forward unchanged."""
    S = batch(kind, "S")
    m = new_model(kind)
    eng = new_engine(m)
    assert same(forward(eng, S), reference(kind, "S"))
    eng.bind_weights()
    if kind == "eqv2":
        t = so3_math.device_tables(eng.lmax, eng.mmax, int(m.grid_resolution))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.adf_eqv2_set_constants(eng.handle, ptr(t["jd"]), ptr(t["to_red"]), ptr(t["from_red"]),
                                                      ptr(t["to_full"]), ptr(t["from_full"])))
    else:
        eng.bind_weights()
    assert same(forward(eng, S), reference(kind, "S"))
    eng.close()


def _timed(read):
    return {k: v for k, v in read.items() if isinstance(v, tuple)}   # (PaiNN's read also carries message_ksteps)


@pytest.mark.parametrize("kind", KINDS)
def test_profiler(kind):
    """Categories of one forward, a read empties, 60 forwards without a read (the event pool grows several times on the
    way) count exactly 60-fold, and nothing is recorded when switched off."""
    L = batch(kind, "L")
    eng = new_engine(new_model(kind))
    forward(eng, L)
    eng.profile_enable(True)
    forward(eng, L)
    one = _timed(eng.profile_read())
    print(kind, one)
    must = ("graph", "message", "node_dense", "heads") if kind == "painn" else ("graph", "so2_conv", "node")
    for k in must:
        assert one[k][1] > 0, k
    for k, (ms, n) in one.items():
        assert (ms > 0) == (n > 0), (k, ms, n)
    assert all(v == (0.0, 0) for v in _timed(eng.profile_read()).values())
    for _ in range(60):
        forward(eng, L)
    many = _timed(eng.profile_read())
    assert sum(n for _, n in one.values()) * 60 * 2 > 2 * 512   # events used: more than two chunks of the pool
    for k in one:
        assert many[k][1] == 60 * one[k][1], (k, many[k], one[k])
        assert (many[k][0] > 0) == (many[k][1] > 0), (k, many[k])
    eng.profile_enable(False)
    forward(eng, L)
    assert all(v == (0.0, 0) for v in _timed(eng.profile_read()).values())
    eng.close()


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _cycle(kind, S, L):
    """New module, engine, forward of S and of L, close (PaiNN: also an energy-gradient evaluation on the S2EF mirror of
    tests/helpers_grad_forces.py, whose state the handle owns through a pointer of its own).  Returns the footprint of
    the live engine: free memory before its creation minus free memory after the forward of L."""
    before = _free()
    m = new_model(kind)
    eng = new_engine(m)
    forward(eng, S)
    forward(eng, L)
    footprint = before - _free()
    eng.close()
    if kind == "painn":
        mirror = make_config_model("one_layer").to(DEV)
        e2 = new_engine(mirror)
        e2.forward_energy_gradient(make_config_batch("one_layer").to(DEV))
        e2.close()
        del mirror, e2
    del m, eng
    gc.collect()
    return footprint


@pytest.mark.parametrize("kind", KINDS)
def test_create_and_destroy_return_the_memory(kind):
    """Six create / use / destroy cycles lose less than half the footprint F of one live engine (a handle that leaked
    everything would lose about 6 F; the margin absorbs allocator granularity and lazily loaded code objects).  L is
    enlarged for this test until F >= 64 MB."""
    S = batch(kind, "S")
    F = 0
    for n_slab in ((1200, 2400, 4800) if kind == "painn" else (36, 72, 144, 288)):
        L = (make_batch(5, n_slab=n_slab, n_ads=4, seed=2) if kind == "painn" else safe_batch(3, n_slab, seed=17)).to(DEV)
        _cycle(kind, S, L)       # warm-up: code objects, the caching allocator's blocks
        F = _cycle(kind, S, L)
        if F >= 64 * MB:
            break
    assert F >= 64 * MB, F
    free0 = _free()
    series = []
    for _ in range(6):
        _cycle(kind, S, L)
        series.append((free0 - _free()) / MB)
    msg = f"{kind}: footprint {F / MB:.1f} MB; MB lost after each cycle: {[round(x, 1) for x in series]}"
    print(msg)
    assert len(series) == 6 and series[-1] * MB < F / 2, msg
