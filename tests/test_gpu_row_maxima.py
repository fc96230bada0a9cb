"""Row maxima from the producers (ADF_ROW_MAXIMA): the f16x3 products of PaiNNUpdate lift every A row by a power of two
taken from max|a| of the row.  With the switch on (default) the message kernel and vec_proj's epilogue leave partial maxima
of the rows they write and a small kernel combines them; with ADF_ROW_MAXIMA=0 a pass of its own measures the rows.  A maximum
is exact and order-free, so nothing here has a tolerance: the combined maxima equal ``abs().amax()`` of the rows and every
result is bit-identical between the two switch values.

Shape: H = 512, 2 layers, R = 128 (the benchmark's kernels at their default tiles), one batch of three systems with 37, 70
and 200 atoms: N = 307 is no multiple of 32, 64, 128 or 192.  One adsorbate atom is lifted out of everybody's cutoff, and the
5 A cutoff leaves targets with 0, 1-16, 17-32 and more than 32 in-edges: every branch of the message kernel's block tail."""
import ctypes as C

import pytest
import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.synthetic import make_system

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP = dict(hidden_channels=512, num_layers=2, num_rbf=128, cutoff=5.0, max_neighbors=50)
NATOMS = (37, 70, 200)


def _batch():
    gen = torch.Generator().manual_seed(77)
    b = Batch.from_data_list([make_system(gen, n - 4, 4, sid=str(i)) for i, n in enumerate(NATOMS)])
    b.pos[-1, 2] = 28.0   # the last adsorbate atom of the 200-atom system: 9 A above the rest, 14 A below the next image
    return b


@pytest.fixture(scope="module")
def weights():
    torch.manual_seed(11)
    m = PaiNN(None, 50, 1, scale_file={"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}, so3_denoising=True,
              **HP)
    return {k: v.clone() for k, v in m.state_dict().items()}


def _model(weights, monkeypatch, switch, inc_sync=False):
    """A model with a handle of its own; the switch is read when the handle is created (first engine() call)."""
    monkeypatch.setenv("ADF_ROW_MAXIMA", switch)
    if inc_sync:   # the choice between the listed and the all-rows form then rests on this forward's own counts, not on timing
        monkeypatch.setenv("ADF_INC_SYNC", "1")
    m = PaiNN(None, 50, 1, scale_file={"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}, so3_denoising=True,
              **HP)
    m.load_state_dict(weights)
    m = m.to(DEV).eval()
    m.engine()
    return m


def _maxima(eng, which, rows_expected, width):
    rows = C.c_int32(0)
    out = torch.full((rows_expected * width,), -1.0, device=DEV)
    with torch.cuda.device(eng.device):
        st = eng.lib.adf_painn_debug_row_maxima(eng.handle, which, out.data_ptr(), out.numel(), C.byref(rows), eng._stream())
    assert st == 0, eng.lib.adf_last_error()
    assert rows.value == rows_expected
    return out


def _capture(eng, on=True):
    """While capture is on, vec_proj leaves its slots on the per-layer entry too and update_layer keeps what it combined."""
    assert eng.lib.adf_painn_debug_row_maxima(eng.handle, 4, None, 1 if on else 0, None, eng._stream()) == 0


def _layer_inputs(m, b):
    x = m.atom_emb.embeddings.weight.detach()[b.atomic_numbers.long() - 1].contiguous()
    return x, torch.zeros(x.shape[0], 3, HP["hidden_channels"], device=DEV)


def test_batch_has_every_in_degree_class(weights, monkeypatch):
    b = _batch().to(DEV)
    N = sum(NATOMS)
    assert b.pos.shape[0] == N and all(N % t for t in (32, 64, 128, 192))
    eng = _model(weights, monkeypatch, "1").engine()
    eng.build_graph(b)
    dst = eng.export_graph()[4]
    deg = torch.bincount(dst.long(), minlength=N)
    print("in-degrees: none %d, 1-16 %d, 17-32 %d, more %d, max %d" % (
        int((deg == 0).sum()), int(((deg > 0) & (deg <= 16)).sum()), int(((deg > 16) & (deg <= 32)).sum()),
        int((deg > 32).sum()), int(deg.max())))
    assert int(deg[N - 1]) == 0, "the lifted atom is not isolated"
    assert bool(((deg > 0) & (deg <= 16)).any()) and bool(((deg > 16) & (deg <= 32)).any()) and bool((deg > 32).any())


def test_combined_maxima_are_exact(weights, monkeypatch):
    """The maxima the producers leave, combined over their slots, equal abs().amax() of the rows they wrote: x_out / vec_out of
    the message kernel (layer 0 with an all-zero vec, layer 1 with a full one) and |v2| of vec_proj's epilogue.  (The kernel
    variant that skips a zero vec runs inside adf_painn_forward: the bit-identity tests below.)"""
    b = _batch().to(DEV)
    m = _model(weights, monkeypatch, "1")
    eng = m.engine()
    _capture(eng)
    eng.build_graph(b)
    N, H = b.pos.shape[0], HP["hidden_channels"]
    x, vec = _layer_inputs(m, b)
    for li in range(HP["num_layers"]):
        x, vec = eng.message_layer(li, x, vec)
        mx, mv = _maxima(eng, 0, N, 1), _maxima(eng, 1, N, 3)
        assert torch.equal(mx, x.abs().amax(dim=1)), li
        assert torch.equal(mv, vec.abs().amax(dim=2).reshape(-1)), li
        if li == 0:
            assert float(mv.reshape(N, 3)[N - 1].max()) == 0.0   # the isolated target wrote its slots too (vec stays 0)
        x, vec = eng.update_layer(li, x, vec)
        cat = _maxima(eng, 3, N, H).reshape(N, H)
        assert bool((cat > 0).all())   # sqrt(|v2|^2 + 1e-8)
        assert torch.equal(_maxima(eng, 2, N, 1), cat.amax(dim=1)), li


def test_update_layer_hands_its_products_the_exact_maxima(weights, monkeypatch):
    """What update_layer itself combined inside adf_painn_forward (the vec form over 3 N rows; the [x | |v2|] form over the
    adjacent runs of x and |v2| slots) for its last layer, against abs().amax() of that layer's rows, rebuilt through the
    per-layer entries.  (The device-side row count of the listed-rows form has no such check: the sampler test below.)"""
    b = _batch().to(DEV)
    m = _model(weights, monkeypatch, "1")
    eng = m.engine()
    _capture(eng)
    m(b)
    N, H, L = b.pos.shape[0], HP["hidden_channels"], HP["num_layers"]
    got_vec, got_xcat = _maxima(eng, 5, N, 3), _maxima(eng, 6, N, 1)
    eng.build_graph(b)
    x, vec = _layer_inputs(m, b)
    for li in range(L):
        x, vec = eng.message_layer(li, x, vec)
        if li == L - 1:
            want_vec, want_x = vec.abs().amax(dim=2).reshape(-1), x.abs().amax(dim=1)
        x, vec = eng.update_layer(li, x, vec)
    cat = _maxima(eng, 3, N, H).reshape(N, H)
    assert torch.equal(got_vec, want_vec)
    assert torch.equal(got_xcat, torch.maximum(want_x, cat.amax(dim=1)))
    assert bool((want_x != cat.amax(dim=1)).any())


def test_switch_on_and_off_are_bit_identical_forward(weights, monkeypatch):
    """Two handles with the same weights: the per-layer rows and both head outputs, switch on against off."""
    b = _batch().to(DEV)
    outs = []
    for switch in ("1", "0"):
        m = _model(weights, monkeypatch, switch)
        f1, f2 = m(b)
        eng = m.engine()
        eng.build_graph(b)
        x, vec = _layer_inputs(m, b)
        rows = [f1.clone(), f2.clone()]
        for li in range(HP["num_layers"]):
            x, vec = eng.message_layer(li, x, vec)
            rows += [x.clone(), vec.clone()]
            x, vec = eng.update_layer(li, x, vec)
            rows += [x.clone(), vec.clone()]
        outs.append(rows)
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][0].abs().max()) > 0
    for k, (a, r) in enumerate(zip(*outs)):
        assert torch.equal(a, r), k


def test_switch_on_and_off_are_bit_identical_sampler(weights, monkeypatch):
    """Four reverse steps with incremental layers on: the listed-rows form (compact output rows, row counts on the device)
    takes the maxima from the producers too; same sites bit for bit, and at least one layer did take the listed form."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    params = dict(num_steps=4, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False, incremental_layers=True)
    sites = []
    for switch in ("1", "0"):
        m = _model(weights, monkeypatch, switch, inc_sync=True)
        torch.manual_seed(5)
        den = Denoiser(_batch(), DiffTorchCalc(DenoisingTrainer(m, device=DEV)), dict(params), device=DEV)
        out = den.run()
        assert den.steps_applied == 4
        c = m.engine().counters()
        print("switch %s: rows %d of %d in %d launches" % (switch, c.inc_rows, c.inc_rows_full, c.inc_msg_launches))
        assert 0 < c.inc_rows < c.inc_rows_full, "no layer took the listed-rows form"
        sites.append(out.pos.clone())
    assert bool(torch.isfinite(sites[0]).all())
    assert torch.equal(sites[0], sites[1])


def test_update_layer_on_foreign_rows_falls_back(weights, monkeypatch):
    """adf_painn_update_layer on rows that did not come from the message kernel - while the slots still hold the maxima of
    the message launch before - measures them itself: same bits as with the switch off."""
    b = _batch().to(DEV)
    N, H = b.pos.shape[0], HP["hidden_channels"]
    g = torch.Generator().manual_seed(3)
    x0 = (torch.randn(N, H, generator=g) * 3.0).to(DEV)
    v0 = (torch.randn(N, 3, H, generator=g) * 0.02).to(DEV)
    outs = []
    for switch in ("1", "0"):
        m = _model(weights, monkeypatch, switch)
        eng = m.engine()
        eng.build_graph(b)
        eng.message_layer(0, *_layer_inputs(m, b))   # leaves maxima of other rows behind
        x, vec = eng.update_layer(0, x0.clone(), v0.clone())
        outs.append((x, vec))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
