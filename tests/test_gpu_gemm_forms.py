"""The two forms of the f16x3 node products (csrc/gemm16.hip): the default, weights streamed as fragments by four waves laid
out 1(M) x 4(N) - 96 x 256 tiles for the plain, vec_proj and vector-norm products (32 atoms x 3 components for the latter
two), 64 x 384 tiles for the fused x_proj.2 / xvec_proj.2 products - against the LDS-staged 2(M) x 2(N) reference form that
ADF_GEMM_STREAM=0 runs everywhere.  Both forms keep the products of every output element, their order along K, the lifts and
the epilogues' arithmetic, so nothing here has a tolerance: every comparison is torch.equal between two engines of one model
in one process, each created under its own environment (the switch is read when the handle is created,
tests/test_gpu_tune.py).

Model: H = 256, 2 layers, R = 128 - every layer product is a multiple of 256 (resp. 384) wide with an even number of K tiles
and streams by default; the heads' products are 128 wide there and run LDS-staged either way, so one case runs H = 512,
1 layer, where they are 256 wide.  Atom counts: 31 (one ragged tile), 32 (exactly one), 33 (a full tile + a one-atom tile), 97
(fused products: one 64-row tile + a ragged one; plain: a full 96-row tile + one row), 210 (the shape of test_gpu_tune.py),
290 (ten 32-atom tiles: the XCD tile map's second group of eight runs with six padding tiles that return at m0 >= M)."""
import contextlib
import ctypes as C
import os

import pytest
import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.synthetic import make_system

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP256 = dict(hidden_channels=256, num_layers=2, num_rbf=128, cutoff=5.0, max_neighbors=50)
HP512 = dict(hidden_channels=512, num_layers=1, num_rbf=128, cutoff=5.0, max_neighbors=50)
SCALES = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
ATOMS = (31, 32, 33, 97, 210, 290)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():   # (None: the variable is absent)
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _batch(n):
    """n atoms: one system up to 40 atoms, else two of unequal size (4 adsorbate atoms each)."""
    gen = torch.Generator().manual_seed(100 + n)
    sizes = (n,) if n <= 40 else (n // 3, n - n // 3)
    b = Batch.from_data_list([make_system(gen, s - 4, 4, sid=str(i)) for i, s in enumerate(sizes)])
    assert b.pos.shape[0] == n
    return b


def _pair(hp, seed, **extra_env):
    """Two engines of one model: ADF_GEMM_STREAM = 0 (LDS-staged everywhere) and the default."""
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in PaiNN(None, 50, 1, scale_file=SCALES, so3_denoising=True, **hp).state_dict().items()}
    models = []
    for stream in (0, 1):
        with _env(ADF_GEMM_STREAM=None if stream else "0", **extra_env):
            m = PaiNN(None, 50, 1, scale_file=SCALES, so3_denoising=True, **hp)
            m.load_state_dict(sd)
            m = m.to(DEV).eval()
            assert m.engine().get_tune()["gemm_stream"] == stream
        models.append(m)
    # every other switch is what it is without the variable
    ta, tb = (m.engine().get_tune() for m in models)
    assert {k: v for k, v in ta.items() if k != "gemm_stream"} == {k: v for k, v in tb.items() if k != "gemm_stream"}
    return models


@pytest.fixture(scope="module")
def pair256():
    return _pair(HP256, 21)


def _maxima(eng, which, rows_expected, width):
    rows = C.c_int32(0)
    out = torch.full((rows_expected * width,), -1.0, device=DEV)
    with torch.cuda.device(eng.device):
        st = eng.lib.adf_painn_debug_row_maxima(eng.handle, which, out.data_ptr(), out.numel(), C.byref(rows), eng._stream())
    assert st == 0, eng.lib.adf_last_error()
    assert rows.value == rows_expected
    return out


def _rows_of(m, hp, b, check_maxima):
    """f1, f2 of a forward, then the outputs of the per-layer entries, layer by layer."""
    N, H = b.pos.shape[0], hp["hidden_channels"]
    f1, f2 = m(b.clone())
    rows = [f1.clone(), f2.clone()]
    eng = m.engine()
    if check_maxima:   # capture on: vec_proj leaves its |v2| slots on the per-layer entry too
        assert eng.lib.adf_painn_debug_row_maxima(eng.handle, 4, None, 1, None, eng._stream()) == 0
    eng.build_graph(b)
    x = m.atom_emb.embeddings.weight.detach()[b.atomic_numbers.long() - 1].contiguous()
    vec = torch.zeros(N, 3, H, device=DEV)
    for li in range(hp["num_layers"]):
        x, vec = eng.message_layer(li, x, vec)
        rows += [x.clone(), vec.clone()]
        x, vec = eng.update_layer(li, x, vec)
        rows += [x.clone(), vec.clone()]
        if check_maxima:
            # EPI 3's slot stores depend on which lanes hold a row: the combined maxima against the |v2| rows themselves
            cat = _maxima(eng, 3, N, H).reshape(N, H)
            assert bool((cat > 0).all())
            assert torch.equal(_maxima(eng, 2, N, 1), cat.amax(dim=1)), li
    return rows


def _compare(models, hp, n):
    b = _batch(n).to(DEV)
    old = _rows_of(models[0], hp, b, False)
    new = _rows_of(models[1], hp, b, True)
    assert all(bool(torch.isfinite(t).all()) for t in old) and float(old[0].abs().max()) > 0
    assert float(old[-1].abs().max()) > 0   # the last layer's vec
    for k, (a, r) in enumerate(zip(old, new)):
        assert a.shape == r.shape and torch.equal(a, r), (n, k)


@pytest.mark.parametrize("n", ATOMS)
def test_forward_and_layers_are_bit_identical(pair256, n):
    _compare(pair256, HP256, n)


def test_heads_256_wide_products_are_bit_identical():
    """H = 512: the heads' ScaledSiLU, plain, gated and vector-norm products are 256 wide and take the 96 x 256 tile.  97 atoms:
    three full 32-atom tiles + one atom; a full 96-row tile + one row; 291 component rows = three 96-row tiles + three rows."""
    _compare(_pair(HP512, 22), HP512, 97)


def test_sampler_with_listed_rows_is_bit_identical():
    """Three reverse steps on four small systems with incremental layers on: the listed-rows form of a layer launches for the
    host's bound of rows and every product reads its row count from device memory (fewer rows than the bound); same sites."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    params = dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False, incremental_layers=True)
    gen = torch.Generator().manual_seed(78)
    batch = Batch.from_data_list([make_system(gen, n - 4, 4, sid=str(i)) for i, n in enumerate((37, 70, 200, 120))])
    sites = []
    # (ADF_INC_SYNC: the choice between the listed and the all-rows form then rests on a forward's own counts, not on timing)
    for m in _pair(HP256, 23, ADF_INC_SYNC="1"):
        torch.manual_seed(5)
        den = Denoiser(batch.clone(), DiffTorchCalc(DenoisingTrainer(m, device=DEV)), dict(params), device=DEV)
        out = den.run()
        assert den.steps_applied == 3
        c = m.engine().counters()
        print("stream %d: rows %d of %d in %d launches" % (m.engine().get_tune()["gemm_stream"], c.inc_rows, c.inc_rows_full,
                                                            c.inc_msg_launches))
        assert 0 < c.inc_rows < c.inc_rows_full, "no layer took the listed-rows form"
        sites.append(out.pos.clone())
    assert bool(torch.isfinite(sites[0]).all())
    assert torch.equal(sites[0], sites[1])
