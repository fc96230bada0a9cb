"""The gather records of x_proj.2's fused epilogue (EPI 1 of gemm16.hip) are stored a whole 128-B line per row and store
instruction: the eight lanes of a row exchange their (P0, P1, P2, xa) float4s through LDS first.  What the exchange could get
wrong is WHERE a float4 lands (another channel, another row of the same wave), which the forms of the kernel cannot show
against each other - they share the epilogue.  So the message layers, which consume nothing but the records, are compared with
the exact-f32 path (ADF_GEMM=f32: gemm.hip writes its records with its own epilogue), row by row.

Bounds.  A f16x3 product carries about 7e-7 relative error (gemm16.hip header) and a message row sums some 50 neighbours'
records: the norm-relative difference of a layer's output is bounded by 2e-5, the bound tests/test_gpu_parity.py holds a whole
forward to, and every single row's difference by 1e-4 of the largest row norm, the project's parity budget.  A misplaced float4
puts a row off by the order of its own magnitude.

Model: H = 256, 2 layers, R = 128 (layer 0 takes the vec_is_zero branch, layer 1 the full one).  Atom counts as for the tile
tests: 31 (one ragged 32-row block), 33 and 65 (a block / a 64-row tile + one row), 290 (padding tiles).  The two forms
(ADF_GEMM_STREAM = 0 LDS-staged weights, and the default) must still give the same bits."""
import contextlib
import os

import pytest
import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.synthetic import make_system
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP = dict(hidden_channels=256, num_layers=2, num_rbf=128, cutoff=5.0, max_neighbors=50)
SCALES = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}
ATOMS = (31, 33, 65, 290)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _batch(n):
    gen = torch.Generator().manual_seed(500 + n)
    sizes = (n,) if n <= 40 else (n // 3, n - n // 3)
    b = Batch.from_data_list([make_system(gen, s - 4, 4, sid=str(i)) for i, s in enumerate(sizes)])
    assert b.pos.shape[0] == n
    return b


@pytest.fixture(scope="module")
def models():
    """One model as three engines: exact f32, and the f16x3 path with x_proj.2 in each of its two forms."""
    torch.manual_seed(41)
    sd = {k: v.clone() for k, v in PaiNN(None, 50, 1, scale_file=SCALES, so3_denoising=True, **HP).state_dict().items()}
    out = {}
    for name, env in (("f32", dict(ADF_GEMM="f32")), ("lds", dict(ADF_GEMM_STREAM="0")), ("default", dict())):
        with _env(**env):
            m = PaiNN(None, 50, 1, scale_file=SCALES, so3_denoising=True, **HP)
            m.load_state_dict(sd)
            m = m.to(DEV).eval()
            eng = m.engine()
            assert eng.exact_f32 == (name == "f32")
            if name != "f32":
                assert eng.get_tune()["gemm_stream"] == (name == "default")
        out[name] = m
    return out


def _message_rows(m, b, x0, vec0):
    """Outputs of both message layers on the same inputs (layer 1 with a non-zero vec: the full record epilogue)."""
    eng = m.engine()
    eng.build_graph(b)
    rows = []
    for li, vec in ((0, torch.zeros_like(vec0)), (1, vec0)):
        x, v = eng.message_layer(li, x0.clone(), vec.clone())
        rows += [x.clone(), v.clone()]
    return rows


@pytest.mark.parametrize("n", ATOMS)
def test_message_layers_match_exact_f32_row_by_row(models, n):
    b = _batch(n).to(DEV)
    m = models["f32"]
    x0 = m.atom_emb.embeddings.weight.detach()[b.atomic_numbers.long() - 1].contiguous()
    vec0 = torch.randn(n, 3, HP["hidden_channels"], generator=torch.Generator().manual_seed(n)).to(DEV)
    ref = _message_rows(m, b, x0, vec0)
    got = {k: _message_rows(models[k], b, x0, vec0) for k in ("lds", "default")}
    for k, (r, a) in enumerate(zip(ref, got["default"])):
        assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0, (n, k)
        e = rel_err(a, r)
        rown = (a.double() - r.double()).reshape(n, -1).norm(dim=1)
        worst = float(rown.max() / r.double().reshape(n, -1).norm(dim=1).max())
        print("n %d tensor %d: rel err %.2e, worst row %.2e" % (n, k, e, worst))
        assert e < 2e-5 and worst < 1e-4, (n, k)
        assert torch.equal(a, got["lds"][k]), (n, k)
