"""The kernel-selection switches (adf_tune, include/adsorbdiff_hip.h) are read when a handle is created and belong to that
handle; the product launcher takes its epilogue operands as a struct."""
import ctypes as C

import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.synthetic import make_batch
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DEFAULTS = dict(gemm_stream=1, head_gate_fused=1, lift_emit=1, graph_sys_csr=1)
# every PaiNN switch at its non-default value: environment variable, field, value
SWITCHED = (("ADF_GEMM_STREAM", "gemm_stream", 0), ("ADF_HEAD_GATE_FUSED", "head_gate_fused", 0),
            ("ADF_LIFT_EMIT", "lift_emit", 0), ("ADF_GRAPH_SYS_CSR", "graph_sys_csr", 0))


def test_selection_switches_belong_to_the_handle(monkeypatch):
    """Three engines of one model in one process: A under the default environment, B with every PaiNN switch at its
    non-default value, C after the variables are gone again.  Each handle holds the selection of the environment it was created
    in (adf_painn_get_tune), whatever ran before it in the process.  210 rows: two full 96-row tiles of the streamed kernels
    + 18 rows, two 128-row tiles of the LDS-staged ones (the second ragged).  At H = 256 the layer products are multiples of
    256 wide with an even number of K tiles - streamed fragments by default, LDS-staged weights when switched; the heads'
    128-wide products take the LDS-staged kernel either way.
    B equals A bit for bit: the two forms keep the products of every output element and their order along K (tile shapes and
    the way the weights reach the registers differ), a row maximum is exact whether a producer emits it or a pass measures it,
    the separate gate kernel does the same single fp32 multiplication as the gate epilogue, and both CSR builds sort the same
    edges by the same key.  (The one-process-per-environment comparison on the parent library that was to confirm this
    before the assertion was written could not be run, profiles/NOTES.md; the notes of the commits that introduced the
    switches report identical benchmark sites for each.)"""
    for name, _, _ in SWITCHED:
        monkeypatch.delenv(name, raising=False)
    torch.manual_seed(0)
    hp = dict(hidden_channels=256, num_layers=2, num_rbf=128, max_neighbors=20, cutoff=6.0, so3_denoising=True)
    sd = PaiNN(None, 50, 1, **hp).state_dict()
    b = make_batch(2, n_slab=100, n_ads=5).to(DEV)
    assert b.pos.shape[0] == 210

    def run():
        m = PaiNN(None, 50, 1, **hp)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        f1, f2 = m(b.clone())
        return m, m.engine().get_tune(), f1.clone(), f2.clone()

    ma, ta, a1, a2 = run()
    for name, _, value in SWITCHED:
        monkeypatch.setenv(name, str(value))
    mb, tb, b1, b2 = run()
    for name, _, _ in SWITCHED:
        monkeypatch.delenv(name)
    mc, tc, c1, c2 = run()
    for t in (ta, tc):
        for field, value in DEFAULTS.items():
            assert t[field] == value, (field, t[field])
    for _, field, value in SWITCHED:
        assert tb[field] == value, (field, tb[field])
    # A's handle keeps its own selection after B was created (and still computes with it)
    assert ma.engine().get_tune() == ta
    assert torch.equal(a1, c1) and torch.equal(a2, c2)
    for t in (b1, b2):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    print("B against A: rel err", rel_err(b1.cpu(), a1.cpu()), rel_err(b2.cpu(), a2.cpu()))
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    del mb, mc


def test_plain_product_into_an_output_that_is_not_16_byte_aligned():
    """adf_launch_gemm16 without a gate through adf_linear_forward: an output that is 4-byte but not 16-byte aligned takes the
    kernel's scalar store branch and still gives the product (the alignment the launcher asks for belongs to the gate
    epilogue alone).  210 x 136: a ragged second row tile and a ragged column tile.  Bounds: those of
    test_linear_kernels_vs_fp64 for this arithmetic."""
    lib = L.load()
    M, N, K = 210, 136, 256
    g = torch.Generator().manual_seed(M + N)
    A = (torch.randn(M, K, generator=g) * 1.5).to(DEV)
    A[::7] *= 1e-3
    W = ((torch.rand(N, K, generator=g) - 0.5) * 0.15).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    buf = torch.full((M * N + 8,), 7.0, device=DEV)
    out = buf[1:1 + M * N].view(M, N)
    assert out.data_ptr() % 16 == 4
    L.check(lib.adf_linear_forward(A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, 1, 1,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    ref = torch.nn.functional.silu(A.double() @ W.double().t() + bias.double()) / 0.6
    scale = (A.double().abs() @ W.double().abs().t()).mean()
    err = float((out.double() - ref).abs().max() / scale)
    print("offset output: err", err, "rel", rel_err(out, ref))
    assert err < 6e-6 and rel_err(out, ref) < 3e-6
    assert float(buf[0]) == 7.0 and bool((buf[1 + M * N:] == 7.0).all())   # nothing written around it
