"""The PaiNN sampler forward (message.hip, gemm16.hip's fused epilogues, nodewise.hip, the heads) row by row against the
float64 oracle over the range adf_painn_create accepts: the cases of tests/helpers_painn_range.CASES - widths 192 .. 1024
(LDS-staged, mixed and streamed node products, partial head tiles, 16 channel slices), bases from 2 to 128 (multiples of 8
that are no multiple of 16, and even sizes that are no multiple of 8), envelope exponents 3 and 7, the message kernel with
every basis value by its own exp2 (ADF_MSG_RBF=direct), K = 1 and K = 128, 16 layers, a single head.

Each case runs in default arithmetic (f16x3 node products; the f16 message kernel wherever it can take the basis) and again
after ``use_exact_f32()`` on the same engine.  Reference: oracle/painn_oracle.py in float64 on the graph the engine exported.
Measures, each bounded by REL_TOL = 1e-4 (the project's parity budget) and printed with ``e32``, what the same evaluation in
float32 leaves in the same norm:
  1. teacher-forced blocks: ``message_layer`` / ``update_layer`` of every layer on the float64 forward's input of that block
     (rounded to float32), x [N, H] and vec [N, 3, H] row by row, |d row| / max(|row|, 1e-3 x largest row norm); rows that
     are exactly zero in the reference (atoms no edge has reached, ``k1``) are exact zeros, and their x after the first
     message block is x_in / sqrt 2 to one ulp;
  2. whole forward ``model(batch)``: every atom of f1 / f2 against the largest atom norm of its own system, the per-system
     adsorbate means against their own norm, ``forward_subset`` on the adsorbate rows bit-identical to the full forward;
  3. for three cases the S2EF PaiNN's energy (row-relative) and gradient forces (relative to max |F|).
A setting the kernels cannot take must raise ValueError before any output is written (the outputs keep their sentinel, the
next forward of a good model is clean); after this work no case of the table is refused.

Measured on an MI355X (profiles/painn_range_pytest_gpu.txt holds the run; worst device figure over all cases, its case, and
the e32 of that case in the same norm - evidence, not tolerances: every assertion stays at 1e-4):
  measure                      default arithmetic            after use_exact_f32()
  1. rows of x / vec           5.1e-6  r120  (e32 4.6e-6)    4.8e-6  r126  (e32 4.8e-6)
  2. atoms of f1 / f2          4.0e-6  p7    (e32 3.6e-6)    5.6e-6  h1024 (e32 1.4e-6)
     adsorbate means           6.1e-7  k128  (e32 9.5e-7)    8.8e-7  k128  (e32 9.5e-7)
  3. energy                    1.1e-6  h320  (e32 1.1e-6)    2.1e-6  h320  (e32 1.1e-6)
     gradient forces           6.1e-6  h320  (e32 3.5e-6)    4.1e-6  p3    (e32 4.0e-6)
k1 has 20 of 134 atoms without incoming edges, k128 a largest in-degree of 156.

What the test found when it first ran (both fixed with it):
  * num_rbf % 8 != 0 in default arithmetic returned finite, wrong numbers: worst row of the first message block 1.5e-1
    (r2), 1.7e-1 (r30), 8.0e-2 (r126); energy 3.9e-1 and gradient forces 1.6e-1 off for r30.  The f16 message kernel read
    its rbf_proj image in 16-byte pieces of 8 basis functions per column against rows of R halves.  Such handles now run the
    exact-f32 message kernel (adf_painn_create); afterwards r2 / r30 / r126 sit at 7e-7 ... 4.8e-6.
  * direct128 (ADF_MSG_RBF=direct, or non-linspace centres): two of 134 rows of a message block 1.09e-4 off, all others
    at 3e-6 (bases 64, 104, 112 alike; 24, 96, 120 clean).  The compiler split one basis value against two different fp16
    roundings of it, so that about one term in 2^13 was off by an fp16 ulp (message.hip, gen_a); afterwards 4.0e-6.
"""
import os

import pytest
import torch

from adsorbdiff_amd.engine import PaiNNEngine
from tests import helpers_painn_range as PR
from tests import helpers_train as HT
from tests.helpers_grad_forces import engine_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0
_SHARED = {}


def _batch():
    if "batch" not in _SHARED:
        b = PR.make_batch()
        _SHARED["batch"] = (b, b.clone().to(DEV))
    return _SHARED["batch"]


def _engine(name, m):
    """The model's engine, created under the case's environment; the environment is as it was afterwards."""
    before = os.environ.get("ADF_MSG_RBF")
    if PR.CASES[name]["direct"]:
        with PR.environment(ADF_MSG_RBF="direct"):
            eng = m.engine(DEV)
    else:
        eng = m.engine(DEV)
    assert os.environ.get("ADF_MSG_RBF") == before, "ADF_MSG_RBF not restored"
    return eng


def _good_model_is_clean():
    """After a refusal: a model the kernels take, on the same device, still meets its bounds."""
    b, bd = _batch()
    m = PR.make_model("p3").to(DEV)
    eng = m.engine(DEV)
    eng.build_graph(bd)
    graph = HT.graph_from_export(eng)
    r1, r2, _ = PR.forward("p3", m, b, graph, torch.float64)
    f1, f2 = m(bd)
    assert PR.head_figure(f1, r1, b.batch) < PR.REL_TOL and PR.head_figure(f2, r2, b.batch) < PR.REL_TOL


def _refused(name, exc, outputs):
    torch.cuda.synchronize()
    assert any(s in str(exc) for s in ("num_rbf", "hidden_channels", "max_neighbors", "num_layers", "envelope")), exc
    for t in outputs:
        assert t is None or bool((t == SENTINEL).all()), (name, "an output was written before the refusal")
    _good_model_is_clean()
    print("%s: refused cleanly (%s)" % (name, exc))


def _blocks(name, eng, inputs, ref, e32, label, first_layer_isolated, bad):
    """Measure 1 on a live engine whose graph is built.  Every figure is printed; what misses its bound goes to ``bad``."""
    worst, worst32 = 0.0, 0.0
    for l, (x_in, vec_in, x_mid, vec_mid) in enumerate(inputs):
        mx, mvec = eng.message_layer(l, x_in.to(DEV), vec_in.to(DEV))
        ux, uvec = eng.update_layer(l, x_mid.to(DEV).clone(), vec_mid.to(DEV).clone())
        torch.cuda.synchronize()
        for what, got, r, r32 in zip(("message x", "message vec", "update x", "update vec"), (mx, mvec, ux, uvec), ref[l], e32[l]):
            e, _, zero = PR.row_figures(got, r)
            f, _, _ = PR.row_figures(r32, r)
            print("%s [%s] layer %d %s: worst row %.2e (e32 %.2e)" % (name, label, l, what, e, f))
            worst, worst32 = max(worst, e), max(worst32, f)
            if not e < PR.REL_TOL:
                bad.append((label, "layer %d %s" % (l, what), e))
            if not PR.zero_rows_exact(got, zero):
                bad.append((label, "layer %d %s" % (l, what), "a row without incoming edges is not exactly zero"))
        if l == 0 and first_layer_isolated is not None:
            iso = first_layer_isolated
            if not bool((mvec[iso.to(DEV)] == 0).all()):
                bad.append((label, "vec rows without incoming edges after message layer 0 are not exact zeros"))
            if not PR.within_one_ulp(mx.cpu()[iso], x_in[iso].double() / 2.0 ** 0.5):
                bad.append((label, "x rows without incoming edges after message layer 0 are not x_in / sqrt 2 to one ulp"))
    return worst, worst32


def _whole(name, m, eng, b, bd, ref, e32, label, first, bad):
    """Measure 2; ``first`` = (f1, f2) that forward_prepared already gave in this arithmetic (same bits expected)."""
    out = m(bd)
    f1, f2 = out if PR.CASES[name]["so3"] else (out, None)
    torch.cuda.synchronize()
    figs = []
    for what, got, r, r32, fst in (("f1", f1, ref[0], e32[0], first[0]), ("f2", f2, ref[1], e32[1], first[1])):
        if r is None:
            assert got is None and name == "one_head"
            continue
        if not (fst is None or torch.equal(got, fst)):
            bad.append((label, what, "two forwards of one engine differ"))
        e, s = PR.head_figure(got, r, b.batch), PR.mean_figure(got, r, b)
        e_32, s_32 = PR.head_figure(r32, r, b.batch), PR.mean_figure(r32, r, b)
        print("%s [%s] %s: worst atom %.2e (e32 %.2e), adsorbate means %.2e (e32 %.2e)" % (name, label, what, e, e_32, s, s_32))
        if not e < PR.REL_TOL:
            bad.append((label, what + " worst atom", e))
        if not s < PR.REL_TOL:
            bad.append((label, what + " adsorbate means", s))
        figs.append((e, e_32, s, s_32))
    # forward_subset on the adsorbate rows: the same bits, nothing else written
    prep = eng.prepare(bd)
    N = bd.pos.shape[0]
    idx = torch.nonzero(bd.tags == 2).reshape(-1).to(torch.int32)
    s1 = torch.full((N, 3), SENTINEL, device=DEV)
    s2 = torch.full((N, 3), SENTINEL, device=DEV) if f2 is not None else None
    eng.forward_prepared(prep, bd.pos.float().contiguous(), s1, s2, idx)
    eng.check_flags()
    sel = idx.long()
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[sel] = False
    for full, sub in ((f1, s1), (f2, s2)):
        if full is not None:
            if not torch.equal(sub[sel], full[sel]):
                bad.append((label, "forward_subset differs from the full forward"))
            if not bool((sub[rest] == SENTINEL).all()):
                bad.append((label, "forward_subset wrote a row it was not asked for"))
    return figs


@pytest.mark.parametrize("name", list(PR.CASES))
def test_forward_row_by_row_vs_float64(name):
    c = PR.CASES[name]
    b, bd = _batch()
    m = PR.make_model(name).to(DEV)
    N = bd.pos.shape[0]
    f1 = torch.full((N, 3), SENTINEL, device=DEV)
    f2 = torch.full((N, 3), SENTINEL, device=DEV) if c["so3"] else None
    try:   # the contract: parity, or ValueError naming the setting before anything is written
        eng = _engine(name, m)
        prep = eng.prepare(bd)
        eng.forward_prepared(prep, bd.pos.float().contiguous(), f1, f2)
        eng.check_flags()
    except ValueError as exc:
        _refused(name, exc, (f1, f2))
        return
    assert not eng.exact_f32
    eng.build_graph(bd)
    graph = HT.graph_from_export(eng)
    PR.assert_structure(name, graph, b, eng.get_tune())
    r1, r2, cap = PR.forward(name, m, b, graph, torch.float64)
    g1, g2, _ = PR.forward(name, m, b, graph, torch.float32)
    inputs = PR.block_inputs(m, b, cap)
    ref = PR.forced_blocks(name, m, graph, inputs, torch.float64)
    e32 = PR.forced_blocks(name, m, graph, inputs, torch.float32)
    iso = None
    if name == "k1":
        iso = PR.in_degree(graph, N) == 0
        print("k1: %d of %d atoms without incoming edges" % (int(iso.sum()), N))
    if name == "k128":
        print("k128: largest in-degree %d" % int(PR.in_degree(graph, N).max()))
    if c["direct"]:   # the handle took the switch: an engine created without it gives other bits (same bound)
        other = PaiNNEngine(m, DEV)
        other.build_graph(bd)
        x_in, vec_in = inputs[-1][0].to(DEV), inputs[-1][1].to(DEV)
        a = eng.message_layer(c["L"] - 1, x_in, vec_in)
        o = other.message_layer(c["L"] - 1, x_in, vec_in)
        torch.cuda.synchronize()
        assert not (torch.equal(a[0], o[0]) and torch.equal(a[1], o[1])), "ADF_MSG_RBF=direct did not select another kernel"
        other.close()
    first = (f1, f2)
    bad = []
    for label in ("default", "exact f32"):
        if label == "exact f32":
            assert eng.use_exact_f32() and m.engine(DEV) is eng and eng.exact_f32
            first = (None, None)
        wb, wb32 = _blocks(name, eng, inputs, ref, e32, label, iso, bad)
        figs = _whole(name, m, eng, b, bd, (r1, r2), (g1, g2), label, first, bad)
        print("%s [%s] SUMMARY rows %.2e (e32 %.2e) atoms %.2e (e32 %.2e) means %.2e (e32 %.2e)" % (
            name, label, wb, wb32, max(f[0] for f in figs), max(f[1] for f in figs), max(f[2] for f in figs),
            max(f[3] for f in figs)))
    assert not bad, (name, bad)   # nothing is skipped: every row, atom, system and arithmetic was measured above


@pytest.mark.parametrize("name", PR.ENERGY_CASES)
def test_energy_and_gradient_forces_vs_float64(name):
    """forward_energy_gradient of the S2EF PaiNN (energy_grad.hip; message_geo.hip where it can take the basis) against
    float64 autograd on the engine's own edge list, with the bounds of tests/test_gpu_grad_forces.py."""
    b, bd = _batch()
    m = PR.make_model(name, energy=True).to(DEV)
    m.force_mode = "energy_gradient"
    N = bd.pos.shape[0]
    energy = torch.full((len(bd.natoms),), SENTINEL, device=DEV)
    forces = torch.full((N, 3), SENTINEL, device=DEV)
    try:
        eng = m.engine(DEV)
        eng.forward_energy_gradient_prepared(eng.prepare(bd), bd.pos.float().contiguous(), energy, forces)
        eng.check_flags()
    except ValueError as exc:
        _refused(name, exc, (energy, forces))
        return
    es, ed, vec = engine_graph(m, bd)
    e64, f64 = PR.energy_reference(name, m, b, es, ed, vec, torch.float64)
    e32, f32 = PR.energy_figures(*PR.energy_reference(name, m, b, es, ed, vec, torch.float32), e64, f64)
    for label in ("default", "exact f32"):
        if label == "exact f32":
            assert eng.use_exact_f32()
        out = m(bd)
        assert label == "exact f32" or (torch.equal(out["energy"], energy) and torch.equal(out["forces"], forces))
        e_err, f_err = PR.energy_figures(out["energy"], out["forces"], e64, f64)
        direct = eng.forward_energy(bd)[0]   # the energy forward alone: the same energy up to its head's unfused activation
        d_err = PR.energy_figures(direct, out["forces"], e64, f64)[0]
        print("%s [%s] SUMMARY energy row-rel %.2e (forward_energy %.2e, e32 %.2e), forces max-rel %.2e (e32 %.2e)" % (
            name, label, e_err, d_err, e32, f_err, f32))
        assert e_err < PR.REL_TOL and d_err < PR.REL_TOL, (name, label, e_err, d_err)
        assert f_err < PR.REL_TOL, (name, label, f_err)
