"""The device's radius graph (csrc/graph.hip) against a float64 brute-force neighbour search on hard cells
(tests/helpers_graph_hard.py: the case table, the band tau and the 5 % condition on boundary centres).

Branches no other test runs, and the case that reaches each: adf_topk_kernel with C > 128 shifts (cached == false) -
uncached147, unwrapped147, k1/k64/k65, seam256, close_pair, one_atom (C = 147), triclinic245 (245), bulk343* / near_cap (343);
C > CSR_C_MAX - bulk343, bulk343_k128, near_cap; K > CSR_K_MAX - k65, bulk343_k128 (K = ADF_MAX_K), K == CSR_K_MAX - k64,
K == 1 - k1; the CSR_SYS_MAX seam - seam256 (256 and 257 atoms); the candidate-overflow flag - overflow, with near_cap
just below it (15 rounds of 64); static-atom cache modes 1 / 2 with 147, 343 and 75 shifts and an atom that leaves the
cell - test_static_cache_on_hard_cells; nine non-zero cell entries, shifts of +-3, unwrapped positions - triclinic245,
all 12 A cases, unwrapped147; pbc (T,T,F) / (T,F,F) / (F,F,F) - pbc_ttf / pbc_tff / pbc_fff.

Measured on an MI355X, the device's lists: boundary share 0.0038 on seam256 (2 of 521 centres) and 0 on every other case;
worst |d^2 - float64| / tau 0.006 on tie and 0.000 elsewhere (the lists are the float32 oracle's wherever its offsets
are exact); dist within 1.79e-6 (seam256; 1.5e-6 one_atom, at most 1.1e-6 elsewhere) and vec within 1.22e-6 of float64.
"""
import functools
import os

import numpy as np
import pytest
import torch

from adsorbdiff_amd.painn_denoising import PaiNN
from tests import helpers_graph_hard as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOT_OVERFLOW = tuple(n for n in H.CASES if n != "overflow")
# limits of the per-system LDS kernels of the CSR build (graph.hip: CSR_SYS_MAX, CSR_K_MAX, CSR_C_MAX)
CSR_SYS_MAX, CSR_K_MAX, CSR_C_MAX = 256, 64, 256

_ENGINES = {}


def engine(cutoff, K, mode, which=0):
    """One small PaiNN (H = 128, one layer) per (cutoff, K, ADF_GRAPH_SYS_CSR mode); the switch belongs to the handle."""
    key = (cutoff, K, mode, which)
    if key not in _ENGINES:
        old = os.environ.get("ADF_GRAPH_SYS_CSR")
        os.environ["ADF_GRAPH_SYS_CSR"] = str(mode)
        try:
            torch.manual_seed(0)
            m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, cutoff=cutoff, max_neighbors=K, so3_denoising=True).to(DEV).eval()
            eng = m.engine()
        finally:
            if old is None:
                del os.environ["ADF_GRAPH_SYS_CSR"]
            else:
                os.environ["ADF_GRAPH_SYS_CSR"] = old
        _ENGINES[key] = (m, eng)
    eng = _ENGINES[key][1]
    assert eng.get_tune()["graph_sys_csr"] == mode
    return eng


def export(eng):
    """The seven exported tensors as numpy, list slots beyond a centre's count set to -1 (they are never written)."""
    cnt, src, sh, es, ed, dist, vec = [t.cpu().numpy() for t in eng.export_graph()]
    pad = np.arange(src.shape[1])[None, :] >= cnt[:, None]
    src, sh = src.copy(), sh.copy()
    src[pad], sh[pad] = -1, 0
    return dict(cnt=cnt, src=src, shift=sh, es=es, ed=ed, dist=dist, vec=vec)


@functools.lru_cache(maxsize=None)
def built(name, mode):
    c = H.case(name)
    eng = engine(c.cutoff, c.K, mode)
    E = eng.build_graph(c.batch.clone().to(DEV))
    eng.check_flags()
    g = export(eng)
    assert E == g["es"].shape[0]
    return g


@functools.lru_cache(maxsize=None)
def oracle(name):
    return H.oracle_graph(H.case(name))


def directed(c, g, pos=None, stats=None):
    b = c.batch
    return H.check_directed(b.pos if pos is None else pos, b.cell, b.natoms, c.cutoff, c.K, c.pbc, g["cnt"], g["src"], g["shift"],
                            stats)


@pytest.mark.parametrize("name", NOT_OVERFLOW)
def test_directed_lists_vs_fp64(name):
    """build_graph, check_flags, export_graph, then rules 1-4 of check_directed on the device's lists."""
    c, g, st = H.case(name), built(name, 1), {}
    share = directed(c, g, stats=st)
    print(f"{name}: boundary share {share:.4f}, worst |dd2|/tau {st['worst']:.3f}")
    if name != "close_pair":
        assert share <= H.MAX_BOUNDARY_SHARE, share
        return
    # the planted atoms one by one: the 0.009 A partner absent, the 0.011 A partner present, neither a boundary centre
    for (i, j, _), listed in zip(H.CLOSE_PAIRS, (False, True)):
        for x, y in ((i, j), (j, i)):
            k = int(g["cnt"][x])
            assert bool(np.any((g["src"][x, :k] == y) & (g["shift"][x, :k] == 0).all(1))) == listed, (x, y)
    assert not st["boundary"][[8, 9, 10, 11]].any()


@pytest.mark.parametrize("name", [n for n in NOT_OVERFLOW if H.offsets_exact(H.case(n))])
def test_exact_order_where_offsets_are_exact(name):
    """Where torch.bmm gives the bits of the kernel's unfused offset chain (offsets_exact on the CPU this runs on: every skew
    cell at every shift, pinned by tests/test_graph_hard_host.py; triclinic245 on some CPUs only), the d^2 of both sides
    are the same floats and both break ties by candidate index: counts, sources and shifts equal the float32 oracle's, the
    exactly tied +s / -s self images of the small cells and the lattice of `tie` included."""
    g, o = built(name, 1), oracle(name)
    assert np.array_equal(g["cnt"], o["cnt"])
    assert np.array_equal(g["src"], o["src"]), "top-K neighbour lists differ from the oracle"
    assert np.array_equal(g["shift"], o["shift"])


def lds_path(c):
    """Per system: can it take the per-system LDS kernels (csr_fits of graph.hip)?"""
    _, sh = H.shift_tables(c.batch.cell, c.cutoff, c.pbc)
    return [n <= CSR_SYS_MAX and c.K <= CSR_K_MAX and sh.shape[0] <= CSR_C_MAX for n in c.batch.natoms.tolist()]


@pytest.mark.parametrize("name", NOT_OVERFLOW)
def test_symmetrised_graph(name):
    """check_symmetrised on the export of both CSR builds, which must be the same bytes.  From the case table: k65 (K),
    bulk343 (C) and the 257-atom system (n) cannot take the LDS path, their neighbours in the table can."""
    c, b = H.case(name), H.case(name).batch
    g0, g1 = built(name, 0), built(name, 1)
    for g in (g0, g1):
        r = H.check_symmetrised(g["cnt"], g["src"], g["shift"], g["es"], g["ed"], g["dist"], g["vec"], b.pos, b.cell, b.natoms)
    print(f"{name}: E {r['E']}, dist err {r['err_dist']:.2e}, vec err {r['err_vec']:.2e}")
    for k in g0:
        assert g0[k].shape == g1[k].shape and g0[k].tobytes() == g1[k].tobytes(), k
    want = dict(k65=[False], bulk343=[False], bulk343_k128=[False], near_cap=[False], triclinic245=[True], k64=[True], k1=[True],
                uncached147=[True], seam256=[True, True, False], one_atom=[True, True])
    if name in want:
        assert lds_path(c) == want[name]


@pytest.mark.parametrize("name", ["uncached147", "bulk343", "tie"])
def test_static_cache_on_hard_cells(name):
    """Cache modes 1 / 2 of adf_topk_kernel with 147, 343 and 75 shifts: the last two atoms move three times (the cache is
    filled once), the second move carries the last atom across the cell face by 1.3 lattice vectors; every incremental
    build equals a full rebuild on a second engine in all seven exported tensors and passes the float64 check."""
    c = H.case(name)
    base = c.batch.clone().to(DEV)
    N = base.pos.shape[0]
    inc_eng, full_eng = engine(c.cutoff, c.K, 1), engine(c.cutoff, c.K, 1, which=1)
    mask = torch.zeros(N, dtype=torch.bool, device=DEV)
    mask[-2:] = True
    prep = inc_eng.prepare(base)
    inc_eng.set_moving_atoms(prep, mask)
    try:
        inc_eng.build_graph(base, prep)   # full evaluation + cache fill
        gen = torch.Generator().manual_seed(5)
        a = base.cell[0, 0].cpu()
        moves = [(torch.rand(2, 3, generator=gen) - 0.5) * 2.0,
                 torch.stack([torch.zeros(3), 1.3 * a]),
                 (torch.rand(2, 3, generator=gen) - 0.5) * 4.0]
        moved = base.clone()
        for step in moves:
            moved.pos[-2:] = moved.pos[-2:] + step.to(DEV)
            E_inc = inc_eng.build_graph(moved, prep)
            inc_eng.check_flags()
            inc = export(inc_eng)
            E_full = full_eng.build_graph(moved)
            full = export(full_eng)
            assert E_inc == E_full
            for k in inc:
                assert torch.equal(torch.from_numpy(inc[k]), torch.from_numpy(full[k])), k
            share = directed(c, inc, pos=moved.pos)
            assert share <= H.MAX_BOUNDARY_SHARE, share
        frac = torch.linalg.solve(base.cell[0].double().t(), moved.pos[-1].double())
        assert float(frac[0]) > 1.0        # the atom did leave the cell
    finally:
        inc_eng.set_moving_atoms(None, None)


def test_candidate_overflow_is_reported():
    """More than TOPK_CAP = 1024 in-cutoff candidates around a centre is an error that names the capacity, not a list cut
    at 1024 candidates; the flag is cleared by the report, so the next build on the same engine (near_cap, 913 of 1024
    candidates) is clean and right."""
    over, near = H.case("overflow"), H.case("near_cap")
    eng = engine(over.cutoff, over.K, 1)
    with pytest.raises(ValueError, match="1024 in-cutoff candidates"):
        eng.build_graph(over.batch.clone().to(DEV))
        eng.check_flags()
    eng.build_graph(near.batch.clone().to(DEV))
    eng.check_flags()
    assert directed(near, export(eng)) <= H.MAX_BOUNDARY_SHARE
