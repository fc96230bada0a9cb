"""The table of settings over adf_painn_create's accepted range that the sampler forward is tested at, and the float64 /
float32 references of every block and of the whole forward (tests/test_painn_range_host.py on the CPU,
tests/test_gpu_painn_range.py on the device).

Reference: oracle/painn_oracle.py (plain PyTorch, pinned to the reference function by function) in float64, on a graph
that is given - the oracle's own on the CPU, the engine's exported one on the device, so that ties at the K-th neighbour
are not part of the comparison.  "Teacher-forced": every message block and every update block is evaluated on the float64
forward's input of that block rounded to float32 - what the device is handed - so that an error of one block cannot hide
in, or be blamed on, the blocks before it.  The same evaluation in float32 gives ``e32``: what single precision itself
leaves in the norm at hand.

Norms.  A node tensor ([N, H] or [N, 3, H]) is compared row by row (a row = one atom): |d row| / max(|row|, ROW_FLOOR x
the largest row norm of that tensor).  A head output is compared atom by atom against the largest atom norm of the
atom's own system, the per-system adsorbate means (what the sampler reads) against their own norm.  Every bound is
REL_TOL = 1e-4, the project's parity budget."""
import contextlib
import math
import os

import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.synthetic import make_system
from oracle import painn_oracle as O
from tests import helpers_grad_forces as HG
from tests import helpers_train as HT
from tests.helpers import row_rel_err

REL_TOL = 1e-4        # every asserted bound
ROW_FLOOR = 1e-3      # rows below this share of the tensor's largest row norm are measured against the floor ...
FLOOR_SHARE = 0.10    # ... and at most this share of a reference tensor's rows may lie there
HOST_MARGIN = 4.0     # the float32 oracle stays inside every bound by this factor (test_painn_range_host.py)

# four systems of (slab, adsorbate) atoms: 134 atoms (no multiple of 32, 64 or 96), a 1-atom adsorbate, self-image edges
SYSTEMS = ((36, 4), (7, 1), (61, 3), (20, 2))
_BASE = dict(H=128, L=2, R=128, cutoff=6.0, K=20, p=5, direct=False, so3=True)


def _case(**kw):
    return dict(_BASE, **kw)


# name -> setting; what each one reaches is in the comment
CASES = {
    # every node product runs LDS-staged; the heads' 96-wide products are partial column tiles; three channel slices
    "h192": _case(H=192),
    # the same with 160-wide head products, five channel slices, a basis that is a multiple of 32 but not of 64
    "h320": _case(H=320, R=96),
    # one forward mixes both tile forms: the 3H- and 2H-wide products stream, the H-wide ones run LDS-staged
    "h384": _case(H=384),
    # ten channel slices, 1920-wide streamed products; the only layer is the vec == 0 one
    "h640": _case(H=640, L=1, R=64),
    # the upper end of the accepted width: 16 channel slices
    "h1024": _case(H=1024),
    # bases that are multiples of 8 but not of 16: the window rounding and clamp of the f16 message kernel
    "r8": _case(R=8),
    "r24": _case(R=24),
    "r40": _case(R=40),
    "r120": _case(R=120),
    # even bases that are no multiple of 8: the fp16 image's 16-byte pieces do not fit their rows
    "r2": _case(R=2),
    "r30": _case(R=30),
    "r126": _case(R=126),
    # envelope exponents other than the shipped 5: the repeated-multiplication loop
    "p3": _case(p=3),
    "p7": _case(p=7),
    # the UNI = false instantiations of the message kernel (every basis value by its own exp2)
    "direct128": _case(direct=True),
    "direct24": _case(R=24, direct=True),
    # one neighbour per atom: many targets without incoming edges
    "k1": _case(K=1),
    # the neighbour cap at its upper end: in-degree above 128 after symmetrisation
    "k128": _case(K=128, cutoff=9.0),
    # the upper end of the accepted depth
    "l16": _case(L=16),
    # a single head (so3_denoising=False) at a width whose head products are partial tiles
    "one_head": _case(H=192, so3=False),
}
# energy forward and gradient forces (the S2EF PaiNN): a basis outside the fused kernels, the envelope derivative for
# p != 5, a width of five channel slices
ENERGY_CASES = ("r30", "p3", "h320")
SCALE_FACTORS = HT.SCALE_FACTORS + (1.04, 0.96, 1.08, 0.93, 1.03, 0.98, 1.06, 0.94, 1.015, 0.985)   # sixteen, none of them 1
assert len(SCALE_FACTORS) == 16


@contextlib.contextmanager
def environment(**kv):
    """Set environment variables for the block and put back what was there."""
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


def make_batch():
    g = torch.Generator().manual_seed(4242)
    return Batch.from_data_list([make_system(g, n_slab, n_ads, sid=str(i)) for i, (n_slab, n_ads) in enumerate(SYSTEMS)])


def make_model(name, energy=False):
    """The mirror model of a case on the CPU by the recipe of helpers_train.make_config_model: seeded initialisers, biases
    and LayerNorm parameters moved off their constants, trained-like rescale, scale factors different from 1.
    ``energy``: the S2EF PaiNN (energy head + one force head) instead of the denoiser."""
    from adsorbdiff_amd.painn import PaiNN as S2EF
    from adsorbdiff_amd.painn_denoising import PaiNN as Denoiser

    c = CASES[name]
    torch.manual_seed(7)
    kw = dict(hidden_channels=c["H"], num_layers=c["L"], num_rbf=c["R"], cutoff=c["cutoff"], max_neighbors=c["K"],
              envelope={"name": "polynomial", "exponent": c["p"]},
              scale_file={"upd_out_scalar_scale_%d" % i: SCALE_FACTORS[i] for i in range(c["L"])})
    m = S2EF(None, 50, 1, **kw) if energy else Denoiser(None, 50, 1, so3_denoising=c["so3"], **kw)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if n_.endswith("bias") or "layernorm" in n_:
                p_.add_(0.1 * torch.randn(p_.shape, generator=g))
    HT.trained_like_rescale_(m)
    assert all(abs(s - 1.0) > 1e-3 for s in m.scale_factors()) and len(m.scale_factors()) == c["L"]
    assert int(m.radial_basis.envelope.p) == c["p"]
    return m.eval()


def oracle_graph(name, batch):
    c = CASES[name]
    return O.generate_graph_values(batch.pos.float(), batch.cell.float().reshape(-1, 3, 3), batch.natoms, c["cutoff"], c["K"])


def in_degree(graph, num_atoms):
    return torch.bincount(graph[0][1], minlength=num_atoms)


def assert_structure(name, graph, batch, tune=None):
    """The property a case exists for, on the graph at hand (and, on the device, on the handle's kernel selection)."""
    c = CASES[name]
    N = int(batch.pos.shape[0])
    assert N == 134 and int((batch.tags == 2).sum(0)) == 10
    indeg = in_degree(graph, N)
    if name == "k1":   # (the one neighbour kept is never the atom's own image)
        assert int((indeg == 0).sum()) > 0, "every atom has an incoming edge"
    else:
        assert int(indeg.min()) > 0
        assert int((graph[0][0] == graph[0][1]).sum()) > 0, "no self-image edge"
    if name == "k128":
        assert int(indeg.max()) > 128, int(indeg.max())
    if name == "h384":
        H = c["H"]
        assert (3 * H) % 384 == 0 and H % 256 != 0
        if tune is not None:
            assert tune["gemm_stream"] == 1


# ------------------------------------------------------------------------------------------------------ references
def _state(model, dtype):
    return {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}


def forward(name, model, batch, graph, dtype):
    """The whole forward by the oracle in ``dtype`` on ``graph`` -> (f1 [N,3], f2 [N,3] or None, capture)."""
    c = CASES[name]
    ei, nb, dist, unit = graph
    cap = {}
    out = O.painn_forward(_state(model, dtype), batch.pos.cpu().to(dtype), batch.atomic_numbers.cpu(), batch.cell.cpu().to(dtype),
                          batch.natoms.cpu(), hidden_channels=c["H"], num_layers=c["L"], num_rbf=c["R"], cutoff=c["cutoff"],
                          max_neighbors=c["K"], scale_factors=model.scale_factors(), so3_denoising=c["so3"],
                          graph=(ei, nb, dist.to(dtype), unit.to(dtype)), capture=cap, envelope_exponent=c["p"])
    f1, f2 = out if c["so3"] else (out, None)
    return f1.reshape(-1, 3), None if f2 is None else f2.reshape(-1, 3), cap


def block_inputs(model, batch, cap64):
    """Per layer, what enters its message block and its update block in the float64 forward, rounded to float32:
    [(x_in [N,H], vec_in [N,3,H], x_mid, vec_mid)].  vec_in of layer 0 is zero."""
    z = batch.atomic_numbers.cpu().long()
    x = model.atom_emb.embeddings.weight.detach().cpu().double()[z - 1]
    vec = torch.zeros(x.shape[0], 3, x.shape[1], dtype=torch.float64)
    out = []
    for lay in cap64["layers"]:
        x_mid = (x + lay["msg_dx"]) * (1 / math.sqrt(2.0))
        vec_mid = vec + lay["msg_dvec"]
        out.append(tuple(t.float().contiguous() for t in (x, vec, x_mid, vec_mid)))
        x, vec = lay["x"], lay["vec"]
    return out


def forced_blocks(name, model, graph, inputs, dtype):
    """Every block of the oracle in ``dtype`` on the float32 ``inputs`` of block_inputs: per layer
    (x, vec after the message block and its residual, x, vec after the update block and its scale factor)."""
    c = CASES[name]
    H = c["H"]
    sd = _state(model, dtype)
    ei, _, dist, unit = graph
    rbf = O.radial_basis(dist.to(dtype), c["cutoff"], c["R"], c["p"])
    sf = model.scale_factors()
    out = []
    for l, (x_in, vec_in, x_mid, vec_mid) in enumerate(inputs):
        x, vec = x_in.to(dtype), vec_in.to(dtype)
        dx, dvec = O.message_layer(sd, "message_layers.%d." % l, x, vec, ei, rbf, unit.to(dtype), H)
        mx, mvec = (x + dx) * (1 / math.sqrt(2.0)), vec + dvec
        x, vec = x_mid.to(dtype), vec_mid.to(dtype)
        dx, dvec = O.update_layer(sd, "update_layers.%d." % l, x, vec, H)
        out.append((mx, mvec, (x + dx) * sf[l], vec + dvec))
    return out


# ------------------------------------------------------------------------------------------------------ measures
def row_figures(got, ref):
    """(worst row error, share of non-zero reference rows under the floor, mask of exactly-zero reference rows) of a node
    tensor against its reference: |d row| / max(|row|, ROW_FLOOR x largest row norm).  No row is left out."""
    n = ref.shape[0]
    g, r = got.detach().cpu().double().reshape(n, -1), ref.detach().cpu().double().reshape(n, -1)
    rn = r.norm(dim=1)
    floor = ROW_FLOOR * float(rn.max())
    assert floor > 0 and bool(torch.isfinite(g).all())
    err = (g - r).norm(dim=1) / rn.clamp(min=floor)
    zero = rn == 0
    share = float(((rn < floor) & ~zero).double().mean())
    return float(err.max()), share, zero


def head_figure(got, ref, batch_index):
    """max over atoms of |d f| / the largest atom norm of the atom's own system."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    bi = batch_index.cpu().long()
    B = int(bi.max()) + 1
    top = torch.zeros(B, dtype=torch.float64).scatter_reduce_(0, bi, r.norm(dim=1), "amax", include_self=True)
    assert float(top.min()) > 0 and bool(torch.isfinite(g).all())
    return float(((g - r).norm(dim=1) / top[bi]).max())


def mean_figure(got, ref, batch):
    """row_rel_err of the per-system means over adsorbate atoms (oracle's ads_mean: what the sampler reads)."""
    B = int(batch.natoms.shape[0])
    tags, bi = batch.tags.cpu(), batch.batch.cpu().long()
    return row_rel_err(O.ads_mean(got.detach().cpu().double(), tags, bi, B), O.ads_mean(ref.detach().cpu().double(), tags, bi, B))


def zero_rows_exact(got, zero):
    """Rows that are exactly zero in the reference (atoms that no edge has reached yet) hold exact zeros."""
    return bool((got.detach().cpu().reshape(got.shape[0], -1)[zero] == 0).all())


def within_one_ulp(got, expected64):
    """|got - expected| <= the float32 spacing at expected, element by element."""
    e32 = expected64.float()
    ulp = (torch.nextafter(e32.abs(), torch.full_like(e32, float("inf"))) - e32.abs()).double()
    return bool(((got.detach().cpu().double() - expected64).abs() <= ulp).all())


# ------------------------------------------------------------------------------------------------------ energy
def energy_reference(name, model, batch, es, ed, vec, dtype):
    """(energy [B], forces [N,3]) of the S2EF model by helpers_grad_forces.energy_forces in ``dtype`` on the edge list
    (es, ed, vec) - the engine's exported one on the device, the oracle's on the CPU."""
    c = CASES[name]
    bc = batch.to("cpu")
    off = HG.edge_offsets(bc.pos, bc.cell, bc.batch, es, ed, vec)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return HG.energy_forces(sd, bc.pos, bc.atomic_numbers, bc.batch, len(bc.natoms), es, ed, off, hidden_channels=c["H"],
                            num_layers=c["L"], num_rbf=c["R"], cutoff=c["cutoff"], scale_factors=model.scale_factors(),
                            envelope_exponent=c["p"], dtype=dtype)


def energy_figures(energy, forces, e_ref, f_ref):
    """The measures of tests/test_gpu_grad_forces.py: energy row-relative, forces relative to max |F|."""
    e_err = row_rel_err(energy.detach().cpu().reshape(-1, 1), e_ref.reshape(-1, 1))
    f, r = forces.detach().cpu().double(), f_ref.double()
    return e_err, float((f - r).abs().max() / r.abs().max())
