"""References for the EquiformerV2 training step (tests/test_eqv2_train_host.py, tests/test_gpu_eqv2_train*.py).

Everything here is float64 (or float32, for the calibration) torch.autograd on the CPU through oracle/eqv2_oracle.py:
the whole forward ``eqv2_forward`` for the plain step, and - for dropout / drop-path masks and the conditional model's
energy term, which the oracle's forward does not have - a restatement of its block loop (``forward_restated``) that the
host test asserts equal to ``eqv2_forward`` when nothing is masked.  The operator tests take the oracle's pieces one by one
on the DEVICE's own edge list and Wigner rows, so an edge's frame (any roll about the edge is a valid one) is the device's.
"""
import math

import torch
import torch.nn.functional as F

from oracle import eqv2_oracle as Q
from oracle import train_oracle as TO
from tests.helpers_eqv2_ragged import (K, MODELS, REL_TOL, SPARSE_CUTOFF, TIGHT_FACTOR, frob, make, one_system_batch, ragged_graph,
                                       sparse_batch)
from tests.helpers_train import igso3_tables, make_targets

__all__ = ["K", "MODELS", "REL_TOL", "TIGHT_FACTOR", "frob", "make", "ragged_graph", "sparse_batch", "make_targets",
           "igso3_tables"]


def hp_of(m):
    return dict(lmax=m.lmax_list[0], mmax=m.mmax_list[0], num_layers=m.num_layers, sphere_channels=m.sphere_channels,
                attn_hidden_channels=m.attn_hidden_channels, num_heads=m.num_heads,
                attn_alpha_channels=m.attn_alpha_channels, attn_value_channels=m.attn_value_channels,
                ffn_hidden_channels=m.ffn_hidden_channels, grid_resolution=m.grid_resolution, max_radius=m.max_radius,
                max_neighbors=m.max_neighbors)


def train_model(name, two_heads=True, conditional=False, seed=0, cutoff=12.0, alpha_drop=0.0, drop_path_rate=0.0):
    """``MODELS[name]`` (tests/helpers_eqv2_ragged.py) as a trainable mirror: biases, norm weights and alpha_dot moved off
    their constants so that every parameter's gradient is a generic number."""
    from adsorbdiff_amd.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos

    c = MODELS[name]
    torch.manual_seed(seed)
    m = EquiformerV2S_OC20_DenoisingPos(
        None, None, None, max_neighbors=K, max_radius=cutoff, max_num_elements=90, num_layers=c["layers"],
        sphere_channels=c["C"], attn_hidden_channels=c["hidden"], num_heads=c["heads"], attn_alpha_channels=c["alpha"],
        attn_value_channels=c["value"], ffn_hidden_channels=c["ffn"], norm_type="layer_norm_sh", lmax_list=[c["lmax"]],
        mmax_list=[c["mmax"]], grid_resolution=18, edge_channels=c["ec"], attn_activation="silu", ffn_activation="silu",
        use_grid_mlp=True, use_sep_s2_act=True, alpha_drop=alpha_drop, drop_path_rate=drop_path_rate, weight_init="uniform",
        FOR_denoising=True, so3_denoising=two_heads, energy_encoding="scalar" if conditional else None)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n == "atom_radii":
                continue
            if n.endswith("source_embedding.weight") or n.endswith("target_embedding.weight"):
                p.mul_(300.0)      # trained-like magnitudes (tests/test_gpu_eqv2.py::make_model)
            if n.endswith("bias") or n.endswith("norm_l0.weight") or n.endswith("affine_weight") or ".net.1." in n or ".net.4." in n \
                    or n.endswith("alpha_norm.weight"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m.train()


def tagged(batch):
    """Every system gets adsorbate atoms (tag 2): its first and, where it has three or more atoms, its third."""
    off = 0
    batch.tags = torch.ones(int(batch.pos.shape[0]), dtype=torch.long)
    for n in batch.natoms.tolist():
        batch.tags[off] = 2
        if n >= 3:
            batch.tags[off + 2] = 2
        off += n
    return batch


def ragged_case():
    """(batch carrying the ragged graph's elements, edge_index, edge_vec) - used through ``engine.set_edges``."""
    ei, vec, Z = ragged_graph()
    b = tagged(one_system_batch(Z))
    b.tags[18] = 2    # the 128-edge hub is an adsorbate atom: its gradient reaches the loss directly
    return b, ei, vec


# ------------------------------------------------------------------------------------------------ restated forward
def attention_block_masked(sd, pre, x, Z, basis, src, dst, D, hp, grids, mask=None):
    """``Q.attention_block`` line by line, with the dropout mask [E, heads] (already divided by keep) on alpha."""
    L, M = hp["lmax"], hp["mmax"]
    H, A, V, hid = hp["num_heads"], hp["attn_alpha_channels"], hp["attn_value_channels"], hp["attn_hidden_channels"]
    N = x.shape[0]
    rm = Q.reduced_mask(L, M)
    scal = torch.cat([basis, sd[pre + "source_embedding.weight"][Z[src]], sd[pre + "target_embedding.weight"][Z[dst]]], dim=1)
    msg = torch.cat([x[src], x[dst]], dim=2)
    msg = torch.bmm(D[:, rm, :], msg)
    radial = Q.radial_mlp(sd, pre + "so2_conv_1.rad_func.", scal)
    msg, ex = Q.so2_conv(sd, pre + "so2_conv_1.", msg, L, M, hid, radial, extra=H * A + hid)
    alpha_in, gate = ex[:, :H * A], ex[:, H * A:]
    g = torch.einsum("bai,zic->zbac", grids.to_red, msg)
    act = torch.einsum("bai,zbac->zic", grids.from_red, F.silu(g))
    msg = torch.cat([F.silu(gate)[:, None, :], act[:, 1:]], dim=1)
    msg = Q.so2_conv(sd, pre + "so2_conv_2.", msg, L, M, H * V, None)
    a = Q.layer_norm(alpha_in.reshape(-1, H, A), sd[pre + "alpha_norm.weight"], sd[pre + "alpha_norm.bias"])
    a = torch.einsum("ehk,hk->eh", Q.smooth_leaky_relu(a), sd[pre + "alpha_dot"])
    a = Q.segment_softmax(a, dst, N)
    if mask is not None:
        a = a * mask
    msg = (msg.reshape(msg.shape[0], -1, H, V) * a[:, None, :, None]).reshape(msg.shape[0], -1, H * V)
    back = D.transpose(1, 2)[:, :, rm] * Q.truncation_rescale(L, M, D.dtype)[None, None, :]
    msg = torch.bmm(back, msg)
    agg = torch.zeros(N, msg.shape[1], msg.shape[2], dtype=msg.dtype).index_add_(0, dst, msg)
    return Q.so3_linear(sd, pre + "proj.", agg, L)


def energy_term(sd, energy, sysidx, dtype):
    """The conditional model's per-atom term: the VALUE the fp16 layer gives, the gradient of e W + b."""
    W, b = sd["energy_embedding.weight"].reshape(-1), sd["energy_embedding.bias"]
    e = energy.to(dtype)
    t = e[:, None] * W[None, :] + b[None, :]
    t16 = (energy.half().float()[:, None] * W.detach().float().half().float()[None, :]
           + b.detach().float().half().float()[None, :]).half().float().to(dtype)
    return (t + (t16 - t).detach())[sysidx]


def forward_restated(sd, hp, Z, graph, dtype, sysidx=None, alpha_masks=None, path_masks=None, rates=(0.0, 0.0), energy=None):
    """The block loop of ``Q.eqv2_forward`` (basis identically zero) with dropout on alpha, drop path on both branches
    (``x / keep * mask`` per graph) and the conditional model's energy term.  sd already in ``dtype``."""
    L, M, C = hp["lmax"], hp["mmax"], hp["sphere_channels"]
    Z = Z.long()
    N = Z.shape[0]
    ei, v = graph
    v = v.to(dtype)
    src, dst = ei[0], ei[1]
    pa, pp = rates
    basis = torch.zeros(v.shape[0], 600, dtype=dtype)
    D = Q.wigner_from_rotation(L, Q.edge_frames(v))
    grids, S = Q.Grids(L, M, hp["grid_resolution"], dtype), (L + 1) ** 2
    x = torch.zeros(N, S, C, dtype=dtype)
    x0 = sd["sphere_embedding.weight"][Z]
    if energy is not None:
        x0 = x0 + energy_term(sd, energy, sysidx, dtype)
    pre = "edge_degree_embedding."
    scal = torch.cat([basis, sd[pre + "source_embedding.weight"][Z[src]], sd[pre + "target_embedding.weight"][Z[dst]]], dim=1)
    m0 = Q.radial_mlp(sd, pre + "rad_func.", scal).reshape(-1, L + 1, C)
    red = Q.lm_list(L, M)
    cols = torch.tensor([red.index((l, 0)) for l in range(L + 1)])
    rm = Q.reduced_mask(L, M)
    back = (D.transpose(1, 2)[:, :, rm] * Q.truncation_rescale(L, M, dtype)[None, None, :])[:, :, cols]
    deg = torch.zeros(N, S, C, dtype=dtype).index_add_(0, dst, torch.bmm(back, m0)) / Q.AVG_DEGREE
    x = torch.cat([deg[:, :1] + x0[:, None, :], deg[:, 1:]], dim=1)
    for i in range(hp["num_layers"]):
        p = f"blocks.{i}."
        am = None if alpha_masks is None or pa == 0.0 else alpha_masks[i].to(dtype) / (1.0 - pa)
        y = attention_block_masked(sd, p + "ga.", Q.norm_sh(sd, p + "norm_1.", x, L), Z, basis, src, dst, D, hp, grids, am)
        if path_masks is not None and pp > 0.0:
            y = y * (path_masks[i, 0].to(dtype) / (1.0 - pp))[sysidx][:, None, None]
        x = x + y
        y = Q.feed_forward(sd, p + "ffn.", Q.norm_sh(sd, p + "norm_2.", x, L), hp, grids)
        if path_masks is not None and pp > 0.0:
            y = y * (path_masks[i, 1].to(dtype) / (1.0 - pp))[sysidx][:, None, None]
        x = x + y
    x = Q.norm_sh(sd, "norm.", x, L)
    f1 = attention_block_masked(sd, "force_block.", x, Z, basis, src, dst, D, hp, grids)[:, 1:4, 0]
    f2 = attention_block_masked(sd, "force_block2.", x, Z, basis, src, dst, D, hp, grids)[:, 1:4, 0]
    return f1, f2


# ------------------------------------------------------------------------------------------------ loss + gradients
def reference_step(model, batch, targets, graph, dtype=torch.float64, masks=None, restated=False):
    """loss (3), outputs and {name: gradient | None} of the score-matching step by autograd in ``dtype`` on the edge list
    ``graph`` = (edge_index [2, E], edge_vec [E, 3]).  Plain cases go through ``Q.eqv2_forward``; masks, the conditional
    model or ``restated`` through ``forward_restated``."""
    _, oracle_tables = igso3_tables()
    two_heads = bool(model.so3_denoising)
    conditional = getattr(model, "energy_embedding", None) is not None
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    sd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    leaves = {k: sd[k].clone().requires_grad_(True) for k in names}
    sd.update(leaves)
    hp = hp_of(model)
    b = batch
    ei, v = graph[0].cpu().long(), graph[1].cpu().float()
    sysidx = b.batch.cpu().long()
    if masks is not None or conditional or restated:
        rates = (float(model.alpha_drop), float(model.drop_path_rate)) if masks is not None else (0.0, 0.0)
        energy = None
        if conditional:
            energy = torch.zeros(int(b.natoms.numel())) if model.sampling else b.energy.cpu().float().reshape(-1)
        f1, f2 = forward_restated(sd, hp, b.atomic_numbers.cpu(), (ei, v), dtype, sysidx,
                                  None if masks is None else [m_.cpu() for m_ in masks["alpha"]],
                                  None if masks is None else masks["path"].cpu(), rates, energy)
    else:
        f1, f2 = Q.eqv2_forward(sd, hp, b.pos.cpu().float(), b.atomic_numbers.cpu(), b.cell.cpu().float().reshape(-1, 3, 3),
                                b.natoms.cpu(), graph=(ei, v), dtype=dtype)
    noised = {k: targets[k].cpu().float().to(dtype) for k in ("tr_sigma", "rot_sigma", "tr_score", "rot_score")}
    loss, terms = TO.score_matching_loss(f1, f2, b.tags.cpu().long(), sysidx, noised, oracle_tables)
    if not two_heads:
        loss, terms = terms[0], [terms[0], torch.zeros((), dtype=dtype)]
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return {"loss": torch.stack([loss.detach(), terms[0].detach(), terms[1].detach()]), "out1": f1.detach(), "out2": f2.detach(),
            "grads": dict(zip(names, grads))}


GROUPS = ("force_block.", "force_block2.", "edge_degree_embedding.", "sphere_embedding.", "norm.", "energy_embedding.")


def group_of(name):
    if name.startswith("blocks."):
        return ".".join(name.split(".")[:2]) + "."
    for g in GROUPS:
        if name.startswith(g):
            return g
    return name


def grouped_ratio(got: dict, ref: dict):
    """{group: Frobenius ratio over all the group's parameters}."""
    num, den = {}, {}
    for k, r in ref.items():
        if r is None:
            continue
        g = group_of(k)
        num[g] = num.get(g, 0.0) + float((got[k].double().cpu() - r.double()).pow(2).sum())
        den[g] = den.get(g, 0.0) + float(r.double().pow(2).sum())
    return {g: math.sqrt(num[g] / max(den[g], 1e-300)) for g in num}


ZERO_GRADIENT_SUFFIXES = ("so2_conv_2.so2_m_conv.1.fc.weight", "proj.bias")


def identically_zero(name):
    """Parameters of the force blocks whose float64 gradient is identically zero: the m = 2 map of the second convolution
    (an l = 1 output has no |m| = 2 coefficient) and the l = 0 bias of the projection."""
    return name.startswith("force_block") and name.endswith(ZERO_GRADIENT_SUFFIXES)


def check_step(label, grads, loss, outs, ref64, ref32, model):
    """The bounds of the issue on one whole step; prints every figure before it asserts.  ``grads``: {name: tensor | None}."""
    rel = lambda a, b: float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-300))
    two = bool(model.so3_denoising)
    lo = float(abs(loss[0].double().cpu() - ref64["loss"][0]) / abs(ref64["loss"][0]))
    terms = [float(abs(loss[i].double().cpu() - ref64["loss"][i]) / abs(ref64["loss"][i])) for i in ((1, 2) if two else (1,))]
    o1 = frob(outs[0], ref64["out1"])
    o2 = frob(outs[1], ref64["out2"]) if two else 0.0
    print(f"{label}: loss {lo:.2e} terms {max(terms):.2e} out1 {o1:.2e} out2 {o2:.2e}")
    assert lo < 1e-5 and max(terms) < 1e-5 and o1 < 1e-5 and o2 < 1e-5, (label, lo, terms, o1, o2)
    unused = [k for k, r in ref64["grads"].items() if r is None]
    for k in unused:
        assert grads[k] is None, (label, k, "has a gradient but no path to the loss")
    assert any(k.startswith("energy_block.") for k in unused)
    live = {k: r for k, r in ref64["grads"].items() if r is not None}
    for k in live:
        assert grads[k] is not None, (label, k, "missing")
    gr = grouped_ratio(grads, live)
    gr32 = grouped_ratio(ref32["grads"], live)
    for g_, e in sorted(gr.items()):
        print(f"{label}:   group {g_:<28s} {e:.2e}   (float32 oracle {gr32[g_]:.2e})")
    for g_, e in gr.items():
        assert e < REL_TOL, (label, g_, e)
    block_max = {}
    for k, r in live.items():
        block_max[group_of(k)] = max(block_max.get(group_of(k), 0.0), float(r.double().norm()))
    worst = (0.0, "")
    for k, r in live.items():
        got = grads[k].double().cpu()
        if identically_zero(k):
            assert float(r.abs().max()) == 0.0, (label, k, "the float64 gradient is not identically zero")
            nz = float(got.norm())
            print(f"{label}:   {k}: {'zero tensor' if nz == 0.0 else f'norm {nz:.2e} of block max {block_max[group_of(k)]:.2e}'}")
            assert nz == 0.0 or nz < 1e-4 * block_max[group_of(k)], (label, k, nz)
            continue
        d32 = frob(ref32["grads"][k], r)
        bound = max(REL_TOL, TIGHT_FACTOR * d32)
        e = frob(got, r)
        worst = max(worst, (e, k))
        if e > 0.3 * bound:
            print(f"{label}:   {k}: {e:.2e}  float32 oracle {d32:.2e}  bound {bound:.2e}")
        assert e < bound, (label, k, e, d32, bound)
    print(f"{label}: worst parameter {worst[0]:.2e} ({worst[1]})")


# ------------------------------------------------------------------------------------------------ operator pieces
def wigner_rows_to_D(wig, L, M, dtype=torch.float64):
    """[E, S_r (degree-major), S] from the device's kept Wigner rows [E, DR]."""
    E = wig.shape[0]
    S = (L + 1) ** 2
    rows, off = [], 0
    for l in range(L + 1):
        ml, n = min(l, M), 2 * l + 1
        blk = wig[:, off:off + (2 * ml + 1) * n].reshape(E, 2 * ml + 1, n).to(dtype)
        full = torch.zeros(E, 2 * ml + 1, S, dtype=dtype)
        full[:, :, l * l:(l + 1) ** 2] = blk
        rows.append(full)
        off += (2 * ml + 1) * n
    assert off == wig.shape[1]
    return torch.cat(rows, 1)


def radial_rows(L, M):
    """Row of the radial weights [RW, c] that the k-th ORDER-MAJOR coefficient is multiplied with."""
    out = list(range(L + 1))
    off = L + 1
    for m in range(1, M + 1):
        nm = L - m + 1
        out += list(range(off, off + nm)) * 2
        off += nm
    return torch.tensor(out)
