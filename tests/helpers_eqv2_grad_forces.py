"""The yardstick of the EquiformerV2 energy-gradient forces (tests/test_eqv2_grad_forces_host.py,
tests/test_gpu_eqv2_grad_forces.py): ``helpers_eqv2_s2ef_train.forward_s2ef``'s energy as a function of the POSITIONS, in
float64 (float32 for the calibration), differentiated by torch.autograd on the CPU.

``pos`` is a leaf; ``vec = pos[src] - pos[dst] + offset`` with the per-edge offset (the periodic image's shift) a constant
recovered from an exported graph; the Gaussian basis is ``live_basis`` of the norm of that vector in the working precision
(``forward_s2ef`` evaluates it from fp32 distances, which cuts the graph); ``D = wigner_from_rotation(edge_frames(vec))``.
``edge_frames`` picks its helper axis per edge - the coordinate axis least aligned with the edge - so this yardstick has no
pole anywhere.  The edge set is held fixed, which is what ``torch.autograd.grad(energy.sum(), pos)`` sees on the reference
model too.  Imports oracle/ modules and changes none."""
import torch

from oracle import eqv2_oracle as Q
from tests import helpers_eqv2_s2ef_train as S
from tests import helpers_eqv2_train as T


def energy_of_vec(sd, hp, Z, ei, vec, sysidx, num_systems):
    """energy [B] of EquiformerV2_OC20.forward in ``vec``'s dtype on the edge list ``ei`` [2, E] (source, target) with the
    edge vectors ``vec`` [E, 3] (differentiable).  The composition is ``forward_s2ef``'s, without its force block."""
    dtype = vec.dtype
    L, M, C = hp["lmax"], hp["mmax"], hp["sphere_channels"]
    Z = Z.long()
    N = Z.shape[0]
    src, dst = ei[0], ei[1]
    basis = S.live_basis(vec.norm(dim=1), hp["max_radius"], dtype)
    D = Q.wigner_from_rotation(L, Q.edge_frames(vec))
    grids, nS = Q.Grids(L, M, hp["grid_resolution"], dtype), (L + 1) ** 2
    x0 = sd["sphere_embedding.weight"][Z]
    pre = "edge_degree_embedding."
    scal = torch.cat([basis, sd[pre + "source_embedding.weight"][Z[src]], sd[pre + "target_embedding.weight"][Z[dst]]], dim=1)
    m0 = Q.radial_mlp(sd, pre + "rad_func.", scal).reshape(-1, L + 1, C)
    red = Q.lm_list(L, M)
    cols = torch.tensor([red.index((l, 0)) for l in range(L + 1)])
    rm = Q.reduced_mask(L, M)
    back = (D.transpose(1, 2)[:, :, rm] * Q.truncation_rescale(L, M, dtype)[None, None, :])[:, :, cols]
    deg = torch.zeros(N, nS, C, dtype=dtype).index_add(0, dst, torch.bmm(back, m0)) / hp["avg_degree"]
    x = torch.cat([deg[:, :1] + x0[:, None, :], deg[:, 1:]], dim=1)
    for i in range(hp["num_layers"]):
        p = f"blocks.{i}."
        x = x + T.attention_block_masked(sd, p + "ga.", Q.norm_sh(sd, p + "norm_1.", x, L), Z, basis, src, dst, D, hp, grids, None)
        x = x + Q.feed_forward(sd, p + "ffn.", Q.norm_sh(sd, p + "norm_2.", x, L), hp, grids)
    x = Q.norm_sh(sd, "norm.", x, L)
    e_atom = Q.feed_forward(sd, "energy_block.", x, hp, grids)[:, 0, 0]
    energy = torch.zeros(num_systems, dtype=dtype).index_add(0, sysidx, e_atom) / hp["avg_num_nodes"]
    if hp["use_energy_lin_ref"]:
        energy = energy.index_add(0, sysidx, sd["energy_lin_ref"].detach()[Z])
    return energy


def state(model, dtype):
    return {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}


def edge_offsets(pos, ei, vec):
    """The constant of every edge, vec - (pos[src] - pos[dst]), in float64 from the graph's fp32 values."""
    pos, vec = pos.detach().cpu().double(), vec.detach().cpu().double()
    return vec - (pos[ei[0]] - pos[ei[1]])


def energy_of_pos(model, Z, pos, ei, offset, sysidx, num_systems, dtype=torch.float64, hp=None):
    """energy [B] at the positions ``pos`` (any float tensor; differentiable when it requires grad) on the fixed edge set."""
    sd = state(model, dtype)
    pos = pos.to(dtype)
    vec = pos[ei[0]] - pos[ei[1]] + offset.to(dtype)
    return energy_of_vec(sd, hp or S.hp_of(model), Z.cpu(), ei, vec, sysidx.cpu().long(), num_systems)


def energy_and_forces(model, Z, pos, ei, offset, sysidx, num_systems, dtype=torch.float64):
    """(energy [B], forces [N, 3] = -dE/dpos) by autograd in ``dtype``."""
    leaf = pos.detach().cpu().to(dtype).clone().requires_grad_(True)
    e = energy_of_pos(model, Z, leaf, ei, offset, sysidx, num_systems, dtype)
    (g,) = torch.autograd.grad(e.sum(), leaf)
    return e.detach(), -g


def reference_on_graph(model, batch, graph, dtype=torch.float64):
    """``energy_and_forces`` of ``batch`` on an exported graph ``(eptr, src, dst, vec, wig)`` of the device."""
    _, src, dst, vec, _ = graph
    ei = torch.stack([src.cpu().long(), dst.cpu().long()])
    off = edge_offsets(batch.pos, ei, vec)
    return energy_and_forces(model, batch.atomic_numbers, batch.pos, ei, off, batch.batch, int(batch.natoms.numel()), dtype)


def pole_cluster():
    """8 atoms, one system, no periodic image: atom 1 sits exactly above atom 0 along +y (so the list holds one edge along
    +y and one along -y, the poles of the device's frame), the rest at generic places -> (Z [8], pos [8, 3] fp32,
    edge_index [2, E] sorted by target: every ordered pair closer than 4.5)."""
    pos = torch.tensor([[0.0, 0.0, 0.0], [0.0, 1.5, 0.0], [1.9, 0.4, -0.3], [-1.2, 1.1, 1.6], [0.7, -1.8, 1.1],
                        [-1.6, -0.9, -1.4], [2.1, 2.2, 1.3], [0.4, 2.9, -1.7]], dtype=torch.float32)
    Z = torch.tensor([29, 8, 29, 1, 6, 29, 8, 1])
    d = (pos[:, None, :] - pos[None, :, :]).norm(dim=2)
    dst, src = torch.nonzero((d < 4.5) & (d > 0), as_tuple=True)      # row-major: sorted by target
    return Z, pos, torch.stack([src, dst])


def rel_force_error(got, ref):
    """max |dF| / max |F|."""
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------- single operators
def transported_frames(vec0, vec):
    """A frame "second row = edge direction" for ``vec`` near ``vec0``: ``edge_frames(vec0)`` carried along by the
    shortest rotation n0 -> n, which has no component about the edge to first order.  At vec = vec0 it is
    ``edge_frames(vec0)``; its derivative there is the one of a frame that does not roll - the derivative
    ``adf_op_eq_wigner_bwd`` returns for any function of the Wigner rows, roll-invariant or not."""
    R0 = Q.edge_frames(vec0.detach())
    n0 = vec0.detach() / vec0.detach().norm(dim=1, keepdim=True)
    n = vec / vec.norm(dim=1, keepdim=True)
    v = torch.cross(n0, n, dim=1)
    c = (n0 * n).sum(1)
    K = torch.zeros(vec.shape[0], 3, 3, dtype=vec.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
    Qm = torch.eye(3, dtype=vec.dtype)[None] + K + torch.bmm(K, K) / (1.0 + c)[:, None, None]     # Qm n0 = n
    return torch.bmm(R0, Qm.transpose(1, 2))


def wigner_generators(L, dtype=torch.float64):
    """[(K_x, K_y, K_z)] per degree: D_l(exp(t [e_k])) = 1 + t K_k + ... in the basis of so3_math.j_matrices.  K_y = Z_l'(0)
    (l - i on the anti-diagonal), K_x = J K_y J, K_z = [K_x, K_y]."""
    from adsorbdiff_amd import so3_math

    out = []
    for l, J in enumerate(so3_math.j_matrices(L)):
        n = 2 * l + 1
        J = torch.from_numpy(J).double()
        ky = torch.zeros(n, n, dtype=torch.float64)
        ky[torch.arange(n), n - 1 - torch.arange(n)] = torch.arange(l, -l - 1, -1, dtype=torch.float64)
        kx = J @ ky @ J
        out.append(tuple(k.to(dtype) for k in (kx, ky, kx @ ky - ky @ kx)))
    return out


def wigner_bwd_torch(L, M, vec, wig, dwig, ddist, dtype):
    """``adf_op_eq_wigner_bwd``'s formula in torch, all operands cast to ``dtype``: dvec = ddist n + (n x tau) / |vec|,
    tau_k = sum_l <dwig_l, wig_l K_k^l>."""
    vec, wig, dwig, ddist = (t.to(dtype) for t in (vec, wig, dwig, ddist))
    tau = torch.zeros(vec.shape[0], 3, dtype=dtype)
    off = 0
    for l, Ks in enumerate(wigner_generators(L, dtype)):
        nr, n = 2 * min(l, M) + 1, 2 * l + 1
        W, Gm = (t[:, off:off + nr * n].reshape(-1, nr, n) for t in (wig, dwig))
        off += nr * n
        for k in range(3):
            tau[:, k] = tau[:, k] + (Gm * (W @ Ks[k])).sum((1, 2))
    d = vec.norm(dim=1, keepdim=True)
    n_ = vec / d
    return ddist[:, None] * n_ + torch.cross(n_, tau, dim=1) / d


def kept_rows(D, L, M):
    """[E, DR]: the rows |m| <= min(l, M) of every D_l of the block-diagonal D [E, S, S], in wig's layout."""
    out = []
    for l in range(L + 1):
        ml = min(l, M)
        out.append(D[:, l * l + l - ml:l * l + l + ml + 1, l * l:(l + 1) ** 2].reshape(D.shape[0], -1))
    return torch.cat(out, 1)


def hard_vectors(E, cutoff, seed=0):
    """[E, 3] fp32 edge vectors: +-y exactly, 1e-4 and 1e-7 off the pole, +-x, +-z, lengths 0.7 and cutoff - 1e-3 (the
    Gaussian window clipped at either end of the basis), then seeded generic directions with lengths in [0.7, cutoff)."""
    g = torch.Generator().manual_seed(seed)
    hard = torch.tensor([[0.0, 1.3, 0.0], [0.0, -2.1, 0.0], [1e-4, 1.0, 0.0], [0.0, -1.0, 1e-7], [1e-7, 1.0, 0.0],
                         [1.7, 0.0, 0.0], [-0.9, 0.0, 0.0], [0.0, 0.0, 2.2], [0.0, 0.0, -1.1], [0.7, 0.0, 0.0],
                         [0.0, cutoff - 1e-3, 0.0], [0.3, 0.4, 0.5]], dtype=torch.float64)
    hard[-1] *= 0.7 / hard[-1].norm()
    dirs = torch.randn(max(E, 1), 3, generator=g, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=1, keepdim=True) * (0.7 + (cutoff - 0.7 - 1e-3) * torch.rand(max(E, 1), 1, generator=g, dtype=torch.float64))
    if E == 1:
        return hard[:1].float()
    return torch.cat([hard, dirs])[:E].float()


# ---------------------------------------------------------------------------------------------------- whole-force cases
def cell4_batch():
    """4 atoms in a cell whose b axis is 2.5 long and exactly along y: every atom's nearest neighbours are its own images at
    (0, +-2.5, 0), edges that sit on the poles of the device's frame and have src == dst."""
    from adsorbdiff_amd.data import Batch

    b = Batch()
    b.pos = torch.tensor([[0.3, 0.2, 0.4], [3.1, 0.9, 0.7], [0.6, 1.4, 3.6], [3.4, 2.1, 3.3]], dtype=torch.float32)
    b.atomic_numbers = torch.tensor([29.0, 8.0, 29.0, 1.0])
    b.tags = torch.tensor([0, 1, 1, 2])
    b.fixed = torch.tensor([1, 0, 0, 0])
    b.cell = torch.tensor([[[5.9, 0.0, 0.0], [0.0, 2.5, 0.0], [0.0, 0.0, 6.3]]], dtype=torch.float32)
    b.natoms = torch.tensor([4])
    b.batch = torch.zeros(4, dtype=torch.long)
    b.sid = ["0"]
    return b


def cluster_batch():
    """``pole_cluster`` plus a ninth atom without any edge, as a batch for ``set_edges`` -> (batch, edge_index, edge_vec)."""
    from tests.helpers_eqv2_ragged import one_system_batch

    Z, pos, ei = pole_cluster()
    b = one_system_batch(torch.cat([Z, torch.tensor([47])]))
    b.pos = torch.cat([pos, torch.tensor([[20.0, 20.0, 20.0]])])
    return b, ei, (pos[ei[0]] - pos[ei[1]]).contiguous()


def brute_force_graph(b, cutoff, cap):
    """(edge_index, edge_vec) of a one-system periodic batch: every image pair closer than ``cutoff``, the ``cap`` nearest
    per target, sorted by target.  The CPU calibration of a case whose graph the device builds itself uses it."""
    pos, cell = b.pos.double(), b.cell[0].double()
    n = pos.shape[0]
    rng = range(-4, 5)
    shifts = torch.tensor([[i, j, k] for i in rng for j in rng for k in rng], dtype=torch.float64) @ cell
    src, dst, vec = [], [], []
    for t in range(n):
        v = (pos[None, :, :] + shifts[:, None, :] - pos[t]).reshape(-1, 3)
        s = torch.arange(n).repeat(shifts.shape[0])
        d = v.norm(dim=1)
        keep = (d < cutoff) & (d > 1e-9)
        order = torch.argsort(d[keep])[:cap]
        src.append(s[keep][order]); dst.append(torch.full((order.numel(),), t)); vec.append(v[keep][order])
    return torch.stack([torch.cat(src), torch.cat(dst)]), torch.cat(vec).float()
