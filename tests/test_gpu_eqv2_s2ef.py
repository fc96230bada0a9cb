"""GPU tests of the EquiformerV2 S2EF force field (adsorbdiff_amd.equiformer_v2_oc20; adf_eqv2_set_weights_s2ef /
adf_eqv2_set_energy_head / adf_eqv2_forward_energy) against the reference model's recordings
(tools/make_golden_eqv2_s2ef.py), the CPU oracle and plain torch, and of relaxations driven by it."""
import ctypes as C

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as _lib
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc
from adsorbdiff_amd.ml_relaxation import ml_relax
from adsorbdiff_amd.trainer import ForcesTrainer
from tests.helpers import batch_from_fixture, load_npz, rel_err, row_rel_err
from tests.helpers_s2ef import RELAX_KW, SMALL_KW, full_model, s2ef_fixture, small_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 1e-4   # the project's parity budget (BASELINE.json north star)


def case(fx, tag):
    return {k[len(tag) + 1:]: v for k, v in fx.items() if k.startswith(tag + "_")}


def oracle_hp(m):
    return dict(lmax=m.lmax_list[0], mmax=m.mmax_list[0], num_layers=m.num_layers, sphere_channels=m.sphere_channels,
                attn_hidden_channels=m.attn_hidden_channels, num_heads=m.num_heads,
                attn_alpha_channels=m.attn_alpha_channels, attn_value_channels=m.attn_value_channels,
                ffn_hidden_channels=m.ffn_hidden_channels, grid_resolution=m.grid_resolution, max_radius=m.max_radius,
                max_neighbors=m.max_neighbors)


def check_outputs(energy, forces, cx, ref_energy_key="energy"):
    e_err = row_rel_err(energy.cpu().reshape(-1, 1), torch.from_numpy(cx[ref_energy_key]).reshape(-1, 1))
    f_err = rel_err(forces.cpu(), cx["forces"])
    atom = float(np.abs(forces.cpu().numpy() - cx["forces"]).max() / np.linalg.norm(cx["forces"], axis=1).max())
    print(f"energy row rel err {e_err:.2e}, forces rel err {f_err:.2e}, worst atom / largest row {atom:.2e}")
    assert e_err < REL_TOL and f_err < REL_TOL and atom < REL_TOL


@pytest.mark.parametrize("exact", [False, True])
def test_s2ef_small_model_vs_reference_fixture(exact):
    """Energies, forces and the node embeddings after the edge-degree embedding and after every block against the
    reference model's own recordings, on its edge list, in f16x3 and exact-f32 arithmetic.  A forward that ignored the
    distance basis (the denoiser's tabulated radial functions) is 126 % off on the forces."""
    cx = case(s2ef_fixture(), "small")
    m = small_model().to(DEV)
    b = batch_from_fixture(cx, device=DEV)
    eng = m.engine()
    eng.set_arithmetic(exact)
    eng.set_edges(torch.from_numpy(cx["edge_index"]), torch.from_numpy(cx["edge_vec"]))
    energy, forces, xb = eng.forward_energy(b, return_blocks=True)
    check_outputs(energy, forces, cx)
    L = m.lmax_list[0]
    for k in range(xb.shape[0]):
        for l in range(L + 1):
            got, ref = xb[k, :, l * l:(l + 1) ** 2].cpu(), torch.from_numpy(cx["x_blocks"][k, :, l * l:(l + 1) ** 2])
            assert rel_err(got, ref) < REL_TOL, (k, l, rel_err(got, ref))
    m.use_energy_lin_ref = True
    eng.bind_weights()
    e2, f2 = eng.forward_energy(b)
    check_outputs(e2, f2, cx, "energy_lin_ref")
    assert torch.equal(f2, forces)


@pytest.mark.parametrize("exact", [False, True])
def test_s2ef_full_width_vs_reference_fixture(exact):
    """The shipped width (config 4 without FOR_denoising, L = 4) on 2 x 40 atoms: energies, forces, strided block samples
    and per-degree norms over all atoms."""
    fx = s2ef_fixture()
    cx = case(fx, "full")
    m = full_model().to(DEV)
    b = batch_from_fixture(cx, device=DEV)
    eng = m.engine()
    eng.set_arithmetic(exact)
    eng.set_edges(torch.from_numpy(cx["edge_index"]), torch.from_numpy(cx["edge_vec"]))
    energy, forces, xb = eng.forward_energy(b, return_blocks=True)
    check_outputs(energy, forces, cx)
    sa, sc = int(fx["atom_stride"]), int(fx["channel_stride"])
    xb = xb.float().cpu()
    ref, got = torch.from_numpy(cx["x_blocks_sample"]), xb[:, ::sa, :, ::sc]
    assert got.shape == ref.shape
    for k in range(ref.shape[0]):
        for l in range(m.lmax_list[0] + 1):
            e = rel_err(got[k, :, l * l:(l + 1) ** 2], ref[k, :, l * l:(l + 1) ** 2])
            assert e < REL_TOL, (k, l, e)
            n, want = float(xb[k, :, l * l:(l + 1) ** 2].double().norm()), float(cx["x_blocks_degree_norms"][k, l])
            assert abs(n - want) < REL_TOL * want, (k, l)


def no_truncation_batch():
    from adsorbdiff_amd.synthetic import make_batch

    return make_batch(2, n_slab=36, n_ads=4, seed=71)


def test_s2ef_own_graph_vs_oracle():
    """The device-built graph and the live radial kernel together: cutoff 5.0, K = 64 (no neighbour list is truncated, so
    no tie at the K-th place can differ) against the oracle with zero radii on the oracle's own graph.  The oracle has
    one code path for both force blocks: force_block2 is aliased to force_block."""
    from oracle import eqv2_oracle as Q

    m = small_model(RELAX_KW)
    b = no_truncation_batch()
    ei, sh, nb = Q.radius_graph_pbc(b.pos, b.cell, b.natoms, 5.0, 64)
    assert int(torch.bincount(ei[1]).max()) < 64
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sd.update({k.replace("force_block.", "force_block2."): v for k, v in sd.items() if k.startswith("force_block.")})
    with torch.no_grad():
        r1, r2 = Q.eqv2_forward(sd, oracle_hp(m), b.pos, b.atomic_numbers, b.cell, b.natoms, atom_radii=torch.zeros(101))
        z1, _ = Q.eqv2_forward(sd, oracle_hp(m), b.pos, b.atomic_numbers, b.cell, b.natoms)
    assert torch.equal(r1, r2) and rel_err(z1, r1) > 1e-2, "the distance basis does not reach this model's forces"
    out = m.to(DEV)(b.to(DEV))
    e = rel_err(out["forces"].cpu(), r1)
    print(f"own graph: forces rel err {e:.2e} (basis ignored: {rel_err(z1, r1):.2e})")
    assert e < REL_TOL
    assert float((out["forces"].cpu() - r1).abs().max()) < REL_TOL * float(r1.norm(dim=1).max())


@pytest.mark.parametrize("which", [0, 1, 3])
def test_radial_first_layer_vs_torch(which):
    """The fused first radial layer (pair table + Gaussian window + LayerNorm + SiLU) against a plain torch evaluation of
    net.0 + net.1 + SiLU on the same edges: random distances plus an edge at d = max_radius, one at the 0.01 A floor of
    the graph, one just inside each end of the basis, and the element pair of the table's last row."""
    m = small_model()
    with torch.no_grad():   # norm gains / shifts away from (1, 0); let the basis part of the layer matter
        for n, p in m.named_parameters():
            if n.endswith("rad_func.net.0.weight"):
                p[:, :600].mul_(3.0)
            if n.endswith(("rad_func.net.1.weight", "rad_func.net.1.bias")):
                p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))))
    mod = (m.edge_degree_embedding, m.blocks[0].ga, m.blocks[1].ga, m.force_block)[which]
    rad = mod.rad_func if which == 0 else mod.so2_conv_1.rad_func
    NE, rc = m.max_num_elements, m.max_radius
    g = torch.Generator().manual_seed(7 + which)
    E = 1000
    d = torch.rand(E, generator=g) * rc
    d[:6] = torch.tensor([rc, 0.01, 0.0101, rc - 1e-4, 0.5 * rc, rc * 0.999])
    zs, zt = torch.randint(0, NE, (E,), generator=g), torch.randint(0, NE, (E,), generator=g)
    zs[:3], zt[:3] = NE - 1, NE - 1          # the table's last row
    zs[3], zt[3], zs[4], zt[4] = 0, 0, NE - 1, 0
    dirs = torch.nn.functional.normalize(torch.randn(E, 3, generator=g), dim=1)
    vec = dirs * d[:, None]
    dist = vec.norm(dim=1)
    offs = torch.linspace(0.0, rc, 600)
    coeff = -0.5 / (2.0 * (offs[1] - offs[0]).item()) ** 2
    with torch.no_grad():
        basis = torch.exp(coeff * (dist[:, None].double() - offs[None, :].double()) ** 2)
        x = torch.cat([basis, mod.source_embedding.weight[zs].double(), mod.target_embedding.weight[zt].double()], dim=1)
        y = x @ rad.net[0].weight.double().T + rad.net[0].bias.double()
        y = torch.nn.functional.layer_norm(y, (y.shape[1],), rad.net[1].weight.double(), rad.net[1].bias.double(), 1e-5)
        want = torch.nn.functional.silu(y).float()
    m = m.to(DEV)
    eng = m.engine()
    Z = torch.cat([zs, zt]).to(DEV, torch.int32)                     # "atoms": edge e goes from atom e to atom E + e
    src = torch.arange(E, dtype=torch.int32, device=DEV)
    dst = src + E
    out = torch.empty(E, m.edge_channels, dtype=torch.float32, device=DEV)
    v = vec.to(DEV).contiguous()
    _lib.check(eng.lib.adf_eqv2_radial_first_layer(eng.handle, which, E, src.data_ptr(), dst.data_ptr(), v.data_ptr(),
                                                   Z.data_ptr(), out.data_ptr(), eng._stream()))
    eng.check_flags()
    err = row_rel_err(out.cpu(), want)
    print(f"radial function {which}: worst row rel err {err:.2e}")
    # fp32 evaluation of a 32-channel LayerNorm row against float64: a few 1e-6; the parity budget bounds it
    assert err < REL_TOL
    assert eng.lib.adf_eqv2_radial_first_layer(eng.handle, 7, E, src.data_ptr(), dst.data_ptr(), v.data_ptr(), Z.data_ptr(),
                                               out.data_ptr(), eng._stream()) == _lib.ADF_EINVAL


def test_energy_is_bit_identical_alone_and_in_a_batch_and_without_the_force_block():
    from adsorbdiff_amd.synthetic import make_batch

    b3 = make_batch(3, n_slab=36, n_ads=4, seed=17)
    m = small_model().to(DEV)
    out = m(b3.clone().to(DEV))
    again = m(b3.clone().to(DEV))
    assert torch.equal(out["energy"], again["energy"]) and torch.equal(out["forces"], again["forces"])
    for s, data in enumerate(b3.to_data_list()):
        one = m(Batch.from_data_list([data]).to(DEV))
        a0 = int(b3.natoms[:s].sum())
        assert torch.equal(one["energy"], out["energy"][s:s + 1]), s
        assert torch.equal(one["forces"], out["forces"][a0:a0 + int(b3.natoms[s])]), s
    # the energy-only model (no force block evaluated) gives the full model's energy bit for bit
    eo = small_model(regress_forces=False)
    eo.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("force_block.")})
    got = eo.to(DEV)(b3.clone().to(DEV))
    assert set(got) == {"energy"} and torch.equal(got["energy"], out["energy"])


def test_energy_lin_ref_adds_exactly_the_reference_sum():
    from adsorbdiff_amd.synthetic import make_batch

    b = make_batch(3, n_slab=36, n_ads=4, seed=19)
    m = small_model().to(DEV)
    off = m(b.clone().to(DEV))["energy"].cpu()
    m.use_energy_lin_ref = True
    m.engine().bind_weights()
    on = m(b.clone().to(DEV))["energy"].cpu()
    # equiformer_v2_oc20.py:544-548: index_add of energy_lin_ref[Z] onto the energies, atom by atom, in fp32
    want = off.clone().index_add(0, b.batch, m.energy_lin_ref.detach().cpu()[b.atomic_numbers.long()])
    seq = off.clone()
    lin = m.energy_lin_ref.detach().cpu()
    for i in range(b.pos.shape[0]):
        seq[b.batch[i]] = seq[b.batch[i]] + lin[int(b.atomic_numbers[i])]
    assert torch.equal(want, seq), "index_add on the host is not the sequential fp32 sum"
    assert torch.equal(on, seq) and not torch.equal(on, off)


def test_atomic_number_outside_the_table_raises_and_the_next_forward_is_clean():
    from adsorbdiff_amd.synthetic import make_batch

    m = small_model().to(DEV)
    b = make_batch(1, n_slab=36, n_ads=4, seed=5)
    good = m(b.clone().to(DEV))
    for z in (m.max_num_elements, 200, -1):
        bad = b.clone()
        bad.atomic_numbers = bad.atomic_numbers.clone()
        bad.atomic_numbers[3] = z
        with pytest.raises(ValueError, match="atomic number"):
            m(bad.to(DEV))
    # elements without a tabulated radius (NaN in the denoiser) are ordinary elements here
    kr = b.clone()
    kr.atomic_numbers = kr.atomic_numbers.clone()
    kr.atomic_numbers[3] = 36
    assert bool(torch.isfinite(m(kr.to(DEV))["forces"]).all())
    after = m(b.clone().to(DEV))
    assert torch.equal(after["energy"], good["energy"]) and torch.equal(after["forces"], good["forces"])


def test_s2ef_relaxation_vs_reference_and_reproducible():
    """Free-running reference relaxation of 4 systems (reference LBFGS.run through its TorchCalc) with the small model at
    cutoff 5.0 / K = 64 (no neighbour list of the run is ever truncated: asserted by the generator)."""
    fx = load_npz("relax_eqv2_run.npz")
    m = small_model(RELAX_KW)
    tr = ForcesTrainer(m, device=DEV)
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    opt = LBFGS(b, TorchCalc(tr), maxstep=0.04, memory=int(fx["memory"]), damping=1.0, alpha=70.0, device=DEV)
    out = opt.run(fmax=float(fx["fmax"]), steps=int(fx["steps"]))
    mf = torch.stack(opt.max_force_log).cpu()
    print("max forces per iteration", mf.tolist(), "reference", fx["max_force"].tolist())
    assert opt.iterations == int(fx["iterations"])
    assert torch.equal(mf.ge(float(fx["fmax"])), torch.from_numpy(fx["masks"]))
    assert float((out.pos.cpu() - torch.from_numpy(fx["pos_final"])).abs().max()) < 1e-4
    assert row_rel_err(out.y.cpu().reshape(-1, 1), torch.from_numpy(fx["y"]).reshape(-1, 1)) < REL_TOL
    assert rel_err(out.force.cpu(), fx["force"]) < REL_TOL
    # a second run and ml_relax on the same batch: the same bits
    b2 = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    out2 = LBFGS(b2, TorchCalc(tr), maxstep=0.04, memory=int(fx["memory"]), damping=1.0, alpha=70.0,
                 device=DEV).run(fmax=float(fx["fmax"]), steps=int(fx["steps"]))
    b3 = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    out3 = ml_relax(b3, tr, steps=int(fx["steps"]), fmax=float(fx["fmax"]), relax_opt={"memory": int(fx["memory"])},
                    save_full_traj=False, device=DEV)
    for o in (out2, out3):
        assert torch.equal(o.pos, out.pos) and torch.equal(o.y, out.y) and torch.equal(o.force, out.force)


def test_the_denoiser_is_untouched_by_an_s2ef_model_on_the_same_device():
    """One forward of the config-4 denoiser before and after an S2EF model has been built and run on the same device:
    identical bits (the two handles share no state)."""
    from tests.helpers import cfg4_model_and_fixture

    den, fx = cfg4_model_and_fixture()
    den = den.to(DEV)
    b = batch_from_fixture(fx, device=DEV)
    f1, f2 = den(b)
    f1, f2 = f1.clone(), f2.clone()
    s = small_model().to(DEV)
    out = s(batch_from_fixture(case(s2ef_fixture(), "small"), device=DEV))
    assert bool(torch.isfinite(out["energy"]).all())
    g1, g2 = den(b)
    assert torch.equal(f1, g1) and torch.equal(f2, g2)
    with pytest.raises(RuntimeError, match="forward_energy"):
        den.engine().forward_energy(b)
    with pytest.raises(RuntimeError, match="forward_energy"):
        s.engine().forward(b)


def test_c_abi_argument_checks():
    m = small_model().to(DEV)
    eng = m.engine()
    lib, h = eng.lib, eng.handle
    w = torch.zeros(4, device=DEV)
    ptrs = (C.c_void_p * 4)(*[w.data_ptr()] * 4)
    assert lib.adf_eqv2_set_energy_head(h, 3, ptrs, 77.8, None, None) == _lib.ADF_EINVAL
    assert lib.adf_eqv2_set_energy_head(h, 4, ptrs, 0.0, None, None) == _lib.ADF_EINVAL
    assert lib.adf_eqv2_set_energy_head(None, 4, ptrs, 77.8, None, None) == _lib.ADF_EINVAL
    assert lib.adf_eqv2_set_weights_s2ef(h, 5, ptrs, None) == _lib.ADF_EINVAL
    eng.bind_weights()
    assert bool(torch.isfinite(m(batch_from_fixture(case(s2ef_fixture(), "small"), device=DEV))["energy"]).all())
