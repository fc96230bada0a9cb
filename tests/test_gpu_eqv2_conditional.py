"""GPU tests of the conditional EquiformerV2 denoiser (energy_encoding "scalar", configs/denoising/eqv2_conditional.yml):
the energy term on the l = 0 row of the node embedding, built by the library in fp16 from the per-system energies
(adf_eqv2_set_energy_embedding / adf_eqv2_set_system_energy).

Parity target: the fp32 reference model with only `energy_embedding` in fp16 (tests/golden/eqv2_conditional_l4.npz,
written by tools/make_golden_eqv2_conditional.py on the reference's CPU code, e3nn stand-in).  Tolerances: outputs 1e-4
relative (BASELINE.json north_star), the l = 0 rows after the embedding 1e-6 relative."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as _lib
from adsorbdiff_amd.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos as M
from tests.helpers import CFG4_KW, batch_from_fixture, load_npz, refill_parameters_by_name, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 1e-4
ROW_TOL = 1e-6
ENERGIES = (-1.73, 2.41, 0.37, -0.58, 1.12, -2.9, 3.3, 0.05)


def yaml_model_and_fixture(sampling):
    """The mirror class at the shipped conditional shape with the fixture's weights (rebuilt from parameter names;
    the energy layer's fp32 values are stored)."""
    fx = load_npz("eqv2_conditional_l4.npz")
    torch.manual_seed(0)
    m = refill_parameters_by_name(M(None, None, None, energy_encoding="scalar", sampling=sampling,
                                    **dict(CFG4_KW, lmax_list=[4])).eval(), float(fx["emb_scale"]))
    with torch.no_grad():
        m.energy_embedding.weight.copy_(torch.from_numpy(fx["ee_weight"]))
        m.energy_embedding.bias.copy_(torch.from_numpy(fx["ee_bias"]))
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    return m, fx


def small_model(conditional=True, sampling=False, layers=2, C_=32, seed=0):
    torch.manual_seed(seed)
    m = M(None, None, None, max_neighbors=20, max_radius=12.0, max_num_elements=90, num_layers=layers,
          sphere_channels=C_, attn_hidden_channels=32, num_heads=2, attn_alpha_channels=16, attn_value_channels=16,
          ffn_hidden_channels=32, norm_type="layer_norm_sh", lmax_list=[4], mmax_list=[2], grid_resolution=18,
          edge_channels=32, attn_activation="silu", ffn_activation="silu", use_grid_mlp=True, use_sep_s2_act=True,
          alpha_drop=0.0, drop_path_rate=0.0, weight_init="uniform", FOR_denoising=True,
          energy_encoding="scalar" if conditional else None, sampling=sampling)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("source_embedding.weight") or n.endswith("target_embedding.weight"):
                p.mul_(300.0)   # trained-like edge embeddings
        if conditional:
            g = torch.Generator().manual_seed(seed + 11)
            m.energy_embedding.weight.copy_(torch.randn(C_, 1, generator=g))
            m.energy_embedding.bias.copy_(torch.randn(C_, generator=g))
    m.so3_denoising = True
    return m.eval()


def safe_batch(n_sys, n_slab, seed, energies=True):
    from adsorbdiff_amd.synthetic import make_batch

    b = make_batch(n_sys, n_slab=n_slab, n_ads=4, seed=seed)
    z = b.atomic_numbers.clone()
    z[(z == 36) | (z == 54)] = 47.0  # elements without a tabulated radius give NaN in the reference
    b.atomic_numbers = z
    if energies:
        b.energy = torch.tensor(ENERGIES[:n_sys], dtype=torch.float32)
    return b


def fresh_engine(m):
    if m._engine is not None:
        m._engine.close()
    m._engine = None
    return m.engine()


@pytest.mark.parametrize("case", ["samp", "cond"])
@pytest.mark.parametrize("exact", [False, True])
def test_conditional_forward_vs_reference_fixture(exact, case):
    """Both arithmetics, sampling mode and per-system energies, on the reference's edge list: (f1, f2) at 1e-4, the l = 0
    rows after the energy and edge-degree embeddings at 1e-6, every block per degree at 1e-4.  The fixture tells the
    fp16 term from an fp32 one: the rows with the fp32 term miss it by more than ten times the row tolerance."""
    m, fx = yaml_model_and_fixture(sampling=(case == "samp"))
    m = m.to(DEV)
    b = batch_from_fixture(fx, device=DEV)
    b.energy = torch.from_numpy(fx["energy"]).to(DEV)   # read only when sampling=False
    eng = m.engine()
    eng.set_arithmetic(exact)
    eng.set_edges(torch.from_numpy(fx["edge_index"]), torch.from_numpy(fx["edge_vec"]))
    f1, f2, xb = eng.forward(b, return_blocks=True)
    e1, e2 = rel_err(f1.cpu(), fx[f"{case}_f1"]), rel_err(f2.cpu(), fx[f"{case}_f2"])
    rows = xb[0, :, 0, :].cpu()
    er = rel_err(rows, fx[f"{case}_x_l0"])
    print(f"conditional L=4 {case} {'exact f32' if exact else 'f16x3'}: f1 {e1:.2e} f2 {e2:.2e} l=0 rows {er:.2e}")
    assert e1 < REL_TOL and e2 < REL_TOL
    assert er < ROW_TOL
    # the fp16 term matters at this tolerance
    bidx = torch.from_numpy(fx["batch"]).long()
    y = torch.zeros(2, dtype=torch.float64) if case == "samp" else torch.from_numpy(fx["energy"]).double()
    t32 = y[:, None] * torch.from_numpy(fx["ee_weight"]).double().reshape(1, -1) + torch.from_numpy(fx["ee_bias"]).double()
    t16 = torch.from_numpy(fx[f"{case}_term"]).double()
    rows32 = torch.from_numpy(fx[f"{case}_x_l0"]).double() - t16[bidx] + t32[bidx]
    assert rel_err(rows32, fx[f"{case}_x_l0"]) > 10 * ROW_TOL
    assert rel_err(rows, rows32) > 10 * ROW_TOL
    # blocks: strided sample per degree, per-degree norms over all atoms
    sa, sc = int(fx["atom_stride"]), int(fx["channel_stride"])
    ref = torch.from_numpy(fx[f"{case}_x_blocks_sample"])
    got = xb.cpu()[:, ::sa, :, ::sc]
    assert got.shape == ref.shape
    for k in range(ref.shape[0]):
        for l in range(5):
            sl = slice(l * l, (l + 1) ** 2)
            assert rel_err(got[k, :, sl], ref[k, :, sl]) < REL_TOL, (k, l)
            n = float(xb[k, :, sl].double().norm())
            want = float(fx[f"{case}_x_blocks_degree_norms"][k, l])
            assert abs(n - want) < REL_TOL * want, (k, l)
    for got_, ref_ in ((f1.cpu().numpy(), fx[f"{case}_f1"]), (f2.cpu().numpy(), fx[f"{case}_f2"])):
        assert np.abs(got_ - ref_).max() < REL_TOL * np.linalg.norm(ref_, axis=1).max()


def test_zero_energy_layer_is_bit_identical_to_the_unconditional_model():
    cond = small_model(conditional=True)
    with torch.no_grad():
        cond.energy_embedding.weight.zero_()
        cond.energy_embedding.bias.zero_()
    plain = small_model(conditional=False)
    sd = {k: v for k, v in cond.state_dict().items() if not k.startswith("energy_embedding")}
    plain.load_state_dict(sd)
    b = safe_batch(2, 196, seed=31).to(DEV)
    f1, f2, xa = cond.to(DEV).engine().forward(b, return_blocks=True)
    g1, g2, xb = plain.to(DEV).engine().forward(b, return_blocks=True)
    assert torch.equal(xa, xb)
    assert torch.equal(f1, g1) and torch.equal(f2, g2)


def _run_sampler(m, b, placement, **extra):
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    params = dict(num_steps=4, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False)
    kw = {k: extra.pop(k) for k in ("traj_dir", "traj_names", "save_full_traj") if k in extra}
    den = Denoiser(b.clone().to(DEV), DiffTorchCalc(DenoisingTrainer(m, device=DEV)),
                   dict(params, placement_noise=placement, **extra), device=DEV, **kw)
    out = den.run()
    assert den.steps_applied == 4
    return out.pos.cpu()


def test_conditional_sampler_sites_are_identical_across_loop_forms(tmp_path):
    """Non-zero energies: adsorbate-only and full outputs, incremental blocks on and off, the per-step loop and the
    trajectory sink all end at the same sites; other energies end elsewhere."""
    m = small_model(conditional=True).to(DEV)
    placement = torch.rand(2, 3, generator=torch.Generator().manual_seed(4))
    b = safe_batch(2, 196, seed=23)
    outs = {}
    for ads_only in (False, True):
        for inc in (False, True):
            outs[(ads_only, inc)] = _run_sampler(m, b, placement, scores_on_adsorbate_only=ads_only,
                                                 incremental_layers=inc)
    c = m.engine().counters()
    assert 0 < int(c.inc_rows) < int(c.inc_rows_full)
    outs["per_step"] = _run_sampler(m, b, placement, step_hook=lambda t: None)
    outs["traj"] = _run_sampler(m, b, placement, traj_dir=tmp_path, traj_names=[str(s) for s in b.sid],
                                save_full_traj=True)
    ref = outs[(False, False)]
    for k, v in outs.items():
        assert torch.equal(v, ref), k
    n0 = int(b.natoms[0])
    z = np.load(tmp_path / f"{b.sid[0]}.npz")
    assert np.array_equal(z["positions"][-1], ref[:n0].numpy())
    other = b.clone()
    other.energy = b.energy + 1.5
    assert not torch.equal(_run_sampler(m, other, placement), ref)
    assert float((ref - b.pos).abs().max()) > 0.1  # the adsorbates did move


def test_energy_change_under_static_atom_promise_equals_a_fresh_engine():
    """Incremental blocks keep rows across forwards; new energies (or new energy weights) must not leave any of them
    stale: every block and both outputs equal a fresh engine's, bit for bit."""
    m = small_model(conditional=True, layers=3).to(DEV)
    b = safe_batch(2, 196, seed=31).to(DEV)
    N = int(b.pos.shape[0])
    ads = b.tags == 2
    pos0 = b.pos.float().contiguous()
    pos1 = pos0.clone()
    pos1[ads] += (0.2 * torch.randn(int(ads.sum()), 3, generator=torch.Generator().manual_seed(2))).to(DEV)
    e1 = b.energy.clone()
    e2 = torch.tensor([0.91, -3.07], device=DEV)

    def run(eng, prep, pos):
        f1, f2 = torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV)
        xb = torch.empty(4, N, 25, 32, device=DEV)
        eng.forward_prepared(prep, pos, f1, f2, x_blocks=xb)
        eng.check_flags()
        return f1, f2, xb

    def fresh(pos, energy):
        eng = fresh_engine(m)
        prep = eng.prepare(b)
        eng.set_system_energy(energy)
        return run(eng, prep, pos)

    want = fresh(pos1, e2)
    eng = fresh_engine(m)
    prep = eng.prepare(b)
    eng.set_moving_atoms(prep, ads)
    eng.set_incremental(True)
    eng.set_system_energy(e1)
    run(eng, prep, pos0)
    run(eng, prep, pos1)
    eng.set_system_energy(e2)
    got = run(eng, prep, pos1)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # the energy weights change: the engine rebinds them (weights version) and the kept rows are dropped
    run(eng, prep, pos0)
    with torch.no_grad():
        m.energy_embedding.bias.mul_(-0.5)
    eng = m.engine()
    got = run(eng, prep, pos1)
    eng.set_moving_atoms(None, None)
    want = fresh(pos1, e2)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_sharded_sampling_with_per_system_energies_equals_the_single_run():
    from adsorbdiff_amd.sampler import shard_batch

    m = small_model(conditional=True, layers=1).to(DEV)
    b = safe_batch(8, 36, seed=41)
    placement = torch.rand(8, 3, generator=torch.Generator().manual_seed(8))
    whole = _run_sampler(m, b, placement)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(b.natoms, 0)])
    seen = []
    for r in range(8):
        sub, ids = shard_batch(b, r, 8)
        assert sub is not None and torch.equal(sub.energy, b.energy[ids])
        part = _run_sampler(m, sub, placement[ids])
        rows = torch.cat([torch.arange(int(off[i]), int(off[i + 1])) for i in ids])
        assert torch.equal(part, whole[rows]), r
        seen += ids
    assert sorted(seen) == list(range(8))


def test_missing_energy_and_bad_arguments_raise():
    m = small_model(conditional=True).to(DEV)
    host = safe_batch(2, 36, seed=5, energies=False)
    b = host.clone().to(DEV)
    with pytest.raises(ValueError, match="data.energy"):
        m(b)
    with pytest.raises(ValueError, match="data.energy"):
        _run_sampler(m, host, torch.rand(2, 3))
    m.sampling = True
    f1, _ = m(b)   # sampling mode reads no energy
    assert bool(torch.isfinite(f1).all())
    m.sampling = False
    eng = m.engine()
    lib, h = eng.lib, eng.handle
    w = torch.zeros(32, device=DEV)
    assert lib.adf_eqv2_set_energy_embedding(h, w.data_ptr(), None, None) == _lib.ADF_EINVAL
    assert lib.adf_eqv2_set_energy_embedding(h, None, w.data_ptr(), None) == _lib.ADF_EINVAL
    assert lib.adf_eqv2_set_system_energy(h, w.data_ptr(), 0, None) == _lib.ADF_EINVAL
    assert lib.adf_eqv2_set_energy_embedding(None, None, None, None) == _lib.ADF_EINVAL
    eng.bind_weights()
    # energies for 3 systems, a 2-system batch
    eng.set_system_energy(torch.tensor([1.0, 2.0, 3.0], device=DEV))
    prep = eng.prepare(b)
    f1, f2 = torch.empty(int(b.pos.shape[0]), 3, device=DEV), torch.empty(int(b.pos.shape[0]), 3, device=DEV)
    with pytest.raises(ValueError, match="systems"):
        eng.forward_prepared(prep, b.pos.float().contiguous(), f1, f2)
    b.energy = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    with pytest.raises(ValueError, match="3 values for 2 systems"):
        m(b)
    b.energy = torch.tensor([0.5, -0.5], device=DEV)
    f1, _ = m(b)
    assert bool(torch.isfinite(f1).all())
