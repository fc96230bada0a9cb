"""GPU parity tests: the HIP path (through the C ABI) against the committed golden fixtures
(generated from the real reference, oracle/make_golden.py) and against the CPU oracle on
seeded inputs.  Tolerances: integer graph outputs bit-exact; floating point 1e-4 relative
(BASELINE.json north_star), written next to each assertion."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS
from adsorbdiff_amd.synthetic import make_batch
from tests.helpers import (batch_from_fixture, canon_edges, load_npz, max_abs_err_rel_to_max, rel_err, row_rel_err,
                           state_dict_from_fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 1e-4  # north_star: "within 1e-4 rel"


def small_model(fx, device=DEV):
    H, L, R = int(fx["hp_hidden_channels"]), int(fx["hp_num_layers"]), int(fx["hp_num_rbf"])
    sf = {f"upd_out_scalar_scale_{i}": float(s) for i, s in enumerate(fx["scale_factors"])}
    m = PaiNN(None, 50, 1, hidden_channels=H, num_layers=L, num_rbf=R, cutoff=float(fx["hp_cutoff"]),
              max_neighbors=int(fx["hp_max_neighbors"]), scale_file=sf, so3_denoising=True)
    missing, unexpected = m.load_state_dict(state_dict_from_fixture(fx), strict=False)
    assert set(missing) <= {"atom_radii"} and not unexpected, (missing, unexpected)
    return m.to(device).eval()


def graph_model(cutoff, K):
    torch.manual_seed(0)
    return PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, cutoff=cutoff, max_neighbors=K,
                 so3_denoising=True).to(DEV).eval()


@pytest.mark.parametrize("name", ["small", "mixed", "bench1", "small12", "tie"])
def test_graph_vs_reference_fixture(name):
    fx = load_npz(f"graph_{name}.npz")
    b = batch_from_fixture(fx, device=DEV)
    m = graph_model(float(fx["cutoff"]), int(fx["K"]))
    eng = m.engine()
    E = eng.build_graph(b)
    cnt, src, sh, es, ed, dist, vec = [t.cpu().numpy() for t in eng.export_graph()]
    ei0, sh0 = fx["edge_index0"], fx["shifts0"].astype(np.int64)
    N = b.pos.shape[0]
    # directed top-K stage, in the reference's own edge order
    got_src = np.concatenate([src[i, : cnt[i]] for i in range(N)])
    got_dst = np.concatenate([np.full(cnt[i], i) for i in range(N)])
    got_sh = np.concatenate([sh[i, : cnt[i]] for i in range(N)])
    assert got_src.shape[0] == ei0.shape[1]
    assert np.array_equal(got_dst, ei0[1])
    if int(fx["exact"]):
        assert np.array_equal(got_src, ei0[0]), "top-K neighbour lists differ from the reference"
        assert np.array_equal(got_sh, sh0)
        # symmetrised stage: same edge multiset, same geometry
        assert E == fx["edge_index"].shape[1]
        a = canon_edges(es, ed, dist, vec)
        r = canon_edges(fx["edge_index"][0], fx["edge_index"][1], fx["dist"], fx["unit_vec"])
        assert np.array_equal(a[0], r[0]) and np.array_equal(a[1], r[1])
        np.testing.assert_allclose(a[2], r[2], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(a[3], r[3], rtol=0, atol=2e-6)
    else:
        # exact d^2 ties at the K-th place: the reference's unstable sort picks arbitrarily;
        # require the same per-centre distance multiset instead
        cell = torch.from_numpy(fx["cell"]).double()
        pos = torch.from_numpy(fx["pos"]).double()
        bidx = torch.from_numpy(fx["batch"])

        def d2(s_, d_, sh_):
            s_, d_ = torch.from_numpy(s_).long(), torch.from_numpy(d_).long()
            off = torch.einsum("ek,ekj->ej", torch.from_numpy(sh_).double(), cell[bidx[d_]])
            v = pos[s_] - pos[d_] + off
            return (v * v).sum(-1)

        dg, dr = d2(got_src, got_dst, got_sh), d2(ei0[0], ei0[1], sh0)
        for i in range(N):
            mk = got_dst == i
            np.testing.assert_allclose(np.sort(dg[mk].numpy()), np.sort(dr[mk].numpy()), rtol=1e-6)


def test_graph_empty_image_raises():
    b = make_batch(1, n_slab=16, n_ads=1, seed=3)
    b.pos = b.pos * 0 + torch.arange(b.pos.shape[0]).float()[:, None] * 40.0  # everything far apart
    b.cell = b.cell * 50
    m = graph_model(2.0, 10)
    with pytest.raises(ValueError):
        m(b.to(DEV))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(1000, 512, 512, 1), (777, 1536, 512, 0), (600, 1024, 512, 0), (300, 64, 128, 1),
                                   (4099, 512, 1024, 1)])
def test_linear_kernels_vs_fp64(mode, shape):
    """Both GEMM kernels (exact-f32 MFMA and the f16x3 split) against an fp64 torch reference."""
    import ctypes as C

    from adsorbdiff_amd import lib as L

    M, N, K, act = shape
    g = torch.Generator().manual_seed(M + N)
    A = (torch.randn(M, K, generator=g) * 1.5).to(DEV)
    A[:: 7] *= 1e-3  # rows of small activations (fp16 subnormal lo parts)
    W = ((torch.rand(N, K, generator=g) - 0.5) * 0.15).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    out = torch.empty(M, N, device=DEV)
    lib = L.load()
    L.check(lib.adf_linear_forward(A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, act, mode,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    ref = A.double() @ W.double().t() + b.double()
    if act:
        ref = torch.nn.functional.silu(ref) / 0.6
    # error relative to the magnitude of the dot products (sum |a||w|), the natural scale of a GEMM
    scale = (A.double().abs() @ W.double().abs().t()).mean()
    err = float((out.double() - ref).abs().max() / scale)
    assert err < (3e-6 if mode == 0 else 6e-6), err
    assert rel_err(out, ref) < (1e-6 if mode == 0 else 3e-6)


@pytest.mark.parametrize("scale,tol", [(1.0e6, 5e-6), (1.0e3, 5e-6), (1.0, 5e-6), (1.0e-2, 5e-6), (1.0e-4, 5e-6), (1.0e-8, 5e-6)])
def test_linear_f16x3_activation_range(scale, tol):
    """Row lifts of the f16x3 split (gemm16.hip, round 3): every A row is multiplied by its own power of two before the
    fp16 hi/lo split (its largest element lands in [2^14, 2^15)) and the lift is divided out in the epilogue, so a
    product keeps ~2^-22 relative precision whatever the magnitude of the activations — rounds 1-2 split them unscaled:
    an element below 0.125 lost its a_lo term to the matrix core's subnormal flush (4e-4 at scales 1e-2 and 1e-4) and
    one above 65504 overflowed.  The lift depends on the row alone (batch-independent bits)."""
    import ctypes as C

    from adsorbdiff_amd import lib as L

    lib = L.load()
    torch.manual_seed(3)
    M, N, K = 512, 256, 512
    A = (torch.randn(M, K, device=DEV) * scale).contiguous()
    W = (torch.randn(N, K, device=DEV) / K**0.5).contiguous()
    Cm = torch.empty(M, N, device=DEV)
    L.check(lib.adf_linear_forward(A.data_ptr(), W.data_ptr(), None, Cm.data_ptr(), M, N, K, 0, 1,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    ref = A.double() @ W.double().T
    err = float((Cm.double() - ref).norm() / ref.norm())
    assert err < tol, (scale, err)
    # rows of very different magnitude in one launch: each against its own norm
    A[::5] *= 1e-4
    L.check(lib.adf_linear_forward(A.data_ptr(), W.data_ptr(), None, Cm.data_ptr(), M, N, K, 0, 1,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    ref = A.double() @ W.double().T
    assert float(((Cm.double() - ref).norm(dim=1) / ref.norm(dim=1)).max()) < tol


def test_out_of_range_activations_are_lifted_or_fall_back(monkeypatch):
    """LayerNorm gain x 1e5 with x_proj.0 weights x 1e-5: the same function in exact arithmetic, but the GEMM input
    exceeds the fp16 range (|a| > 65504).  With the row lifts the f16x3 forward handles it directly (no fallback, the
    oracle's answer at 1e-4).  Without them (ADF_LIFT=0, the arithmetic of rounds 1-2) the forward produces a non-finite
    output, adf_check_flags reports ADF_ENUMERIC and the engine re-runs in exact f32 - the caller still sees the oracle's
    answer; the sampler does the same for a whole run."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer
    from oracle import painn_oracle as O

    fx = load_npz("painn_small.npz")
    def rescaled():
        mm = small_model(fx)
        with torch.no_grad():
            mm.message_layers[1].x_layernorm.weight.mul_(1.0e5)
            mm.message_layers[1].x_layernorm.bias.mul_(1.0e5)
            mm.message_layers[1].x_proj[0].weight.mul_(1.0e-5)
        return mm

    ml = rescaled()
    b = batch_from_fixture(fx, device=DEV)
    l1, l2 = ml(b)
    assert not ml.engine().exact_f32 and bool(torch.isfinite(l1).all()) and bool(torch.isfinite(l2).all())
    monkeypatch.setenv("ADF_LIFT", "0")
    m = rescaled()
    f1, f2 = m(b)
    assert m.engine().exact_f32 and bool(torch.isfinite(f1).all()) and bool(torch.isfinite(f2).all())
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    bc = batch_from_fixture(fx)
    o1, o2 = O.painn_forward(sd, bc.pos, bc.atomic_numbers, bc.cell, bc.natoms, hidden_channels=int(fx["hp_hidden_channels"]),
                             num_layers=int(fx["hp_num_layers"]), cutoff=float(fx["hp_cutoff"]),
                             max_neighbors=int(fx["hp_max_neighbors"]), scale_factors=m.scale_factors())
    assert rel_err(f1.cpu(), o1) < REL_TOL and rel_err(f2.cpu(), o2) < REL_TOL
    assert rel_err(l1.cpu(), o1) < REL_TOL and rel_err(l2.cpu(), o2) < REL_TOL
    # a fresh engine (f16x3 again) inside the sampler: the run is repeated in exact f32 from the initial placement
    m2 = rescaled()
    params = dict(num_steps=2, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False)
    torch.manual_seed(3)
    out = Denoiser(batch_from_fixture(fx, device=DEV), DiffTorchCalc(DenoisingTrainer(m2, device=DEV)), params,
                   device=DEV).run()
    assert m2.engine().exact_f32 and bool(torch.isfinite(out.pos).all())
    torch.manual_seed(3)
    ref = Denoiser(batch_from_fixture(fx, device=DEV), DiffTorchCalc(DenoisingTrainer(m, device=DEV)), params,
                   device=DEV).run()
    assert torch.equal(out.pos, ref.pos)  # m's engine is in exact f32 already: same arithmetic, same run


def test_painn_small_layers_and_output():
    fx = load_npz("painn_small.npz")
    m = small_model(fx)
    b = batch_from_fixture(fx, device=DEV)
    f1, f2 = m(b)
    assert rel_err(f1.cpu(), fx["f1"]) < REL_TOL
    assert rel_err(f2.cpu(), fx["f2"]) < REL_TOL
    assert max_abs_err_rel_to_max(f1.cpu(), fx["f1"]) < REL_TOL and max_abs_err_rel_to_max(f2.cpu(), fx["f2"]) < REL_TOL
    # per-layer: message block then update block, against the reference's captured activations
    eng = m.engine()
    eng.build_graph(b)
    H = m.hidden_channels
    emb = m.atom_emb.embeddings.weight.detach()
    x = emb[b.atomic_numbers.long() - 1].contiguous()
    vec = torch.zeros(x.shape[0], 3, H, device=DEV)
    for li in range(m.num_layers):
        x_in, vec_in = x.clone(), vec.clone()
        x, vec = eng.message_layer(li, x_in, vec_in)
        dx = x * (2.0 ** 0.5) - x_in
        dvec = vec - vec_in
        assert rel_err(dx.cpu(), fx[f"layer{li}_msg_dx"]) < REL_TOL
        assert rel_err(dvec.cpu(), fx[f"layer{li}_msg_dvec"]) < REL_TOL
        x, vec = eng.update_layer(li, x.contiguous(), vec.contiguous())
        assert rel_err(x.cpu(), fx[f"layer{li}_x"]) < REL_TOL
        assert rel_err(vec.cpu(), fx[f"layer{li}_vec"]) < REL_TOL


def test_forward_is_run_to_run_deterministic():
    """No atomics on floats anywhere on the path (edges are pre-sorted, sums run in registers): two runs of the
    same forward must agree bit for bit.  (Guards against the packed-f32 miscompute seen with SLP
    vectorisation next to the f16 MFMA loop, see adsorbdiff_amd/build.py.)"""
    fx = load_npz("painn_small.npz")
    m = small_model(fx)
    b = batch_from_fixture(fx, device=DEV)
    f1, f2 = m(b)
    for _ in range(5):
        g1, g2 = m(b)
        assert torch.equal(f1, g1) and torch.equal(f2, g2)


def test_exact_f32_mode_matches_default(monkeypatch):
    """ADF_GEMM=f32 selects the exact-f32 MFMA kernels everywhere; the default f16x3-split path must agree
    with it far inside the 1e-4 budget."""
    fx = load_npz("painn_small.npz")
    b = batch_from_fixture(fx, device=DEV)
    f1, f2 = small_model(fx)(b)
    monkeypatch.setenv("ADF_GEMM", "f32")
    e1, e2 = small_model(fx)(b)
    assert rel_err(f1, e1) < 2e-5 and rel_err(f2, e2) < 2e-5
    assert rel_err(e1.cpu(), fx["f1"]) < 1e-5 and rel_err(e2.cpu(), fx["f2"]) < 1e-5


def test_painn_trained_like_magnitudes_vs_reference_fixture(monkeypatch):
    """Reference outputs for weights rescaled to trained-like magnitudes (LayerNorm gain x 0.05, vec stream x 1e-2:
    oracle/make_golden.py section 9): |vec| ~ 1e-3, i.e. every operand row of vec_proj sits below the unlifted fp16
    split's 0.1 threshold.  With the row lifts: 1e-4 on the outputs and on every layer's activations."""
    fx = load_npz("painn_small_scaled.npz")
    b = batch_from_fixture(fx, device=DEV)

    def run():
        m = small_model(fx)
        f1, f2 = m(b)
        eng = m.engine()
        eng.build_graph(b)
        H = m.hidden_channels
        x = m.atom_emb.embeddings.weight.detach()[b.atomic_numbers.long() - 1].contiguous()
        vec = torch.zeros(x.shape[0], 3, H, device=DEV)
        worst = max(rel_err(f1.cpu(), fx["f1"]), rel_err(f2.cpu(), fx["f2"]))
        for li in range(m.num_layers):
            x, vec = eng.message_layer(li, x.contiguous(), vec.contiguous())
            x, vec = eng.update_layer(li, x.contiguous(), vec.contiguous())
            worst = max(worst, rel_err(x.cpu(), fx[f"layer{li}_x"]), rel_err(vec.cpu(), fx[f"layer{li}_vec"]))
        return worst

    lifted = run()
    monkeypatch.setenv("ADF_LIFT", "0")
    unlifted = run()
    print(f"trained-like magnitudes: worst rel err with row lifts {lifted:.2e}, without {unlifted:.2e}")
    assert lifted < REL_TOL


def test_painn_tag_based_Z_no_op_vs_reference_fixture():
    """PaiNN.tag_based_Z (painn_denoising.py:156-168) is a no-op by operator precedence.  The batch has
    H, C, N and O atoms INSIDE the slab (tags 0 and 1); the reference's own forward on it is the fixture: the HIP path
    must embed them with their plain atomic numbers (a "fixed" Z + 100 would leave the 83-row table)."""
    fx = load_npz("painn_tagz.npz")
    light = np.isin(fx["atomic_numbers"], [1, 6, 7, 8]) & (fx["tags"] < 2)
    assert int(light.sum()) >= 6
    m = small_model(fx)
    b = batch_from_fixture(fx, device=DEV)
    f1, f2 = m(b)
    assert torch.equal(b.atomic_numbers.cpu(), torch.from_numpy(fx["atomic_numbers"]).float())  # not modified either
    assert rel_err(f1.cpu(), fx["f1"]) < REL_TOL and rel_err(f2.cpu(), fx["f2"]) < REL_TOL
    assert max_abs_err_rel_to_max(f1.cpu(), fx["f1"]) < REL_TOL and max_abs_err_rel_to_max(f2.cpu(), fx["f2"]) < REL_TOL
    # the rows of the light slab atoms themselves
    idx = torch.from_numpy(np.nonzero(light)[0])
    assert rel_err(f1.cpu()[idx], fx["f1"][light]) < REL_TOL and rel_err(f2.cpu()[idx], fx["f2"][light]) < REL_TOL


def test_painn_full_h512_vs_reference_fixture():
    fx = load_npz("painn_full.npz")
    torch.manual_seed(int(fx["seed"]))
    m = PaiNN(None, 50, 1, cutoff=float(fx["cutoff"]), max_neighbors=int(fx["max_neighbors"]),
              scale_file=PAINN_NB6_SCALE_FACTORS, so3_denoising=True).to(DEV).eval()
    b = batch_from_fixture(fx, device=DEV)
    f1, f2 = m(b)
    assert rel_err(f1.cpu(), fx["f1"]) < REL_TOL
    assert rel_err(f2.cpu(), fx["f2"]) < REL_TOL
    assert max_abs_err_rel_to_max(f1.cpu(), fx["f1"]) < REL_TOL and max_abs_err_rel_to_max(f2.cpu(), fx["f2"]) < REL_TOL


def test_painn_vs_oracle_bench_shape():
    """Seeded benchmark-shaped systems (200 atoms, 10 A, K=50, H=512): HIP vs the CPU oracle."""
    from oracle import painn_oracle as O

    torch.manual_seed(0)
    m = PaiNN(None, 50, 1, cutoff=10.0, max_neighbors=50, scale_file=PAINN_NB6_SCALE_FACTORS,
              so3_denoising=True).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    b = make_batch(3, seed=1000)
    f1_o, f2_o = O.painn_forward(sd, b.pos, b.atomic_numbers, b.cell, b.natoms, cutoff=10.0, max_neighbors=50,
                                 scale_factors=m.scale_factors())
    m = m.to(DEV)
    f1, f2 = m(b.clone().to(DEV))
    assert rel_err(f1.cpu(), f1_o) < REL_TOL
    assert rel_err(f2.cpu(), f2_o) < REL_TOL
    # per-system adsorbate means = the quantities the stepper consumes
    for f, fo in ((f1.cpu(), f1_o), (f2.cpu(), f2_o)):
        s = O.ads_mean(f, b.tags, b.batch, 3)
        so = O.ads_mean(fo, b.tags, b.batch, 3)
        assert rel_err(s, so) < REL_TOL
        assert row_rel_err(s, so) < REL_TOL, row_rel_err(s, so)  # every system against its own score norm
        assert max_abs_err_rel_to_max(f, fo) < REL_TOL


STEP_HP = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)


def _stepper_model(fx):
    m = PaiNN(None, 50, 1, scale_file={"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9},
              so3_denoising=True, **STEP_HP)
    m.load_state_dict(state_dict_from_fixture(fx), strict=False)
    return m


def _params(fx):
    return dict(num_steps=int(fx["num_steps"]), ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01,
                rot_std_high=1.55, ode=bool(int(fx["ode"])))


def _run_denoiser(fx, noise_fn=None, traj_dir=None):
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    tr = DenoisingTrainer(_stepper_model(fx), device=DEV)
    b = batch_from_fixture(fx, pos_key="pos_in")
    torch.manual_seed(int(fx["seed"]))
    den = Denoiser(b, DiffTorchCalc(tr), _params(fx), device=DEV, traj_dir=traj_dir, traj_names=b.sid,
                   noise_fn=noise_fn)
    return den.run(), den


@pytest.mark.parametrize("name", ["ode5", "sde3", "ode8", "ode3_fixed", "ode3_img"])
def test_stepper_each_step_vs_reference_fixture(name):
    """Teacher forcing on the reference's recorded positions: for every step t, start from the positions the
    reference had before its t-th model call, run forward + adf_sde_step and compare with what the REFERENCE recorded
    for that step (oracle/make_golden.py hooks the real Denoiser): the per-system translation and rotation scores
    (north_star: "COM + rotation scores within 1e-4 rel"), the wrapped COM displacement, the rotation vector, and the
    positions afterwards.  ode3_fixed: an adsorbate atom with fixed == 1 (its positions_free row is zeroed, reference
    :498); ode3_img: 75 periodic images per system."""
    from adsorbdiff_amd.denoising_torch import schedule_coefs

    fx = load_npz(f"stepper_{name}.npz")
    m = _stepper_model(fx).to(DEV).eval()
    eng = m.engine()
    params = _params(fx)
    T = params["num_steps"]
    coefs = schedule_coefs(params)
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    prep = eng.prepare(b)
    B, N = prep.num_systems, prep.num_atoms
    if name == "ode3_fixed":
        assert int((b.fixed[b.tags == 2] == 1).sum()) == B
    if name == "ode3_img":
        assert prep.reps[:2] == [2, 2]
    torch.manual_seed(int(fx["seed"]))
    noise = torch.rand(B, 3)
    pos = b.pos.clone().contiguous()
    eng.init_placement(prep, pos, noise.to(DEV))
    log = torch.from_numpy(fx["pos_log"])  # [T,N,3] positions before each model call
    np.testing.assert_allclose(pos.cpu().numpy(), log[0].numpy(), rtol=0, atol=2e-6)
    f1 = torch.empty(N, 3, device=DEV)
    f2 = torch.empty(N, 3, device=DEV)
    tags = torch.from_numpy(fx["tags"])
    ads = (b.tags == 2)
    keep = (b.fixed != 1).float()[:, None]
    cnt = torch.zeros(B, device=DEV).index_add_(0, b.batch[ads], torch.ones(int(ads.sum()), device=DEV))[:, None]
    for t in range(T):
        pos = log[t].to(DEV).contiguous()
        z_tr = z_rot = None
        if not params["ode"]:
            z_tr = torch.normal(mean=0, std=1, size=(B, 3)).to(DEV)
            z_rot = torch.normal(mean=0, std=1, size=(B, 3)).to(DEV)
        state = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
        dcom = torch.empty(B, 3, device=DEV)
        drot = torch.empty(B, 3, device=DEV)
        eng.forward_prepared(prep, pos, f1, f2)
        # (1) the scores: per-system means over the adsorbate atoms, 1e-4 relative per step
        s_tr = torch.zeros(B, 3, device=DEV).index_add_(0, b.batch[ads], f1[ads]) / cnt
        s_rot = torch.zeros(B, 3, device=DEV).index_add_(0, b.batch[ads], (f2 * keep)[ads]) / cnt
        assert rel_err(s_tr.cpu(), fx["ref_score_tr"][t]) < REL_TOL, (name, t, rel_err(s_tr.cpu(), fx["ref_score_tr"][t]))
        assert rel_err(s_rot.cpu(), fx["ref_score_rot"][t]) < REL_TOL, (name, t)
        # each system against its own score norm (floor 1e-7)
        assert row_rel_err(s_tr.cpu(), fx["ref_score_tr"][t]) < REL_TOL, (name, t, row_rel_err(s_tr.cpu(), fx["ref_score_tr"][t]))
        assert row_rel_err(s_rot.cpu(), fx["ref_score_rot"][t]) < REL_TOL, (name, t, row_rel_err(s_rot.cpu(), fx["ref_score_rot"][t]))
        eng.sde_step(prep, pos, f1, f2, coefs[t], state, z_tr, z_rot, early_stop_count=0, dcom=dcom, drot=drot)
        # (2) the update the stepper derives from them.  drot is linear in the score: 1e-4 relative.  dcom is the
        # wrapped displacement cell.frac - com: its error is 1e-4 of the unwrapped step (tens of A at sigma = 10)
        # plus the rounding of a difference of O(10 A) numbers
        assert rel_err(drot.cpu(), fx["ref_drot"][t]) < REL_TOL, (name, t)
        raw_step = abs(coefs[t].coef_tr) * float(np.abs(fx["ref_score_tr"][t]).max())
        tol_com = 1e-4 * raw_step + 2e-5
        assert float((dcom.cpu() - torch.from_numpy(fx["ref_dcom"][t])).abs().max()) < tol_com, (name, t, tol_com)
        # (3) positions after the step: COM error as above + the rotation's 1e-4 * |drot| * lever arm (<= 2 A)
        want = log[t + 1] if t + 1 < T else torch.from_numpy(fx["pos_final"])
        tol = tol_com + 1e-4 * float(np.abs(fx["ref_drot"][t]).max()) * 2.0 + 1e-5
        diff = (pos.cpu() - want).abs()
        assert float(diff.max()) < tol, (name, t, float(diff.max()), tol)
        assert float(diff[tags != 2].max()) == 0.0  # slab atoms never move


def test_sampling_1000_systems_5_steps_spot_check_vs_oracle():
    """BASELINE-size batch through the sampler (5 reverse steps, fused loop, static-atom cache): systems 0, 500 and
    999 must land where the CPU oracle puts them when it samples each of them alone with the same placement noise."""
    from adsorbdiff_amd.data import Batch
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer
    from oracle import painn_oracle as O

    torch.manual_seed(0)
    m = PaiNN(None, 50, 1, cutoff=10.0, max_neighbors=50, scale_file=PAINN_NB6_SCALE_FACTORS, so3_denoising=True).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    B = 1000
    b = make_batch(B, seed=1000)
    data = b.to_data_list()
    torch.manual_seed(7)
    noise = torch.rand(B, 3)
    params = dict(num_steps=5, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False, placement_noise=noise)
    out = Denoiser(b.clone(), DiffTorchCalc(DenoisingTrainer(m, device=DEV)), params, device=DEV).run()
    got = out.pos.cpu()
    assert bool(torch.isfinite(got).all())
    for k in (0, 500, 999):
        one = Batch.from_data_list([data[k]])

        def fn(p):
            return O.painn_forward(sd, p, one.atomic_numbers, one.cell, one.natoms, cutoff=10.0, max_neighbors=50,
                                   scale_factors=m.scale_factors())

        want = O.reverse_sde_sampling_rot(one.pos.clone(), one.cell, one.tags, one.batch, one.fixed, fn,
                                          dict(params, early_stop=False), noise[k : k + 1])
        sl = slice(200 * k, 200 * (k + 1))
        # random-init scores are small (|dcom| << 1 A per step): the 5-step trajectory is well conditioned
        assert float((got[sl] - want).abs().max()) < 1e-4, (k, float((got[sl] - want).abs().max()))


def test_sampling_50_steps_teacher_forced_vs_oracle(tmp_path):
    """The full 50-step schedule of the benchmark (H = 512, 200-atom systems, 10 A, K = 50) on one system of a 4-system
    batch, step by step: the oracle starts every step from the HIP sampler's own previous frame (teacher forcing, so the
    chaos of the free-running trajectory does not enter) and must land on the sampler's next frame."""
    from adsorbdiff_amd.data import Batch
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc, schedule_coefs
    from adsorbdiff_amd.trainer import DenoisingTrainer
    from oracle import painn_oracle as O

    torch.manual_seed(0)
    m = PaiNN(None, 50, 1, cutoff=10.0, max_neighbors=50, scale_file=PAINN_NB6_SCALE_FACTORS, so3_denoising=True).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    B, T, k = 4, 50, 2
    b = make_batch(B, seed=1000)
    torch.manual_seed(11)
    noise = torch.rand(B, 3)
    params = dict(num_steps=T, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False)
    den = Denoiser(b.clone(), DiffTorchCalc(DenoisingTrainer(m, device=DEV)), dict(params, placement_noise=noise), device=DEV,
                   save_full_traj=True, traj_dir=tmp_path, traj_names=[str(i) for i in range(B)])
    den.run()
    assert den.steps_applied == T
    frames = torch.from_numpy(np.load(tmp_path / f"{k}.npz")["positions"])  # [T, 200, 3]: after every step
    assert frames.shape[0] == T
    one = Batch.from_data_list([b.to_data_list()[k]])
    start = O.initial_placement(one.pos.clone(), one.cell, one.tags, one.batch, noise[k : k + 1])
    coefs = schedule_coefs(params)
    worst = 0.0
    for t in range(T):
        p_in = start if t == 0 else frames[t - 1]
        f1, f2 = O.painn_forward(sd, p_in, one.atomic_numbers, one.cell, one.natoms, cutoff=10.0, max_neighbors=50,
                                 scale_factors=m.scale_factors())
        want, dcom, _, _ = O.reverse_step(p_in, one.cell, one.tags, one.batch, f1, f2, one.fixed, t, params)
        s_tr = O.ads_mean(f1, one.tags, one.batch, 1)
        tol = 1e-4 * abs(coefs[t].coef_tr) * float(s_tr.abs().max()) + 2e-5  # 1e-4 of the raw step + rounding of O(10 A) sums
        err = float((frames[t] - want).abs().max())
        worst = max(worst, err / tol)
        assert err < tol, (t, err, tol)
    print(f"50-step teacher-forced check: worst error / tolerance = {worst:.3f}")


def _bench_model():
    """The model the headline is quoted on (bench.py::bench_painn_model: H = 512 x 6, 10 A, K = 50, seed 0, shipped scale
    factors, the last linear map of both heads x 100)."""
    import bench

    return bench.bench_painn_model()


def test_bench_workload_model_teacher_forced_vs_oracle(tmp_path):
    """the HEADLINE workload's own model (heads x 100) on the 50-step schedule of the benchmark, four
    systems of the seed-1000 batch, fused loop with every frame kept.  On 12 steps spread over the schedule and for two
    of the systems the CPU oracle starts from the sampler's own previous frame (teacher forcing) and must (1) give the
    per-system translation / rotation scores the HIP forward gives on that frame (row-wise 1e-4) and (2) land on the
    sampler's next frame."""
    from adsorbdiff_amd.data import Batch
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc, schedule_coefs
    from adsorbdiff_amd.trainer import DenoisingTrainer
    from oracle import painn_oracle as O

    m = _bench_model()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sf = m.scale_factors()
    B, T = 4, 50
    b = make_batch(B, seed=1000)
    torch.manual_seed(0)
    noise = torch.rand(B, 3)
    params = dict(num_steps=T, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False)
    den = Denoiser(b.clone(), DiffTorchCalc(DenoisingTrainer(m, device=DEV)), dict(params, placement_noise=noise), device=DEV,
                   save_full_traj=True, traj_dir=tmp_path, traj_names=[str(i) for i in range(B)])
    den.run()
    assert den.steps_applied == T
    allf = torch.from_numpy(np.load(tmp_path / "batch_0.frames.npy"))   # [T, 800, 3]: the batch after every step
    assert allf.shape == (T, 800, 3)
    start = O.initial_placement(b.pos.clone(), b.cell, b.tags, b.batch, noise)
    coefs = schedule_coefs(params)
    eng = m.engine()
    bd = b.clone().to(DEV)
    prep = eng.prepare(bd)
    f1 = torch.empty(800, 3, device=DEV)
    f2 = torch.empty(800, 3, device=DEV)
    data = b.to_data_list()
    worst_s = worst_p = 0.0
    for t in (0, 1, 2, 3, 5, 8, 12, 20, 30, 40, 45, 49):
        p_in = start if t == 0 else allf[t - 1]
        eng.forward_prepared(prep, p_in.to(DEV).contiguous(), f1, f2)
        s_hip = O.ads_mean(f1.cpu(), b.tags, b.batch, B)
        r_hip = O.ads_mean(f2.cpu() * (b.fixed != 1).float()[:, None], b.tags, b.batch, B)
        for k in (1, 3):
            one = Batch.from_data_list([data[k]])
            sl = slice(200 * k, 200 * (k + 1))
            o1, o2 = O.painn_forward(sd, p_in[sl], one.atomic_numbers, one.cell, one.natoms, cutoff=10.0, max_neighbors=50,
                                     scale_factors=sf)
            s_o = O.ads_mean(o1, one.tags, one.batch, 1)
            r_o = O.ads_mean(o2 * (one.fixed != 1).float()[:, None], one.tags, one.batch, 1)
            es, er = row_rel_err(s_hip[k : k + 1], s_o), row_rel_err(r_hip[k : k + 1], r_o)
            worst_s = max(worst_s, es, er)
            assert es < REL_TOL and er < REL_TOL, (t, k, es, er)
            want, _, _, _ = O.reverse_step(p_in[sl], one.cell, one.tags, one.batch, o1, o2, one.fixed, t, params)
            tol = 1e-4 * abs(coefs[t].coef_tr) * float(s_o.abs().max()) + 2e-5
            err = float((allf[t][sl] - want).abs().max())
            worst_p = max(worst_p, err / tol)
            assert err < tol, (t, k, err, tol)
    print(f"bench workload, teacher-forced: worst score row error {worst_s:.2e}, worst position error / tolerance {worst_p:.3f}")


def test_bench_workload_model_each_step_vs_reference_fixture():
    """The same model on the REAL reference (tests/golden/stepper_bench_gain.npz, oracle/make_golden.py section 11: the
    reference's Denoiser.run on the first two systems of the seed-1000 batch; its cumulative early stop ends the run after
    35 applied steps): teacher forcing on the reference's recorded positions, per step the per-system scores (1e-4
    row-wise), the rotation vector, the wrapped COM displacement and the positions afterwards."""
    from adsorbdiff_amd.denoising_torch import schedule_coefs

    fx = load_npz("stepper_bench_gain.npz")
    m = _bench_model().to(DEV).eval()
    eng = m.engine()
    params = _params(fx)
    T, calls, applied = params["num_steps"], int(fx["model_calls"]), int(fx["steps_applied"])
    coefs = schedule_coefs(params)
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    prep = eng.prepare(b)
    B, N = prep.num_systems, prep.num_atoms
    torch.manual_seed(int(fx["seed"]))
    noise = torch.rand(B, 3)
    pos = b.pos.clone().contiguous()
    eng.init_placement(prep, pos, noise.to(DEV))
    log = torch.from_numpy(fx["pos_log"])  # [calls, N, 3] positions before each model call
    np.testing.assert_allclose(pos.cpu().numpy(), log[0].numpy(), rtol=0, atol=2e-6)
    f1 = torch.empty(N, 3, device=DEV)
    f2 = torch.empty(N, 3, device=DEV)
    tags = torch.from_numpy(fx["tags"])
    ads = (b.tags == 2)
    keep = (b.fixed != 1).float()[:, None]
    cnt = torch.zeros(B, device=DEV).index_add_(0, b.batch[ads], torch.ones(int(ads.sum()), device=DEV))[:, None]
    worst = 0.0
    for t in range(calls):
        pos = log[t].to(DEV).contiguous()
        eng.forward_prepared(prep, pos, f1, f2)
        s_tr = torch.zeros(B, 3, device=DEV).index_add_(0, b.batch[ads], f1[ads]) / cnt
        s_rot = torch.zeros(B, 3, device=DEV).index_add_(0, b.batch[ads], (f2 * keep)[ads]) / cnt
        e1, e2 = row_rel_err(s_tr.cpu(), fx["ref_score_tr"][t]), row_rel_err(s_rot.cpu(), fx["ref_score_rot"][t])
        worst = max(worst, e1, e2)
        assert e1 < REL_TOL and e2 < REL_TOL, (t, e1, e2)
        if t >= applied:
            continue   # the reference broke out of its loop before applying this step
        state = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
        dcom = torch.empty(B, 3, device=DEV)
        drot = torch.empty(B, 3, device=DEV)
        eng.sde_step(prep, pos, f1, f2, coefs[t], state, None, None, early_stop_count=0, dcom=dcom, drot=drot)
        assert rel_err(drot.cpu(), fx["ref_drot"][t]) < REL_TOL, t
        raw_step = abs(coefs[t].coef_tr) * float(np.abs(fx["ref_score_tr"][t]).max())
        tol_com = 1e-4 * raw_step + 2e-5
        assert float((dcom.cpu() - torch.from_numpy(fx["ref_dcom"][t])).abs().max()) < tol_com, (t, tol_com)
        want = log[t + 1] if t + 1 < calls else torch.from_numpy(fx["pos_final"])
        tol = tol_com + 1e-4 * float(np.abs(fx["ref_drot"][t]).max()) * 2.0 + 1e-5
        diff = (pos.cpu() - want).abs()
        assert float(diff.max()) < tol, (t, float(diff.max()), tol)
        assert float(diff[tags != 2].max()) == 0.0
    print(f"bench workload vs the reference's own run: worst per-system score error {worst:.2e} over {calls} model calls")


def test_bench_workload_model_early_stop_matches_the_reference_run():
    """The reference's Denoiser.run on that fixture stopped after 35 applied steps (ten steps with |dcom| <= 1e-3 A on both
    systems): `Denoiser.run()` with its defaults stops at the same step and ends on the same positions (the trajectory is
    well conditioned at this gain: |dcom| <= 0.07 A per step)."""
    fx = load_npz("stepper_bench_gain.npz")
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    b = batch_from_fixture(fx, pos_key="pos_in")
    tr = DenoisingTrainer(_bench_model(), device=DEV)   # (built BEFORE seeding: the model's initialisers draw from the stream)
    torch.manual_seed(int(fx["seed"]))
    den = Denoiser(b, DiffTorchCalc(tr), _params(fx), device=DEV)
    out = den.run()
    assert den.steps_applied == int(fx["steps_applied"]), (den.steps_applied, int(fx["steps_applied"]))
    np.testing.assert_allclose(out.pos.cpu().numpy(), fx["pos_final"], rtol=0, atol=2e-4)


def test_denoiser_end_to_end_vs_reference_fixture(tmp_path):
    fx = load_npz("stepper_ode8.npz")
    out, den = _run_denoiser(fx, traj_dir=tmp_path)
    assert den.steps_applied == 8
    # well-conditioned fixture (|dcom| <= 0.3 A per step): whole trajectory comparable
    np.testing.assert_allclose(out.pos.cpu().numpy(), fx["pos_final"], rtol=0, atol=1e-4)
    files = sorted(p.name for p in tmp_path.iterdir())
    # written under a temporary name, renamed at the end; without the ase package the sink is <sid>.npz
    # plus the batch-level pair of the asynchronous sink (trajectory.py): all frames of the batch in one file + its index
    assert files == sorted([f"{s}.npz" for s in out.sid] + [f"batch_{out.sid[0]}.frames.npy", f"batch_{out.sid[0]}.json"])
    z = np.load(tmp_path / f"{out.sid[0]}.npz")
    assert z["positions"].shape[0] == 8
    assert float(out.y.abs().sum()) == 0.0 and out.force.shape == out.pos.shape  # reference side effects


def test_lift_rule_and_final_frame_records(tmp_path):
    """Hand-off: the 0.1 A lift rule of pred_traj_to_lmdb.py:81-90 on the device vs a restatement in
    numpy, and the per-system records of the final frames."""
    from adsorbdiff_amd.handoff import lift_adsorbates, write_final_frames

    b = make_batch(5, n_slab=36, n_ads=4, seed=77)
    ads = b.tags == 2
    # systems 0..4: adsorbate far above / 0.05 A above / exactly 0.1 A above / below the surface / deep inside
    for k, dz in enumerate((2.0, 0.05, 0.1, -0.3, -4.0)):
        m = (b.batch == k)
        top = float(b.pos[m & (b.tags == 1), 2].max())
        zmin = float(b.pos[m & ads, 2].min())
        b.pos[m & ads, 2] += top + dz - zmin
    want = b.pos.clone().numpy()
    shifts = []
    for k in range(5):
        m = (b.batch == k).numpy()
        a, s1 = m & ads.numpy(), m & (b.tags == 1).numpy()
        diff = want[a, 2].min() - want[s1, 2].max()
        sh = abs(diff) + 0.1 if diff < 0.1 else 0.0
        want[a, 2] += np.float32(sh)
        shifts.append(sh)
    g = b.clone().to(DEV)
    lifted = lift_adsorbates(g)
    np.testing.assert_allclose(lifted.cpu().numpy(), np.array(shifts, np.float32), rtol=0, atol=2e-6)
    np.testing.assert_allclose(g.pos.cpu().numpy(), want, rtol=0, atol=2e-6)
    assert shifts[0] == 0.0 and shifts[1] > 0 and shifts[3] > 0.39
    out = write_final_frames(g, tmp_path / "final_frames.lmdb", apply_lift=False)
    z = np.load(out, allow_pickle=False)
    assert int(z["length"]) == 5 and z["3/pos"].shape == (40, 3) and str(z["4/sid"]) == b.sid[4]
    np.testing.assert_allclose(z["1/pos"], want[40:80], atol=2e-6)


def test_lift_rule_vs_reference_fixture():
    """adf_lift_adsorbates against positions produced by EXECUTING the lift block of the reference's converter
    (scripts/create_lmdbs/pred_traj_to_lmdb.py:81-90, oracle/make_golden.py section 8) on six seeded systems: adsorbate far
    above, 0.05 / 0.1 / 0.0999 A above, below and deep inside the surface."""
    from adsorbdiff_amd.handoff import lift_adsorbates

    fx = load_npz("handoff_lift.npz")
    g = batch_from_fixture(fx, device=DEV)
    lifted = lift_adsorbates(g)
    np.testing.assert_allclose(g.pos.cpu().numpy(), fx["pos_after"], rtol=0, atol=2e-6)
    moved = np.abs(fx["pos_after"] - fx["pos"]).reshape(6, -1).max(axis=1)
    np.testing.assert_allclose(lifted.cpu().numpy(), moved, rtol=0, atol=2e-6)


def test_graph_replay_matches_eager():
    """denoising_pos_params["use_graph"]: one captured hipGraph per step gives bit-identical positions."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("stepper_ode8.npz")
    tr = DenoisingTrainer(_stepper_model(fx), device=DEV)
    outs = []
    for use_graph in (False, True):
        b = batch_from_fixture(fx, pos_key="pos_in")
        torch.manual_seed(int(fx["seed"]))
        den = Denoiser(b, DiffTorchCalc(tr), dict(_params(fx), use_graph=use_graph), device=DEV)
        outs.append(den.run().pos.clone())
        assert den.steps_applied == 8
    assert torch.equal(outs[0], outs[1])


def test_stepper_early_stop_vs_reference_fixture():
    fx = load_npz("stepper_ode_early.npz")
    out, den = _run_denoiser(fx)
    # the reference made 10 model calls and applied 9 updates before its cumulative break
    assert den.steps_applied == 9 and den.cvg_count == 10
    np.testing.assert_allclose(out.pos.cpu().numpy(), fx["pos_final"], rtol=0, atol=1e-5)


def test_ml_diffuse_and_trainer_entry(tmp_path):
    """Driver-level contract: ml_diffuse returns a re-collated batch; run_relaxations skips batches
    whose trajectories already exist (resume rule, reference utils/utils.py:968-973)."""
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("stepper_ode8.npz")
    cfg = {"task": {"relax_opt": {"traj_dir": str(tmp_path)}},
           "optim": {"denoising_pos_params": _params(fx)}}
    tr = DenoisingTrainer(_stepper_model(fx), device=DEV, config=cfg)
    b = batch_from_fixture(fx, pos_key="pos_in")
    torch.manual_seed(int(fx["seed"]))
    res = tr.run_relaxations([b])
    assert len(res) == 1
    np.testing.assert_allclose(res[0].pos.cpu().numpy(), fx["pos_final"], rtol=0, atol=1e-4)
    assert tr.run_relaxations([batch_from_fixture(fx, pos_key="pos_in")]) == []  # every <sid>.traj / .npz present -> skipped


def test_full_size_properties():
    """BASELINE-size batch (1000 systems x 200 atoms, 10 A, K=50, H=512).  Size-independent properties:
    (1) reversing the order of the systems permutes the per-system scores and nothing else;
    (2) a rigid in-plane shift of every atom leaves them unchanged (up to re-rounded positions);
    (3) two systems picked from the middle of the batch agree with the CPU oracle run on them alone."""
    from oracle import painn_oracle as O

    torch.manual_seed(0)
    m = PaiNN(None, 50, 1, cutoff=10.0, max_neighbors=50, scale_file=PAINN_NB6_SCALE_FACTORS,
              so3_denoising=True).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    B = 1000
    b = make_batch(B, seed=1234)
    f1, f2 = m(b.clone().to(DEV))
    assert bool(torch.isfinite(f1).all()) and bool(torch.isfinite(f2).all())
    s1 = O.ads_mean(f1.cpu(), b.tags, b.batch, B)
    # (1) reverse the order of the systems
    rev = type(b).from_data_list(list(reversed(b.to_data_list())))
    g1, _ = m(rev.clone().to(DEV))
    t1 = O.ads_mean(g1.cpu(), rev.tags, rev.batch, B)
    assert rel_err(t1.flip(0), s1) < REL_TOL
    # (2) rigid shift of everything by 0.37 A in x / -0.21 A in y keeps all interatomic vectors
    sh = b.clone()
    sh.pos = sh.pos + torch.tensor([0.37, -0.21, 0.0])
    h1, _ = m(sh.to(DEV))
    u1 = O.ads_mean(h1.cpu(), b.tags, b.batch, B)
    per_sys = (u1 - s1).norm(dim=1) / s1.norm(dim=1)
    # positions are re-rounded, so a K-th-neighbour near-tie can flip in a handful of systems
    assert float(per_sys.median()) < 1e-4 and float((per_sys > 1e-3).float().mean()) < 0.01
    # (3) systems 500 and 777 against the oracle evaluated on them alone
    data = b.to_data_list()
    for k in (500, 777):
        one = type(b).from_data_list([data[k]])
        r1, r2 = O.painn_forward(sd, one.pos, one.atomic_numbers, one.cell, one.natoms, cutoff=10.0, max_neighbors=50,
                                 scale_factors=m.scale_factors())
        sl = slice(200 * k, 200 * (k + 1))
        assert rel_err(f1[sl].cpu(), r1) < REL_TOL and rel_err(f2[sl].cpu(), r2) < REL_TOL


def _oracle_vs_hip(b, hp, seed=0, so3=True, pbc=None, scale=None):
    from oracle import painn_oracle as O

    torch.manual_seed(seed)
    m = PaiNN(None, 50, 1, so3_denoising=so3, scale_file=scale, **hp).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    kw = dict(hidden_channels=hp["hidden_channels"], num_layers=hp["num_layers"], cutoff=hp["cutoff"],
              max_neighbors=hp["max_neighbors"], scale_factors=m.scale_factors(), so3_denoising=so3)
    if pbc is not None:
        graph = O.radius_graph_pbc(b.pos, b.cell, b.natoms, hp["cutoff"], hp["max_neighbors"], pbc=pbc)
        ei, d, v, _ = O.pbc_distances(b.pos, graph[0], b.cell, graph[1], graph[2])
        ei, sh, nb, d, u = O.symmetrize_edges(ei, graph[1], graph[2], d, v / d[:, None])
        kw["graph"] = (ei, nb, d, u)
    ref = O.painn_forward(sd, b.pos, b.atomic_numbers, b.cell, b.natoms, **kw)
    bd = b.clone().to(DEV)
    if pbc is not None:
        bd.pbc = torch.tensor([list(pbc)] * len(b.natoms))
    out = m.to(DEV)(bd)
    return out, ref


def test_ragged_batch_vs_oracle():
    """Systems of different sizes in one batch (16+3, 100+4 and 36+4 atoms; N = 163 is not a multiple of the
    32-atom work groups)."""
    from adsorbdiff_amd.data import Batch

    parts = (make_batch(1, n_slab=16, n_ads=3, seed=61).to_data_list() + make_batch(1, n_slab=100, n_ads=4, seed=62).to_data_list()
             + make_batch(1, n_slab=36, n_ads=4, seed=63).to_data_list())
    b = Batch.from_data_list(parts)
    hp = dict(hidden_channels=128, num_layers=3, cutoff=6.0, max_neighbors=20)
    (f1, f2), (r1, r2) = _oracle_vs_hip(b, hp, scale={"upd_out_scalar_scale_1": 0.8})
    assert rel_err(f1.cpu(), r1) < REL_TOL and rel_err(f2.cpu(), r2) < REL_TOL


def test_single_head_and_k_not_binding():
    """so3_denoising=False returns one tensor; a tiny cutoff keeps every centre below K neighbours."""
    b = make_batch(2, n_slab=36, n_ads=2, seed=64)
    hp = dict(hidden_channels=128, num_layers=2, cutoff=3.0, max_neighbors=50)
    out, ref = _oracle_vs_hip(b, hp, so3=False)
    assert torch.is_tensor(out) and out.shape == (76, 3)
    assert rel_err(out.cpu(), ref) < REL_TOL


def test_non_periodic_z_vs_oracle():
    """data.pbc = [T, T, F]: no images along the third lattice vector (reference utils/utils.py:566-576,650-655)."""
    b = make_batch(2, n_slab=36, n_ads=4, seed=65)
    b.cell[:, 2, 2] = 9.0  # short c axis: periodic images along z would be inside the cutoff
    b.pos[:, 2] -= 6.0
    hp = dict(hidden_channels=128, num_layers=2, cutoff=6.0, max_neighbors=20)
    (f1, f2), (r1, r2) = _oracle_vs_hip(b, hp, pbc=(True, True, False))
    assert rel_err(f1.cpu(), r1) < REL_TOL and rel_err(f2.cpu(), r2) < REL_TOL
    (g1, _), (s1, _) = _oracle_vs_hip(b, hp)  # fully periodic gives a different answer
    assert rel_err(g1.cpu(), s1) < REL_TOL and rel_err(g1.cpu(), r1) > 1e-3


def test_weight_update_is_picked_up():
    """EMA-style in-place parameter changes re-bind / re-pack the device weights."""
    fx = load_npz("painn_small.npz")
    m = small_model(fx)
    b = batch_from_fixture(fx, device=DEV)
    f1, _ = m(b)
    with torch.no_grad():
        m.message_layers[0].rbf_proj.weight.mul_(1.5)
        m.update_layers[1].xvec_proj[2].bias.add_(0.3)
    g1, _ = m(b)
    assert rel_err(g1, f1) > 1e-3
    with torch.no_grad():
        m.message_layers[0].rbf_proj.weight.div_(1.5)
        m.update_layers[1].xvec_proj[2].bias.sub_(0.3)
    h1, _ = m(b)
    assert rel_err(h1, f1) < 1e-6


def test_ema_param_data_copy_is_picked_up():
    """The reference's EMA writes through param.data.copy_ (modules/exponential_moving_average.py:113,147), which
    bumps no autograd version counter: the engine key fingerprints the contents.  An engine that already packed the
    raw weights must sample with the EMA weights inside the EMA scope and with the raw ones after restore()."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.exponential_moving_average import ExponentialMovingAverage
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("painn_small.npz")
    m = small_model(fx)
    b = batch_from_fixture(fx, device=DEV)
    raw1, _ = m(b)                                   # engine created and packed with the raw weights
    ema = ExponentialMovingAverage(m.parameters(), 0.5)
    with torch.no_grad():
        for s_ in ema.shadow_params:
            s_.mul_(0.9)                             # shadow != raw
    versions = [p._version for p in m.parameters()]
    ema.store(); ema.copy_to()
    assert [p._version for p in m.parameters()] == versions  # the hazard: nothing autograd-visible changed
    in_scope, _ = m(b)
    ref = small_model(fx)                            # a second model that simply holds the shadow weights
    with torch.no_grad():
        for p, s_ in zip([q for q in ref.parameters() if q.requires_grad], ema.shadow_params):
            p.copy_(s_)
    want, _ = ref(b)
    assert rel_err(in_scope, raw1) > 1e-3 and torch.equal(in_scope, want)
    ema.restore()
    raw2, _ = m(b)
    assert torch.equal(raw2, raw1)
    # sampler: a trainer with an EMA samples with the shadow weights although the engine was bound to the raw ones
    params = dict(num_steps=3, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False)
    torch.manual_seed(3)
    a = Denoiser(batch_from_fixture(fx, device=DEV), DiffTorchCalc(DenoisingTrainer(m, device=DEV, ema=ema)), params,
                 device=DEV).run().pos.clone()
    torch.manual_seed(3)
    c = Denoiser(batch_from_fixture(fx, device=DEV), DiffTorchCalc(DenoisingTrainer(ref, device=DEV)), params,
                 device=DEV).run().pos.clone()
    assert torch.equal(a, c)
    raw3, _ = m(b)
    assert torch.equal(raw3, raw1)


def test_bad_atomic_number_is_reported():
    """Z outside the embedding table raises instead of reading out of bounds (torch's nn.Embedding: IndexError)."""
    fx = load_npz("painn_small.npz")
    m = small_model(fx)
    b = batch_from_fixture(fx, device=DEV)
    b.atomic_numbers = b.atomic_numbers.clone()
    b.atomic_numbers[0] = 0
    with pytest.raises(ValueError, match="atomic number"):
        m(b)
    b.atomic_numbers[0] = 200
    with pytest.raises(ValueError, match="atomic number"):
        m(b)
    m(batch_from_fixture(fx, device=DEV))  # flags were cleared by the failed checks


def test_hub_atom_with_many_incoming_edges():
    """In-degree is not bounded by 2K (only sum(deg) <= 2NK): a hub listed by > 256 centres takes the register path
    of the per-target sorter; the message layer must still match the oracle."""
    import math

    from oracle import painn_oracle as O

    from adsorbdiff_amd.data import Batch

    torch.manual_seed(11)
    n, K, rc = 900, 120, 12.0
    # log-uniform radii around a hub atom, isotropic directions: the hub is among the K nearest of many centres
    # (272 incoming edges with this seed), the other atoms see 100-200
    r = torch.exp(torch.rand(n - 1) * math.log(11.0 / 0.02)) * 0.02
    pos = torch.zeros(n, 3)
    pos[1:] = torch.nn.functional.normalize(torch.randn(n - 1, 3), dim=1) * r[:, None]
    b = Batch()
    b.pos = (pos + 50.0).float(); b.atomic_numbers = torch.randint(1, 80, (n,)).float()
    b.tags = torch.ones(n, dtype=torch.long); b.fixed = torch.zeros(n, dtype=torch.long)
    b.cell = (torch.eye(3) * 100.0).reshape(1, 3, 3); b.natoms = torch.tensor([n]); b.batch = torch.zeros(n, dtype=torch.long)
    b.sid = ["hub"]
    torch.manual_seed(0)
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=2, cutoff=rc, max_neighbors=K, so3_denoising=True).to(DEV).eval()
    f1, f2 = m(b.to(DEV))
    eng = m.engine()
    eng.build_graph(b.to(DEV))
    _, _, _, es, ed, _, _ = eng.export_graph()
    indeg = torch.bincount(ed.long().cpu(), minlength=n)
    assert int(indeg.max()) > 256, int(indeg.max())
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    o1, o2 = O.painn_forward(sd, b.pos.cpu(), b.atomic_numbers.cpu(), b.cell.cpu(), b.natoms.cpu(), hidden_channels=128,
                             num_layers=2, cutoff=rc, max_neighbors=K, scale_factors=m.scale_factors())
    assert rel_err(f1.cpu(), o1) < REL_TOL and rel_err(f2.cpu(), o2) < REL_TOL


_CSR_SCRIPT = r"""
import math, sys, numpy as np, torch
sys.path.insert(0, {root!r})
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.painn_denoising import PaiNN
from adsorbdiff_amd.synthetic import make_batch, make_system
out = {{}}
def export(name, b, **hp):
    torch.manual_seed(0)
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, so3_denoising=True, **hp).to("cuda:0").eval()
    eng = m.engine()
    E = eng.build_graph(b.clone().to("cuda:0"))
    cnt, src, sh, es, ed, dist, vec = eng.export_graph()
    for k, v in (("es", es), ("ed", ed), ("dist", dist), ("vec", vec)):
        out[name + "_" + k] = v.cpu().numpy()
    out[name + "_E"] = np.int64(E)
# (a) benchmark-shaped systems; (b) small cells with many periodic images; (c) a system of 300 atoms (> 256: global path)
#     between two that fit; (d) the hub atom: one segment beyond the per-wave sorter
export("bench", make_batch(5, seed=1000), cutoff=10.0, max_neighbors=50)
export("img", make_batch(4, n_slab=9, n_ads=4, seed=60), cutoff=6.0, max_neighbors=20)
g = torch.Generator().manual_seed(3)
export("mixed", Batch.from_data_list([make_system(g, 196, 4, "0"), make_system(g, 296, 4, "1"), make_system(g, 100, 4, "2")]),
       cutoff=10.0, max_neighbors=50)
torch.manual_seed(11)
n = 900
r = torch.exp(torch.rand(n - 1) * math.log(11.0 / 0.02)) * 0.02
pos = torch.zeros(n, 3)
pos[1:] = torch.nn.functional.normalize(torch.randn(n - 1, 3), dim=1) * r[:, None]
b = Batch()
b.pos = (pos + 50.0).float(); b.atomic_numbers = torch.randint(1, 80, (n,)).float()
b.tags = torch.ones(n, dtype=torch.long); b.fixed = torch.zeros(n, dtype=torch.long)
b.cell = (torch.eye(3) * 100.0).reshape(1, 3, 3); b.natoms = torch.tensor([n]); b.batch = torch.zeros(n, dtype=torch.long)
b.sid = ["hub"]
export("hub", b, cutoff=12.0, max_neighbors=120)
small = Batch.from_data_list(make_batch(2, seed=7).to_data_list() + [b.to_data_list()[0]])
export("hubmixed", small, cutoff=12.0, max_neighbors=120)
np.savez({dst!r}, **out)
"""


def test_system_csr_kernels_equal_the_global_pipeline(tmp_path):
    """Round 6: count / fill / sort of a system out of LDS (graph.hip, one workgroup per system) against the global-memory
    pipeline it replaces (ADF_GRAPH_SYS_CSR=0; the switch is read once per process, hence two children): the exported
    symmetrised graph - edge order inside every target's segment included - must be the SAME BYTES, for systems that fit,
    for one that does not (300 atoms between two that do), and for a hub atom whose segment exceeds the per-wave sorter."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parent.parent)
    res = {}
    for mode in ("0", "1"):
        env = dict(os.environ, ADF_GRAPH_SYS_CSR=mode)
        dst = str(tmp_path / f"csr{mode}.npz")
        r = subprocess.run([sys.executable, "-c", _CSR_SCRIPT.format(root=root, dst=dst)], env=env, capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[mode] = dict(np.load(dst))
    assert set(res["0"]) == set(res["1"])
    for k in sorted(res["0"]):
        a, b_ = res["0"][k], res["1"][k]
        assert a.shape == b_.shape and a.tobytes() == b_.tobytes(), k
    assert int(res["1"]["bench_E"]) > 40000 and int(np.bincount(res["1"]["hub_ed"]).max()) > 256


def test_calculator_single_structure_api():
    """AdsorbDiffCalculator.run_diffusion on one structure against the CPU oracle's reverse loop on the same system with the
    same placement noise (the calculator seeds torch's CPU generator, the Denoiser draws torch.rand(1, 3) from it -
    reference calculator.py:180-210, denoising_torch.py:215): final positions within 2e-4 A over the 8 well-conditioned
    steps of the fixture's schedule; tags and atom order preserved."""
    from adsorbdiff_amd.calculator import AdsorbDiffCalculator, SimpleAtoms
    from adsorbdiff_amd.data import Batch
    from oracle import painn_oracle as O

    fx = load_npz("stepper_ode8.npz")
    params = dict(_params(fx), early_stop=False)
    b = batch_from_fixture(fx, pos_key="pos_in")
    one = b.to_data_list()[0]
    atoms = SimpleAtoms(one.atomic_numbers.long().numpy(), one.pos.numpy(), one.cell[0].numpy(), one.tags.numpy(),
                        one.fixed.numpy())
    model = _stepper_model(fx)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    calc = AdsorbDiffCalculator(model, params, device=DEV, seed=11)
    out = calc.run_diffusion(atoms)
    ob = Batch.from_data_list([one])
    torch.manual_seed(11)
    noise = torch.rand(1, 3)   # what the Denoiser drew after the calculator's torch.manual_seed(11)

    def fn(p):
        return O.painn_forward(sd, p, ob.atomic_numbers, ob.cell, ob.natoms, scale_factors=[1.05, 0.9], **STEP_HP)

    want = O.reverse_sde_sampling_rot(ob.pos.clone(), ob.cell, ob.tags, ob.batch, ob.fixed, fn, params, noise)
    moved = float((want - ob.pos).abs().max())
    assert moved > 0.5, moved   # the adsorbate was placed and stepped, not left where it was
    np.testing.assert_allclose(out.get_positions(), want.numpy(), rtol=0, atol=2e-4)
    assert (out.get_tags() == one.tags.numpy()).all()


def test_other_hyperparameters_vs_oracle():
    """H=256, R=64, K=30, 1 layer: exercises the generic paths (4 channel slices, 64-deep basis)."""
    b = make_batch(2, n_slab=36, n_ads=4, seed=66)
    from oracle import painn_oracle as O

    torch.manual_seed(4)
    m = PaiNN(None, 50, 1, hidden_channels=256, num_layers=1, num_rbf=64, cutoff=5.0, max_neighbors=30,
              so3_denoising=True).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    r1, r2 = O.painn_forward(sd, b.pos, b.atomic_numbers, b.cell, b.natoms, hidden_channels=256, num_layers=1,
                             num_rbf=64, cutoff=5.0, max_neighbors=30, scale_factors=[1.0])
    f1, f2 = m.to(DEV)(b.clone().to(DEV))
    assert rel_err(f1.cpu(), r1) < REL_TOL and rel_err(f2.cpu(), r2) < REL_TOL


@pytest.mark.parametrize("shape", [dict(n_slab=36, n_ads=4, cutoff=6.0, K=20), dict(n_slab=196, n_ads=4, cutoff=10.0, K=50)])
def test_static_atom_cache_gives_identical_graph(shape):
    """adf_graph_set_moving: after the adsorbate moved, the cached incremental top-K equals a full rebuild."""
    b = make_batch(3, n_slab=shape["n_slab"], n_ads=shape["n_ads"], seed=71).to(DEV)
    m = graph_model(shape["cutoff"], shape["K"])
    eng = m.engine()
    prep = eng.prepare(b)
    eng.set_moving_atoms(prep, b.tags == 2)
    eng.build_graph(b)  # full evaluation + cache fill
    g = torch.Generator().manual_seed(5)
    for trial in range(3):
        moved = b.clone()
        ads = moved.tags == 2
        moved.pos[ads] = moved.pos[ads] + (torch.rand(int(ads.sum()), 3, generator=g).to(DEV) - 0.5) * torch.tensor(
            [6.0, 6.0, 1.5], device=DEV)
        E_inc = eng.build_graph(moved)  # incremental
        inc = [t.clone() for t in eng.export_graph()]
        eng.set_moving_atoms(None, None)
        E_full = eng.build_graph(moved)
        full = eng.export_graph()
        assert E_inc == E_full
        for a, f in zip(inc[:3], full[:3]):
            assert torch.equal(a, f)
        for a, f in zip(inc[3:], full[3:]):
            assert torch.equal(a, f)  # edges are sorted per target, so even the order matches
        eng.set_moving_atoms(prep, b.tags == 2)
        eng.build_graph(b)  # refill the cache from the reference positions
    eng.set_moving_atoms(None, None)


def test_forward_subset_rows_are_bit_identical():
    """adf_painn_forward_subset: the listed atoms' outputs equal the full forward's bit for bit (last layer and
    heads evaluated on compact rows); the other rows are not written."""
    b = make_batch(3, n_slab=60, n_ads=4, seed=17).to(DEV)
    torch.manual_seed(3)
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=3, num_rbf=32, cutoff=6.0, max_neighbors=20,
              so3_denoising=True, scale_file={f"upd_out_scalar_scale_{i}": 1.0 for i in range(3)}).to(DEV).eval()
    eng = m.engine()
    prep = eng.prepare(b)
    N = b.pos.shape[0]
    full1, full2 = torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV)
    eng.forward_prepared(prep, b.pos, full1, full2)
    idx = torch.nonzero(b.tags == 2).reshape(-1).to(torch.int32)
    sub1, sub2 = torch.full((N, 3), 7.0, device=DEV), torch.full((N, 3), 7.0, device=DEV)
    eng.forward_prepared(prep, b.pos, sub1, sub2, idx)
    torch.cuda.synchronize()
    sel = idx.long()
    assert torch.equal(sub1[sel], full1[sel]) and torch.equal(sub2[sel], full2[sel])
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[sel] = False
    assert bool((sub1[rest] == 7.0).all()) and bool((sub2[rest] == 7.0).all())
    # a scattered, non-adsorbate subset as well (single-layer model: the subset path starts at layer 0)
    torch.manual_seed(4)
    m1 = PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, num_rbf=32, cutoff=6.0, max_neighbors=20,
               so3_denoising=True, scale_file={"upd_out_scalar_scale_0": 1.0}).to(DEV).eval()
    e1 = m1.engine()
    p1 = e1.prepare(b)
    e1.forward_prepared(p1, b.pos, full1, full2)
    idx2 = torch.arange(1, N, 5, dtype=torch.int32, device=DEV)
    e1.forward_prepared(p1, b.pos, sub1, sub2, idx2)
    torch.cuda.synchronize()
    assert torch.equal(sub1[idx2.long()], full1[idx2.long()]) and torch.equal(sub2[idx2.long()], full2[idx2.long()])


@pytest.mark.parametrize("case", ["ode", "sde", "early_stop", "trajectory_sink", "per_step"])
def test_scores_on_adsorbate_only_gives_identical_samples(tmp_path, case):
    """denoising_pos_params["scores_on_adsorbate_only"] (the DEFAULT inside the fused loop since round 5): the sampled
    positions equal the full-output run's bit for bit - ODE, SDE (same device noise stream), under the reference's early
    stop, with the per-step trajectory sink (identical files), and on the per-step host path; and a run WITHOUT the key
    equals both (whichever form the default picks)."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("stepper_ode_early.npz" if case == "early_stop" else "stepper_ode8.npz")
    tr = DenoisingTrainer(_stepper_model(fx), device=DEV)
    outs, steps = [], []
    for flag in (False, True, None):
        b = batch_from_fixture(fx, pos_key="pos_in")
        torch.manual_seed(int(fx["seed"]))
        torch.cuda.manual_seed(4321)
        params = dict(_params(fx))
        if case == "sde":
            params.update(ode=False)
        if case != "early_stop":
            params.update(early_stop=False)
        if case == "per_step":
            params.update(step_hook=lambda t: None)
        if flag is not None:
            params.update(scores_on_adsorbate_only=flag)
        kw = dict(traj_dir=tmp_path / str(flag), traj_names=b.sid) if case == "trajectory_sink" else {}
        den = Denoiser(b, DiffTorchCalc(tr), params, device=DEV, **kw)
        outs.append(den.run().pos.clone())
        steps.append(den.steps_applied)
    assert steps[0] == steps[1] == steps[2] and (case == "early_stop" or steps[0] == 8)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    if case == "trajectory_sink":
        for sid in batch_from_fixture(fx, pos_key="pos_in").sid:
            a, c = np.load(tmp_path / "False" / f"{sid}.npz"), np.load(tmp_path / "None" / f"{sid}.npz")
            assert np.array_equal(a["positions"], c["positions"]) and a["positions"].shape[0] == 8


@pytest.mark.parametrize("ode", [True, False])
def test_fused_loop_matches_per_step_loop(tmp_path, ode):
    """adf_sample (whole loop in one call), adf_sample_traj (the same with a frame leaving the device after every step,
    csrc/frames.hip + trajectory.py's writer thread) and the per-step host loop (taken when a step hook is installed; it
    clones the positions after every step): identical final positions, ODE and SDE (the SDE noise is drawn from the
    device generator in the same order on all paths), and the two trajectory sinks write IDENTICAL files - per system
    <sid>.npz with one frame per applied step, plus the batch file and its index."""
    import json

    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("stepper_ode8.npz")
    tr = DenoisingTrainer(_stepper_model(fx), device=DEV)
    outs = []
    for mode in ("fused", "fused_sink", "per_step"):
        b = batch_from_fixture(fx, pos_key="pos_in")
        torch.manual_seed(int(fx["seed"]))
        torch.cuda.manual_seed(1234)
        extra = {"step_hook": (lambda t: None)} if mode == "per_step" else {}
        den = Denoiser(b, DiffTorchCalc(tr), dict(_params(fx), ode=ode, early_stop=False, **extra), device=DEV,
                       traj_dir=(tmp_path / mode) if mode != "fused" else None, traj_names=b.sid)
        outs.append(den.run().pos.clone())
        assert den.steps_applied == 8
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for sid in batch_from_fixture(fx, pos_key="pos_in").sid:
        a, c = np.load(tmp_path / "fused_sink" / f"{sid}.npz"), np.load(tmp_path / "per_step" / f"{sid}.npz")
        assert a["positions"].shape[0] == 8
        for k in ("positions", "numbers", "tags", "fixed", "cell"):
            assert np.array_equal(a[k], c[k]), (sid, k)
    idx = json.loads((tmp_path / "fused_sink" / f"batch_{b.sid[0]}.json").read_text())
    frames = np.load(tmp_path / "fused_sink" / idx["frames_file"])
    assert frames.shape == (8, outs[0].shape[0], 3) and idx["frames"] == 8 and idx["sids"] == list(b.sid)
    assert np.array_equal(frames[-1], outs[1].cpu().numpy())
    assert not list((tmp_path / "fused_sink").glob("*_tmp"))   # everything was renamed to its final name


def test_trajectory_sink_early_stop_and_final_frame_only(tmp_path):
    """The sink under the reference's early stop (cumulative count, break BEFORE applying: the frames pushed after the stop
    are dropped, one frame per APPLIED step remains) and with save_full_traj=False (the final frame only), and a ring of 2
    slots (the enqueueing thread has to wait for the writer)."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("stepper_ode_early.npz")
    tr = DenoisingTrainer(_stepper_model(fx), device=DEV)
    res = {}
    for mode, full in (("sink", True), ("per_step", True), ("last", False)):
        b = batch_from_fixture(fx, pos_key="pos_in")
        torch.manual_seed(int(fx["seed"]))
        extra = {"step_hook": (lambda t: None)} if mode == "per_step" else {}
        den = Denoiser(b, DiffTorchCalc(tr), dict(_params(fx), trajectory_ring_slots=2, **extra), device=DEV,
                       traj_dir=tmp_path / mode, traj_names=b.sid, save_full_traj=full)
        out = den.run()
        res[mode] = (den.steps_applied, out.pos.cpu().numpy(), np.load(tmp_path / mode / f"{b.sid[0]}.npz")["positions"])
    n = res["sink"][0]
    assert n == res["per_step"][0] == 9 and n < int(fx["num_steps"])   # the reference applied 9 updates before its break
    assert res["sink"][2].shape[0] == max(n, 1) and np.array_equal(res["sink"][2], res["per_step"][2])
    assert res["last"][2].shape[0] == 1
    na = res["last"][2].shape[1]
    assert np.array_equal(res["last"][2][0], res["last"][1][:na])


def test_static_promise_forward_is_bit_identical():
    """adf_graph_set_moving also lets the forward keep the layer-0 gather records (they depend on the atomic
    numbers only): after the adsorbate moved, the outputs equal those of a forward without any promise."""
    b = make_batch(3, n_slab=60, n_ads=4, seed=23).to(DEV)
    torch.manual_seed(5)
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=2, num_rbf=32, cutoff=6.0, max_neighbors=20,
              so3_denoising=True, scale_file={f"upd_out_scalar_scale_{i}": 1.0 for i in range(2)}).to(DEV).eval()
    eng = m.engine()
    prep = eng.prepare(b)
    N = b.pos.shape[0]
    g = torch.Generator().manual_seed(9)
    ads = b.tags == 2
    eng.set_moving_atoms(prep, ads)
    pos = b.pos.clone()
    cached = []
    for trial in range(3):
        f1, f2 = torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV)
        eng.forward_prepared(prep, pos, f1, f2)
        cached.append((pos.clone(), f1, f2))
        pos = pos.clone()
        pos[ads] = pos[ads] + (torch.rand(int(ads.sum()), 3, generator=g).to(DEV) - 0.5) * 2.0
    eng.set_moving_atoms(None, None)
    for p_, c1, c2 in cached:
        f1, f2 = torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV)
        eng.forward_prepared(prep, p_, f1, f2)
        assert torch.equal(f1, c1) and torch.equal(f2, c2)


def test_incremental_layers_forward_is_bit_identical():
    """Incremental layers (adf_painn_set_incremental): a sequence of forwards under a static-atom promise — adsorbate
    moved a little, a lot, not at all; all outputs and adsorbate-only outputs interleaved — equals, bit for bit, the
    same forwards with every row recomputed.  The cutoff is short against the cell so that the recompute lists of the
    first layers are proper subsets, and the row counters must show it."""
    b = make_batch(4, n_slab=196, n_ads=4, seed=31).to(DEV)
    torch.manual_seed(8)
    L = 4
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=L, num_rbf=32, cutoff=3.6, max_neighbors=12,
              so3_denoising=True, scale_file={f"upd_out_scalar_scale_{i}": 1.0 for i in range(L)}).to(DEV).eval()
    eng = m.engine()
    prep = eng.prepare(b)
    N = b.pos.shape[0]
    ads = b.tags == 2
    idx = torch.nonzero(ads).reshape(-1).to(torch.int32)
    g = torch.Generator().manual_seed(10)
    moves = [0.05, 0.05, 0.0, 3.0, 0.2, 0.0, 0.1, 1.5, 0.05, 0.05]
    subset = [False, False, False, False, True, True, False, True, True, False]
    seq, pos = [], b.pos.clone()
    for mv in moves:
        pos = pos.clone()
        pos[ads] = pos[ads] + (torch.rand(int(ads.sum()), 3, generator=g).to(DEV) - 0.5) * 2.0 * mv
        seq.append(pos)

    def run(incremental):
        eng.set_moving_atoms(prep, ads)
        eng.set_incremental(incremental)
        outs = []
        for p_, sub in zip(seq, subset):
            f1, f2 = torch.zeros(N, 3, device=DEV), torch.zeros(N, 3, device=DEV)
            eng.forward_prepared(prep, p_, f1, f2, idx if sub else None)
            outs.append((f1, f2))
        torch.cuda.synchronize()
        c = eng.counters()
        eng.set_moving_atoms(None, None)
        return outs, c

    ref, c_ref = run(False)
    inc, c_inc = run(True)
    for (a1, a2), (b1, b2), sub in zip(ref, inc, subset):
        sel = idx.long() if sub else slice(None)
        assert torch.equal(a1[sel], b1[sel]) and torch.equal(a2[sel], b2[sel])
    assert c_ref.inc_rows_full == 0  # the plain path does not count
    assert c_inc.inc_rows_full == len(moves) * L * N
    assert 0 < c_inc.inc_rows < 0.7 * c_inc.inc_rows_full, (c_inc.inc_rows, c_inc.inc_rows_full)
    eng.set_incremental(True)


def test_incremental_layers_survive_foreign_builds_and_weight_updates():
    """The kept layer state must not outlive what it was computed from: a stand-alone graph build between two forwards
    (the previous-CSR buffers then hold a foreign graph) and an in-place weight update both force a full recompute."""
    b = make_batch(3, n_slab=100, n_ads=4, seed=37).to(DEV)
    torch.manual_seed(9)
    L = 3
    m = PaiNN(None, 50, 1, hidden_channels=128, num_layers=L, num_rbf=32, cutoff=3.6, max_neighbors=12,
              so3_denoising=True, scale_file={f"upd_out_scalar_scale_{i}": 1.0 for i in range(L)}).to(DEV).eval()
    eng = m.engine()
    prep = eng.prepare(b)
    N = b.pos.shape[0]
    ads = b.tags == 2
    g = torch.Generator().manual_seed(12)

    def moved(p, amp):
        q = p.clone()
        q[ads] = q[ads] + (torch.rand(int(ads.sum()), 3, generator=g).to(DEV) - 0.5) * 2.0 * amp
        return q

    def fwd(p):
        f1, f2 = torch.zeros(N, 3, device=DEV), torch.zeros(N, 3, device=DEV)
        m.engine().forward_prepared(prep, p, f1, f2)  # engine(): re-binds the weights when they changed
        return f1, f2

    p0 = b.pos.clone(); p1 = moved(p0, 0.1); p2 = moved(p1, 0.1); p3 = moved(p2, 0.1)
    eng.set_moving_atoms(prep, ads)
    eng.set_incremental(True)
    got = [fwd(p0), fwd(p1)]
    other = b.clone(); other.pos = moved(p1, 2.0)
    eng.build_graph(other)  # foreign build: same handle, different positions
    got.append(fwd(p2))
    w = m.message_layers[1].x_proj[0].weight
    w_old = w.detach().clone()
    w_new = w_old * 1.01
    with torch.no_grad():   # in-place update, like an optimizer step / EMA copy
        w.copy_(w_new)
    got.append(fwd(p3))
    eng.set_incremental(False)
    eng.set_moving_atoms(None, None)
    with torch.no_grad():
        w.copy_(w_old)
    ref = [fwd(p0), fwd(p1), fwd(p2)]
    with torch.no_grad():
        w.copy_(w_new)
    ref.append(fwd(p3))
    eng.set_incremental(True)
    for k, ((a1, a2), (b1, b2)) in enumerate(zip(got, ref)):
        assert torch.equal(a1, b1) and torch.equal(a2, b2), k


def test_incremental_layers_switch_gives_identical_samples():
    """denoising_pos_params["incremental_layers"]=False recomputes every row every step: same sampled positions, with
    and without scores_on_adsorbate_only."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("stepper_ode8.npz")
    tr = DenoisingTrainer(_stepper_model(fx), device=DEV)
    outs = []
    for inc, ads_only in ((False, False), (True, False), (True, True)):
        b = batch_from_fixture(fx, pos_key="pos_in")
        torch.manual_seed(int(fx["seed"]))
        den = Denoiser(b, DiffTorchCalc(tr), dict(_params(fx), incremental_layers=inc, scores_on_adsorbate_only=ads_only),
                       device=DEV)
        outs.append(den.run().pos.clone())
        assert den.steps_applied == 8
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_static_atom_cache_switch_gives_identical_samples():
    """denoising_pos_params["static_atom_cache"]=False recomputes everything every step: same positions."""
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.trainer import DenoisingTrainer

    fx = load_npz("stepper_ode8.npz")
    tr = DenoisingTrainer(_stepper_model(fx), device=DEV)
    outs = []
    for flag in (True, False):
        b = batch_from_fixture(fx, pos_key="pos_in")
        torch.manual_seed(int(fx["seed"]))
        den = Denoiser(b, DiffTorchCalc(tr), dict(_params(fx), static_atom_cache=flag), device=DEV)
        outs.append(den.run().pos.clone())
    assert torch.equal(outs[0], outs[1])
