"""CPU tests of the EquiformerV2 S2EF mirror (adsorbdiff_amd.equiformer_v2_oc20): parameter names / shapes / seeded values
against what tools/make_golden_eqv2_s2ef.py recorded from the reference class, state_dict loading, the configuration
checks, the library's weight table and the way ml_relax reaches the model."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import equiformer_v2_denoising as ED
from adsorbdiff_amd import ml_relaxation as MR
from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20
from adsorbdiff_amd.eqv2_engine import ENERGY_HEAD_NAMES, s2ef_weight_names, weight_names
from adsorbdiff_amd.synthetic import make_batch
from adsorbdiff_amd.trainer import ForcesTrainer
from tests.helpers_s2ef import FULL_KW, SMALL_KW, check_keys_shapes_sums, full_model, s2ef_fixture, small_model

DEAD = ("energy_block.so3_linear_1.", "energy_block.grid_mlp.")   # never reach the energy (module docstring)


def test_seeded_small_model_holds_the_reference_weights():
    fx = s2ef_fixture()
    m = small_model()
    check_keys_shapes_sums(m, fx, "small")
    sd = m.state_dict()
    assert "atom_radii" not in sd and "energy_lin_ref" in sd
    assert not any(k.startswith(("force_block2.", "energy_embedding.")) for k in sd)


def test_full_width_model_holds_the_reference_weights():
    check_keys_shapes_sums(full_model(), s2ef_fixture(), "full")


def test_it_is_not_a_denoiser_and_shares_the_containers():
    m = small_model()
    assert isinstance(m, ED.EqV2Host) and not isinstance(m, ED.EquiformerV2S_OC20_DenoisingPos)
    assert m.so3_denoising is False and not hasattr(m, "sample") and not hasattr(m, "atom_radii")
    assert isinstance(m.blocks[0], ED.TransBlockV2) and isinstance(m.force_block, ED.SO2EquivariantGraphAttention)
    assert m.num_params == sum(p.numel() for p in m.parameters())
    assert "energy_block.so3_linear_2.bias" in m.no_weight_decay()


def test_construction_mode_does_not_leak_into_the_denoiser_mirror():
    kw = {k: v for k, v in SMALL_KW.items() if k != "load_energy_lin_ref"}
    torch.manual_seed(1)
    a = ED.EquiformerV2S_OC20_DenoisingPos(None, None, None, FOR_denoising=True, **kw)
    small_model()
    torch.manual_seed(1)
    b = ED.EquiformerV2S_OC20_DenoisingPos(None, None, None, FOR_denoising=True, **kw)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) or k == "atom_radii" for k in sa)
    assert ED._REFERENCE_CONSTRUCTION is False


def test_energy_only_model_has_no_force_block():
    m = small_model(regress_forces=False)
    assert not hasattr(m, "force_block") and not any(k.startswith("force_block") for k in m.state_dict())


def test_dead_energy_block_parameters_load_under_strict():
    src, dst = small_model(), small_model()
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    dead = [k for k in sd if k.startswith(DEAD) or k == "energy_block.so3_linear_2.weight"]
    assert len(dead) == 6
    for k in dead:
        sd[k] = sd[k] + 1.0
    # a reference checkpoint also carries constant buffers: accepted and ignored
    sd["blocks.0.ga.proj.expand_index"] = torch.zeros(25, dtype=torch.long)
    sd["energy_block.so3_linear_2.expand_index"] = torch.zeros(25, dtype=torch.long)
    sd["SO3_grid.4.2.to_grid_mat"] = torch.zeros(3, 3)
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(dst.state_dict()[k], sd[k]) for k in dead)
    for extra in ("atom_radii", "force_block2.alpha_dot", "energy_embedding.weight"):
        with pytest.raises(RuntimeError, match="unexpected"):
            dst.load_state_dict(dict(sd, **{extra: torch.zeros(1)}), strict=True)
    with pytest.raises(RuntimeError, match="missing"):
        dst.load_state_dict({k: v for k, v in sd.items() if k != "energy_lin_ref"}, strict=True)
    with pytest.raises(RuntimeError, match="size mismatch"):
        dst.load_state_dict(dict(sd, **{"energy_block.so3_linear_2.bias": torch.zeros(2)}), strict=True)


@pytest.mark.parametrize("kw", [
    dict(use_pbc=False), dict(otf_graph=False), dict(use_energy_lin_ref=True, load_energy_lin_ref=False),
    dict(mmax_list=[3]), dict(lmax_list=[4, 2], mmax_list=[2, 2]), dict(norm_type="rms_norm_sh"),
    dict(attn_activation="scaled_silu"), dict(use_gate_act=True), dict(use_grid_mlp=False), dict(use_sep_s2_act=False),
    dict(share_atom_edge_embedding=True), dict(use_m_share_rad=True), dict(grid_resolution=None),
    dict(distance_function="sigmoid"), dict(weight_init="xavier"), dict(enforce_max_neighbors_strictly=False),
])
def test_unsupported_configurations_raise(kw):
    with pytest.raises(ValueError):
        EquiformerV2_OC20(None, None, None, **dict(SMALL_KW, **kw))


def test_reference_defaults_of_the_signature():
    import inspect

    p = inspect.signature(EquiformerV2_OC20.__init__).parameters
    assert [p[k].default for k in ("avg_num_nodes", "avg_degree", "use_energy_lin_ref", "load_energy_lin_ref",
                                   "regress_forces", "max_num_elements")] == [None, None, False, False, True, 90]
    m = EquiformerV2_OC20(None, None, None, **dict(SMALL_KW, avg_num_nodes=50.0, avg_degree=12.5))
    assert (m.avg_num_nodes, m.avg_degree) == (50.0, 12.5)
    assert small_model().avg_num_nodes == pytest.approx(77.81317)


def test_forward_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        small_model()(make_batch(1, n_slab=16, n_ads=2, seed=1))


@pytest.mark.parametrize("kw,layers", [(SMALL_KW, 2), (FULL_KW, 8)])
def test_weight_table_covers_every_live_parameter_exactly_once(kw, layers):
    m = EquiformerV2_OC20(None, None, None, **dict(kw, num_layers=layers))
    table = s2ef_weight_names(layers, 2) + ENERGY_HEAD_NAMES
    assert len(table) == len(set(table))
    live = [k for k, _ in m.named_parameters() if not k.startswith(DEAD) and k != "energy_lin_ref"]
    assert sorted(table) == sorted(live)
    # the denoiser's table keeps its layout: the S2EF table is that table without the radii and the second force block
    den = weight_names(layers, 2)
    assert den[0] == "atom_radii" and [n for n in den[1:] if not n.startswith("force_block2.")] == s2ef_weight_names(layers, 2)


def test_ml_relax_reaches_the_model_through_forces_trainer(monkeypatch):
    """ForcesTrainer / TorchCalc / ml_relax are model-agnostic: with the engine replaced by a recorder, a relaxation's
    optimizer (stubbed: the device L-BFGS needs a GPU) gets the model's energy and forces through trainer.predict."""
    m = small_model()
    calls = []

    class FakeEngine:
        device = torch.device("cpu")

        def forward_energy(self, data):
            calls.append(int(data.pos.shape[0]))
            return torch.arange(len(data.natoms), dtype=torch.float32), data.pos * 2.0

    monkeypatch.setattr(EquiformerV2_OC20, "engine", lambda self, device=None: FakeEngine())
    tr = ForcesTrainer(m, device="cpu", normalizers={"target": {"mean": 1.0, "stdev": 2.0}})
    assert tr._unwrapped_model is m and m.otf_graph

    class StubLBFGS:
        def __init__(self, batch, calc, **kw):
            self.batch, self.calc = batch, calc

        def run(self, fmax, steps):
            e, f = self.calc.get_energy_and_forces(self.batch, apply_constraint=True)
            self.batch.y, self.batch.force = e, f
            return self.batch

    monkeypatch.setattr(MR, "LBFGS", StubLBFGS)
    b = make_batch(2, n_slab=4, n_ads=1, seed=3)
    out = MR.ml_relax(b, model=tr, steps=3, fmax=0.05, relax_opt={"memory": 5}, save_full_traj=False, device="cpu")
    assert calls == [10]
    assert torch.equal(out.y, torch.tensor([1.0, 3.0]))            # denormalised energies
    free = (b.fixed == 0)
    assert torch.equal(out.force[free], b.pos[free] * 2.0) and bool((out.force[~free] == 0).all())
    m2 = small_model(regress_forces=False)
    monkeypatch.setattr(EquiformerV2_OC20, "engine", lambda self, device=None: type("E", (), {
        "forward_energy": lambda s, d: (torch.zeros(len(d.natoms)), None)})())
    assert set(m2(b)) == {"energy"}


def test_fixture_energies_are_not_cancellation_noise():
    fx = s2ef_fixture()
    for tag in ("small", "full"):
        batch = torch.from_numpy(fx[f"{tag}_batch"]).long()
        tot = torch.zeros(2).index_add_(0, batch, torch.from_numpy(fx[f"{tag}_atom_energy"]).abs()) / 77.81317
        assert np.all(np.abs(fx[f"{tag}_energy"]) >= 0.1 * tot.numpy())
