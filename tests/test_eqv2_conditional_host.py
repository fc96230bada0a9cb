"""Host-side tests of the conditional EquiformerV2 denoiser (energy_encoding "scalar", the model of
configs/denoising/eqv2_conditional.yml): construction, parameter layout against the reference's (recorded in
tests/golden/eqv2_conditional_l4.npz by tools/make_golden_eqv2_conditional.py), checkpoint ingest."""
import pytest
import torch

from adsorbdiff_amd.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos as M
from tests.helpers import CFG4_KW, load_npz

YAML_KW = dict(CFG4_KW, lmax_list=[4])   # the shipped conditional config: L = 4 / M = 2, C = 128, 8 blocks
SMALL_KW = dict(max_neighbors=20, max_radius=6.0, max_num_elements=90, num_layers=1, sphere_channels=8,
                attn_hidden_channels=8, num_heads=2, attn_alpha_channels=4, attn_value_channels=4, ffn_hidden_channels=16,
                norm_type="layer_norm_sh", lmax_list=[4], mmax_list=[2], grid_resolution=18, edge_channels=8,
                num_distance_basis=16, attn_activation="silu", ffn_activation="silu", use_grid_mlp=True,
                use_sep_s2_act=True, weight_init="uniform", FOR_denoising=True)


def test_constructor_accepts_scalar_and_rejects_other_encodings():
    m = M(None, None, None, energy_encoding="scalar", **SMALL_KW)
    assert tuple(m.energy_embedding.weight.shape) == (8, 1) and tuple(m.energy_embedding.bias.shape) == (8,)
    assert torch.count_nonzero(m.energy_embedding.bias) == 0   # the reference's _init_weights zeroes it
    for bad in ("vector", "one_hot", "", 1):
        with pytest.raises(ValueError, match="energy_encoding"):
            M(None, None, None, energy_encoding=bad, **SMALL_KW)


def test_sampling_flag_is_kept():
    assert M(None, None, None, energy_encoding="scalar", sampling=True, **SMALL_KW).sampling is True
    assert M(None, None, None, energy_encoding="scalar", **SMALL_KW).sampling is False


def test_normal_init_draws_the_energy_weight_from_a_unit_normal():
    torch.manual_seed(0)
    m = M(None, None, None, energy_encoding="scalar", **dict(SMALL_KW, sphere_channels=512, weight_init="normal"))
    w = m.energy_embedding.weight.detach()
    assert 0.85 < float(w.std()) < 1.15 and float(w.abs().max()) > 1.5   # N(0, 1 / sqrt(in_features = 1))


def test_parameter_names_order_and_shapes_equal_the_reference():
    fx = load_npz("eqv2_conditional_l4.npz")
    m = M(None, None, None, energy_encoding="scalar", **YAML_KW)
    got = [(k, ",".join(map(str, p.shape))) for k, p in m.named_parameters()]
    want = list(zip([s.decode() for s in fx["param_names"]], [s.decode() for s in fx["param_shapes"]]))
    assert got == want
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    names = [k for k, _ in got]
    assert names.index("energy_embedding.weight") == names.index("force_block2.alpha_dot") - 2


def test_unconditional_model_has_no_energy_embedding():
    m = M(None, None, None, **SMALL_KW)
    assert not hasattr(m, "energy_embedding")
    assert not any(k.startswith("energy_embedding") for k in m.state_dict())


def test_reference_layout_checkpoint_loads_under_strict(tmp_path):
    """A checkpoint as the reference's trainer writes it (base_trainer.py): `module.` prefixed state_dict with the
    constant buffers, an `ema` with shadow parameters in parameter order, and the conditional model's `config`."""
    from adsorbdiff_amd.trainer import DenoisingTrainer

    cfg = dict(SMALL_KW, energy_encoding="scalar", so3_denoising=True)
    torch.manual_seed(1)
    src = M(None, None, None, **cfg)
    with torch.no_grad():
        src.energy_embedding.weight.normal_()
        src.energy_embedding.bias.normal_()
    sd = {"module." + k: v.clone() for k, v in src.state_dict().items()}
    sd["module.SO3_grid.4.2.to_grid_mat"] = torch.zeros(3)
    sd["module.distance_expansion.offset"] = torch.zeros(16)
    shadow = [p.detach().clone() + 0.25 for p in src.parameters() if p.requires_grad]
    ckpt = {"state_dict": sd, "ema": {"decay": 0.999, "num_updates": 7, "shadow_params": shadow},
            "config": {"model": "EquiformerV2S_OC20_DenoisingPos", "model_attributes": cfg}, "epoch": 3, "step": 70}

    dst = M(None, None, None, **ckpt["config"]["model_attributes"])
    clean = {k[len("module."):]: v for k, v in ckpt["state_dict"].items()}
    res = dst.load_state_dict(clean, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.energy_embedding.weight, src.energy_embedding.weight)
    assert torch.equal(dst.energy_embedding.bias, src.energy_embedding.bias)

    path = tmp_path / "checkpoint.pt"
    torch.save(ckpt, path)
    dst2 = M(None, None, None, **cfg)
    DenoisingTrainer(dst2, device="cpu").load_checkpoint(str(path))
    got = [p for p in dst2.parameters() if p.requires_grad]
    assert len(got) == len(shadow) and all(torch.equal(a, b) for a, b in zip(got, shadow))
    # the conditional checkpoint still refuses to load into the unconditional model under strict
    with pytest.raises(RuntimeError, match="unexpected"):
        M(None, None, None, **SMALL_KW).load_state_dict(clean)


def test_no_weight_decay_lists_the_energy_bias():
    m = M(None, None, None, energy_encoding="scalar", **SMALL_KW)
    nwd = m.no_weight_decay()
    assert "energy_embedding.bias" in nwd and "energy_embedding.weight" not in nwd


def test_shard_batch_carries_energy():
    from adsorbdiff_amd.sampler import shard_batch
    from adsorbdiff_amd.synthetic import make_batch

    b = make_batch(8, n_slab=12, n_ads=2, seed=3)
    b.energy = torch.arange(8, dtype=torch.float32) * 0.37 - 1.1
    seen = {}
    for r in range(3):
        sub, ids = shard_batch(b, r, 3)
        assert sub is not None and len(ids) == int(sub.natoms.numel())
        assert torch.equal(sub.energy, b.energy[ids])
        seen.update({i: float(e) for i, e in zip(ids, sub.energy)})
    assert sorted(seen) == list(range(8))
