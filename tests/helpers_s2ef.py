"""What the fixture generator (tools/make_golden_eqv2_s2ef.py) and the tests of the EquiformerV2 S2EF model share: the
model configurations and the recipe that turns a freshly initialised model into the fixtures' model."""
import torch

from tests.helpers import CFG4_KW, load_npz, refill_parameters_by_name

EMB_SCALE = 300.0
SEED_SMALL = 5
HEAD_SEED = 20251

_SHIPPED = dict(norm_type="layer_norm_sh", grid_resolution=18, attn_activation="silu", ffn_activation="silu",
                use_grid_mlp=True, use_sep_s2_act=True, alpha_drop=0.0, drop_path_rate=0.0, weight_init="uniform",
                load_energy_lin_ref=True)
# every contraction length is a multiple of 32 (the shapes the f16x3 matrix-core kernels take)
SMALL_KW = dict(_SHIPPED, max_neighbors=20, max_radius=6.0, max_num_elements=90, num_layers=2, sphere_channels=32,
                attn_hidden_channels=32, num_heads=2, attn_alpha_channels=16, attn_value_channels=16,
                ffn_hidden_channels=32, lmax_list=[4], mmax_list=[2], edge_channels=32)
# the relaxation fixture's model: a cutoff and a cap under which no neighbour list of its batch is ever truncated
RELAX_KW = dict(SMALL_KW, max_radius=5.0, max_neighbors=64)
FULL_KW = {k: v for k, v in dict(CFG4_KW, lmax_list=[4], load_energy_lin_ref=True).items() if k != "FOR_denoising"}


def trained_like(model, scale_emb=True):
    """Atom edge embeddings lifted from the 1e-3 initialisation (``scale_emb``; refill_parameters_by_name has done it
    already), seeded non-zero biases of the two energy-head layers the energy reaches, a seeded ``energy_lin_ref``."""
    g = torch.Generator().manual_seed(HEAD_SEED)
    with torch.no_grad():
        if scale_emb:
            for n, p in model.named_parameters():
                if n.endswith("source_embedding.weight") or n.endswith("target_embedding.weight"):
                    p.mul_(EMB_SCALE)
        eb = model.energy_block
        eb.scalar_mlp[0].bias.copy_(0.5 * torch.randn(eb.scalar_mlp[0].bias.shape, generator=g))
        eb.so3_linear_2.bias.copy_(0.5 + torch.rand(1, generator=g))
        model.energy_lin_ref.copy_(0.1 * torch.randn(model.energy_lin_ref.shape, generator=g))
    return model


def energy_formula(sd, x_l0):
    """Per-atom energy from the l = 0 row [N, C] of the final-normed embedding: with use_grid_mlp and use_sep_s2_act only
    the gating scalars reach the l = 0 output of energy_block (transformer_block.py:473-530)."""
    hid = torch.nn.functional.silu(x_l0 @ sd["energy_block.scalar_mlp.0.weight"].T + sd["energy_block.scalar_mlp.0.bias"])
    return hid @ sd["energy_block.so3_linear_2.weight"][0, 0] + sd["energy_block.so3_linear_2.bias"][0]


def small_model(kw=None, **over):
    from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20

    torch.manual_seed(SEED_SMALL)
    return trained_like(EquiformerV2_OC20(None, None, None, **dict(kw or SMALL_KW, **over)).eval())


def full_model(**over):
    from adsorbdiff_amd.equiformer_v2_oc20 import EquiformerV2_OC20

    torch.manual_seed(0)
    m = refill_parameters_by_name(EquiformerV2_OC20(None, None, None, **dict(FULL_KW, **over)).eval(), EMB_SCALE)
    return trained_like(m, scale_emb=False)


def tensor_sum(v) -> float:
    """fp64 sum in numpy's fixed pairwise order (torch's sum splits by the thread count of the moment)."""
    import numpy as np

    return float(np.sum(v.detach().double().contiguous().numpy().reshape(-1)))


def check_keys_shapes_sums(model, fx, tag):
    import numpy as np

    sd = dict(model.named_parameters())
    assert [k.encode() for k in sd] == list(fx[f"{tag}_keys"])
    assert [",".join(map(str, v.shape)).encode() for v in sd.values()] == list(fx[f"{tag}_shapes"])
    sums = np.array([tensor_sum(v) for v in sd.values()])
    assert np.array_equal(sums, fx[f"{tag}_sums"])
    assert sum(p.numel() for p in model.parameters()) == int(fx[f"{tag}_n_params"])


def s2ef_fixture():
    return load_npz("eqv2_s2ef.npz")
