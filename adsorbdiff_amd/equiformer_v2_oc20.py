"""EquiformerV2 S2EF force field — host-side mirror of the reference module
``adsorbdiff.models.equiformer_v2.equiformer_v2_oc20.EquiformerV2_OC20`` (registered there as ``"equiformer_v2"``;
reference: models/equiformer_v2/equiformer_v2_oc20.py:67-562), the force field that matches the EquiformerV2 denoiser and
that ``ml_relax`` can drive.

It is the denoiser (``equiformer_v2_denoising.EquiformerV2S_OC20_DenoisingPos``) with four differences
(equiformer_v2_oc20.py:415-562 against equiformer_v2_denoising.py:186-318): no ``tag_based_Z``; **no atomic radii** - the
edge distances enter the Gaussian basis as they are, so the basis is live on every edge (the denoiser's is identically
zero) and the radial functions are evaluated per edge; an energy output - ``energy_block`` on the final-normed
embedding, l = 0 coefficient, summed per system, divided by ``avg_num_nodes``, plus ``energy_lin_ref[Z]`` with
``use_energy_lin_ref``; one force block.  Same constructor signature as the reference, same ``state_dict`` keys and
shapes (no ``atom_radii``, no ``force_block2``, no ``energy_embedding``; ``energy_lin_ref`` with ``load_energy_lin_ref``)
and the same consumption of the global random generator, so ``torch.manual_seed(s); EquiformerV2_OC20(...)`` draws the
reference's weights.  ``forward(data) -> {"energy": [B], "forces": [N, 3]}`` (``{"energy"}`` alone with
``regress_forces=False``; the force block is then not evaluated).

The sub-modules are the denoiser mirror's parameter containers (shared through ``EqV2Host``, the common base of both
mirrors; this class is not a denoiser and has no sampler entry points); ``forward`` runs in the HIP library
(``adf_eqv2_set_weights_s2ef`` / ``adf_eqv2_set_energy_head`` / ``adf_eqv2_forward_energy``).  There is no CPU / eager
fallback.  With the shipped switches (``use_grid_mlp``, ``use_sep_s2_act``) only the gating scalars of ``energy_block``
reach the energy (transformer_block.py:473-530): ``so3_linear_1``, ``grid_mlp.*`` and the l > 0 slices of
``so3_linear_2.weight`` are dead parameters; they exist and load, the library reads ``scalar_mlp.0`` and row 0 of
``so3_linear_2.weight[0]`` only.

Forces come in two ways, chosen by ``force_mode`` (as ``painn.PaiNN``): ``"direct"`` (default) returns the force block's
output as before; ``"energy_gradient"`` returns ``-dE/dpos`` of the energy the same call reports, with the edge set held
fixed - what ``torch.autograd.grad(energy.sum(), pos)`` gives on the reference model with a frozen graph
(``EqV2Engine.forward_energy_gradient``, ``eqv2_train_step.EqV2EnergyGradient``, csrc/eqv2_geo.hip).  It works
with ``regress_forces=False``: the force block is neither needed nor evaluated.  The energy that mode reports is the energy
of the graph it differentiates - the exact-f32 training forward in ``eval()``, no dropout - which lies within 1.3e-6 of
max|E| of the direct mode's (whose products run in f16x3).  Training with it needs a second-order backward and is refused.

Supported configuration: what the denoiser mirror accepts, with ``use_pbc = otf_graph = True`` and ``mmax_list = [m]``,
m <= 2 (no kernel of this library has been run against a reference at m = 3); anything else raises ``ValueError``.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import equiformer_v2_denoising as _ed

_AVG_NUM_NODES = 77.81317
_AVG_DEGREE = 23.395238876342773  # equiformer_v2_oc20.py:54-57 (IS2RE: 100k, max_radius = 5, max_neighbors = 100)


class EquiformerV2_OC20(_ed.EqV2Host):
    """See module docstring.  ``num_atoms, bond_feat_dim, num_targets`` are accepted and ignored like the reference."""

    s2ef = True           # EqV2Engine binds the S2EF table and the energy head and offers forward_energy
    so3_denoising = False
    FORCE_MODES = ("direct", "energy_gradient")

    def __init__(
        self,
        num_atoms=None, bond_feat_dim=None, num_targets=None,
        use_pbc=True, regress_forces=True, otf_graph=True, max_neighbors=500, max_radius=5.0, max_num_elements=90,
        num_layers=12, sphere_channels=128, attn_hidden_channels=128, num_heads=8, attn_alpha_channels=32,
        attn_value_channels=16, ffn_hidden_channels=512, norm_type="rms_norm_sh", lmax_list=[6], mmax_list=[2],
        grid_resolution=None, num_sphere_samples=128, edge_channels=128, use_atom_edge_embedding=True,
        share_atom_edge_embedding=False, use_m_share_rad=False, distance_function="gaussian", num_distance_basis=512,
        attn_activation="scaled_silu", use_s2_act_attn=False, use_attn_renorm=True, ffn_activation="scaled_silu",
        use_gate_act=False, use_grid_mlp=False, use_sep_s2_act=True, alpha_drop=0.1, drop_path_rate=0.05, proj_drop=0.0,
        weight_init="normal", enforce_max_neighbors_strictly=True, avg_num_nodes=None, avg_degree=None,
        use_energy_lin_ref=False, load_energy_lin_ref=False,
    ) -> None:
        super().__init__()
        bad = _ed.unsupported_configuration(lmax_list, mmax_list, norm_type, attn_activation, ffn_activation, use_s2_act_attn,
                                            use_attn_renorm, use_gate_act, use_grid_mlp, use_sep_s2_act,
                                            use_atom_edge_embedding, share_atom_edge_embedding, use_m_share_rad,
                                            distance_function, grid_resolution, weight_init)
        if not (use_pbc and otf_graph and enforce_max_neighbors_strictly):
            bad.append("use_pbc = otf_graph = enforce_max_neighbors_strictly = True")
        if len(mmax_list) == 1 and mmax_list[0] > 2:
            bad.append("mmax_list[0] <= 2 (no kernel has been checked against the reference at m = 3)")
        if use_energy_lin_ref and not load_energy_lin_ref:
            bad.append("load_energy_lin_ref=True with use_energy_lin_ref=True (the model would have no reference table)")
        if bad:
            raise ValueError("the HIP EquiformerV2 path implements the shipped configuration only; needs " + "; ".join(bad))
        self.use_pbc, self.regress_forces, self.otf_graph = use_pbc, regress_forces, otf_graph
        self.direct_forces = True
        self.max_neighbors, self.max_radius, self.cutoff = max_neighbors, max_radius, max_radius
        self.max_num_elements, self.num_layers, self.sphere_channels = max_num_elements, num_layers, sphere_channels
        self.attn_hidden_channels, self.num_heads = attn_hidden_channels, num_heads
        self.attn_alpha_channels, self.attn_value_channels = attn_alpha_channels, attn_value_channels
        self.ffn_hidden_channels, self.norm_type = ffn_hidden_channels, norm_type
        self.lmax_list, self.mmax_list, self.grid_resolution = list(lmax_list), list(mmax_list), grid_resolution
        self.edge_channels, self.num_distance_basis = edge_channels, num_distance_basis
        self.weight_init = weight_init
        # read by the training step alone (eqv2_train_step.EqV2S2EFTrainStep); the inference forward has no dropout
        self.alpha_drop, self.drop_path_rate, self.proj_drop = float(alpha_drop), float(drop_path_rate), float(proj_drop)
        self.avg_num_nodes = avg_num_nodes or _AVG_NUM_NODES
        self.avg_degree = avg_degree or _AVG_DEGREE
        self.use_energy_lin_ref, self.load_energy_lin_ref = use_energy_lin_ref, load_energy_lin_ref
        self.enforce_max_neighbors_strictly = enforce_max_neighbors_strictly
        lmax, mmax = self.lmax_list[0], self.mmax_list[0]
        ecl = [self.NUM_GAUSSIANS, edge_channels, edge_channels]
        self.edge_channels_list = ecl

        with _ed.reference_construction():   # the reference constructors' draws only; its two passes follow
            self.sphere_embedding = nn.Embedding(max_num_elements, sphere_channels)
            self.edge_degree_embedding = _ed.EdgeDegreeEmbedding(sphere_channels, lmax, max_num_elements, ecl)
            self.blocks = nn.ModuleList([
                _ed.TransBlockV2(sphere_channels, attn_hidden_channels, num_heads, attn_alpha_channels, attn_value_channels,
                                 ffn_hidden_channels, lmax, mmax, max_num_elements, ecl, False)
                for _ in range(num_layers)])
            self.norm = _ed.EquivariantLayerNormArraySphericalHarmonics(lmax, sphere_channels)
            self.energy_block = _ed.FeedForwardNetwork(sphere_channels, ffn_hidden_channels, 1, lmax, False)
            if regress_forces:
                self.force_block = _ed.SO2EquivariantGraphAttention(sphere_channels, attn_hidden_channels, num_heads,
                                                                    attn_alpha_channels, attn_value_channels, 1, lmax, mmax,
                                                                    max_num_elements, ecl, False)
        if load_energy_lin_ref:
            self.energy_lin_ref = nn.Parameter(torch.zeros(max_num_elements), requires_grad=False)
        self.apply(self._init_weights)                            # equiformer_v2_oc20.py:411, 572-582
        self.apply(self._uniform_init_rad_func_linear_weights)    # :412, 584-593
        self._engine = None
        self._engine_key = None
        self._force_mode = "direct"

    @property
    def force_mode(self) -> str:
        """``"direct"``: forces from the force block; ``"energy_gradient"``: forces = -dE/dpos of the reported energy."""
        return self._force_mode

    @force_mode.setter
    def force_mode(self, mode: str) -> None:
        if mode not in self.FORCE_MODES:
            raise ValueError(f"force_mode must be one of {self.FORCE_MODES}, got {mode!r}")
        self._force_mode = mode

    def _init_weights(self, m) -> None:
        if isinstance(m, (nn.Linear, _ed.SO3_LinearV2)):
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
            if self.weight_init == "normal":
                nn.init.normal_(m.weight, 0, 1 / math.sqrt(m.in_features))
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @staticmethod
    def _uniform_init_rad_func_linear_weights(m) -> None:
        if isinstance(m, _ed.RadialFunction):
            for lin in m.modules():
                if isinstance(lin, nn.Linear):
                    nn.init.constant_(lin.bias, 0)
                    std = 1 / math.sqrt(lin.in_features)
                    nn.init.uniform_(lin.weight, -std, std)

    def forward(self, data):
        """data: pos [N,3] f32, atomic_numbers [N], batch [N], natoms [B], cell [B,3,3]
        -> {"energy": [B], "forces": [N,3]} ({"energy"} only with regress_forces=False and force_mode "direct")."""
        if self._force_mode == "energy_gradient":
            # the graph and the constant tables come from the handle, the weights are read where they live
            energy, forces = self.engine(data.pos.device, refresh=False).forward_energy_gradient(data)
            return {"energy": energy, "forces": forces}
        eng = self.engine(data.pos.device)
        energy, forces = eng.forward_energy(data)
        out = {"energy": energy}
        if self.regress_forces:
            out["forces"] = forces
        return out
