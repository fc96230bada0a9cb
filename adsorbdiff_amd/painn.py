"""OCP PaiNN S2EF force field — host-side mirror of the reference module ``adsorbdiff.models.painn.painn.PaiNN``
(registered as ``"painn"``, reference: adsorbdiff/models/painn/painn.py:52-432), the machine-learned force field that
``ml_relax`` drives.

It is the denoiser (``painn_denoising.PaiNN``) with three differences: no ``tag_based_Z``, edge distances floored at 1e-6
instead of 1e-3 (painn.py:334-335), and a real energy head ``out_energy`` = Linear(H, H/2), ScaledSiLU, Linear(H/2, 1)
summed per system (painn.py:412-414) next to one direct-force ``PaiNNOutput`` head.  Same constructor arguments and
``state_dict`` keys / shapes as the reference (no ``atom_radii``, no ``out_forces2``), and the same construction order, so
``torch.manual_seed(s); PaiNN(...)`` draws the reference's weights.  The sub-modules are parameter containers; ``forward``
runs in the HIP library through the denoiser's engine (``engine.PaiNNEngine``, shared through ``PaiNNHost``, the common
base of both mirrors; this class is not a denoiser) with one force head plus the energy head
(``adf_painn_forward_energy``).  There is no eager / CPU fallback.

Forces come in two ways, chosen by ``force_mode``: ``"direct"`` (default) returns the force head's output as before;
``"energy_gradient"`` returns ``-dE/dpos`` of the energy the same call reports (``adf_painn_forward_energy_gradient``; what
``torch.autograd.grad(out["energy"].sum(), pos)`` gives on the reference with the edge set held fixed).  The second works
without a force head (``regress_forces=False``).  It is not the reference's ``direct_forces=False`` branch
(painn.py:421-429), which differentiates the sum of the last node embedding instead of the energy: the constructor keeps
rejecting that.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Union

import torch
from torch import nn

from . import painn_denoising as _pd
from .scaling import ScaleFactor, load_scales_compat


class PaiNN(_pd.PaiNNHost):
    """See module docstring.  ``num_atoms, bond_feat_dim, num_targets`` are accepted and ignored like the reference."""

    distance_floor = 1.0e-6   # painn.py:334-335 (the denoiser: 1e-3)
    energy_head = True        # PaiNNEngine binds out_energy and offers forward_energy
    FORCE_MODES = ("direct", "energy_gradient")

    def __init__(
        self,
        num_atoms: Optional[int] = None,
        bond_feat_dim: Optional[int] = None,
        num_targets: Optional[int] = None,
        hidden_channels: int = 512,
        num_layers: int = 6,
        num_rbf: int = 128,
        cutoff: float = 12.0,
        max_neighbors: int = 50,
        rbf: Dict[str, str] = {"name": "gaussian"},
        envelope: Dict[str, Union[str, int]] = {"name": "polynomial", "exponent": 5},
        regress_forces: bool = True,
        direct_forces: bool = True,
        use_pbc: bool = True,
        otf_graph: bool = True,
        num_elements: int = 83,
        scale_file: Optional[str] = None,
    ) -> None:
        super().__init__()
        self.num_atoms, self.bond_feat_dim, self.num_targets = num_atoms, bond_feat_dim, num_targets
        self.hidden_channels = hidden_channels
        self.num_layers = num_layers
        self.num_rbf = num_rbf
        self.cutoff = cutoff
        self.max_neighbors = max_neighbors
        self.regress_forces = regress_forces
        self.direct_forces = direct_forces
        self.otf_graph = otf_graph
        self.use_pbc = use_pbc
        self.num_elements = num_elements
        self.so3_denoising = False
        self.symmetric_edge_symmetrization = False
        if regress_forces and not direct_forces:
            raise ValueError("forces as the gradient of the energy (direct_forces=False) are not offered on the HIP path")
        if not (use_pbc and otf_graph):
            raise ValueError("the HIP path builds the periodic graph on the fly (use_pbc=otf_graph=True)")
        self.num_force_heads = 1 if regress_forces else 0

        self.atom_emb = _pd.AtomEmbedding(hidden_channels, num_elements)
        self.radial_basis = _pd.RadialBasis(num_rbf, cutoff, dict(rbf), dict(envelope))
        self.message_layers = nn.ModuleList()
        self.update_layers = nn.ModuleList()
        for i in range(num_layers):
            self.message_layers.append(_pd.PaiNNMessage(hidden_channels, num_rbf))
            self.update_layers.append(_pd.PaiNNUpdate(hidden_channels))
            setattr(self, "upd_out_scalar_scale_%d" % i, ScaleFactor())
        self.out_energy = nn.Sequential(
            nn.Linear(hidden_channels, hidden_channels // 2),
            _pd.ScaledSiLU(),
            nn.Linear(hidden_channels // 2, 1),
        )
        if regress_forces:
            self.out_forces = _pd.PaiNNOutput(hidden_channels)
        self.inv_sqrt_2 = 1 / math.sqrt(2.0)
        for lin in (self.out_energy[0], self.out_energy[2]):   # painn.py:132-136 (reset_parameters)
            nn.init.xavier_uniform_(lin.weight)
            lin.bias.data.fill_(0)
        load_scales_compat(self, scale_file)

        self._engine = None
        self._engine_key = None
        self._force_mode = "direct"

    @property
    def force_mode(self) -> str:
        """``"direct"``: forces from the force head; ``"energy_gradient"``: forces = -dE/dpos of the reported energy."""
        return self._force_mode

    @force_mode.setter
    def force_mode(self, mode: str) -> None:
        if mode not in self.FORCE_MODES:
            raise ValueError(f"force_mode must be one of {self.FORCE_MODES}, got {mode!r}")
        self._force_mode = mode

    def forward(self, data):
        """data: pos[N,3] f32, atomic_numbers[N], batch[N], natoms[B], cell[B,3,3]
        -> {"energy": [B], "forces": [N,3]} ({"energy"} only with regress_forces=False in the direct mode)."""
        eng = self.engine(data.pos.device)
        if self._force_mode == "energy_gradient":
            energy, forces = eng.forward_energy_gradient(data)
            return {"energy": energy, "forces": forces}
        energy, forces = eng.forward_energy(data)
        out = {"energy": energy}
        if self.regress_forces:
            out["forces"] = forces
        return out
