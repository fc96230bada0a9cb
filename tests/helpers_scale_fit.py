"""What the scale-fit tests and tools/make_golden_scale_fit.py share: the two small models (drawn from a seed, not stored),
the three ragged batches and the torch stand-in module of the host tests.  tests/golden/scale_fit.npz holds the reference's
results for exactly these."""
import torch
from torch import nn

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.scaling import ScaleFactor
from adsorbdiff_amd.synthetic import make_system
from tests.helpers_train import trained_like_rescale_

HP = dict(hidden_channels=128, num_layers=3, num_rbf=32, cutoff=6.0, max_neighbors=20)
L = HP["num_layers"]
NAMES = ["upd_out_scalar_scale_%d" % i for i in range(L)]
WEIGHT_SEEDS, BIAS_SEED, BATCH_SEED = dict(denoiser=21, s2ef=23), 22, 2326
# (n_slab, n_adsorbate) per system: 9 to 40 atoms, the second batch a single system.  BATCH_SEED is the first from 2323 on
# under which no atom of any batch has an exact distance tie at its 20th neighbour: there the reference's pick depends on
# torch.sort's unstable order (exact ties) and no graph is THE reference's; the generator asserts it.
BATCHES = (((36, 4), (8, 1), (20, 2), (13, 2)), ((30, 3),), ((9, 2), (36, 4), (25, 3)))
PRESET = 0.8            # mode "unfitted": factor 1 is preset to this value
MODELS = ("denoiser", "s2ef")


def make_batches():
    g = torch.Generator().manual_seed(BATCH_SEED)
    out = []
    for i, systems in enumerate(BATCHES):
        out.append(Batch.from_data_list([make_system(g, ns, na, sid=f"{i}.{j}") for j, (ns, na) in enumerate(systems)]))
    return out


def prepare_weights_(model) -> None:
    """Biases and LayerNorm parameters off their constants, then trained-like magnitudes (tests/helpers_train.py)."""
    g = torch.Generator().manual_seed(BIAS_SEED)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if n_.endswith("bias") or "layernorm" in n_:
                p_.add_(0.1 * torch.randn(p_.shape, generator=g))
    trained_like_rescale_(model)


def build_model(kind: str, cls=None, scale_file=None):
    """The model ``kind`` ("denoiser": two heads; "s2ef": energy head + one force head) of class ``cls`` (default: this
    package's mirror; the generator passes the reference's class) with unfitted scale factors unless ``scale_file``."""
    if cls is None:
        if kind == "denoiser":
            from adsorbdiff_amd.painn_denoising import PaiNN as cls
        else:
            from adsorbdiff_amd.painn import PaiNN as cls
    kw = dict(so3_denoising=True) if kind == "denoiser" else {}
    torch.manual_seed(WEIGHT_SEEDS[kind])
    m = cls(None, 50, 1, scale_file=scale_file, **HP, **kw)
    prepare_weights_(m)
    return m.eval()


def weight_sums(model):
    return torch.tensor([float(v.double().sum()) for k, v in model.state_dict().items() if k != "atom_radii"],
                        dtype=torch.float64)


class StandIn(nn.Module):
    """Three Linear + ScaleFactor stages in plain torch: what the host tests fit (the reference's generic loop)."""

    def __init__(self, scale_cls=ScaleFactor, width: int = 24, seed: int = 5) -> None:
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.lins = nn.ModuleList([nn.Linear(width, width) for _ in range(3)])
        with torch.no_grad():
            for k, lin in enumerate(self.lins):
                lin.weight.copy_(torch.randn(width, width, generator=g) * (0.5 + 0.4 * k) / width ** 0.5)
                lin.bias.copy_(0.3 * torch.randn(width, generator=g))
        for k in range(3):
            setattr(self, "scale_%d" % k, scale_cls())

    def forward(self, x):
        for k, lin in enumerate(self.lins):
            x = getattr(self, "scale_%d" % k)(x + torch.tanh(lin(x)))
        return x


def standin_batches(width: int = 24):
    g = torch.Generator().manual_seed(6)
    return [torch.randn(n, width, generator=g) * (1.0 + 0.5 * i) + 0.2 for i, n in enumerate((17, 2, 40, 9))]
