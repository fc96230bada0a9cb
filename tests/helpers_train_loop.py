"""What the tests of the training loop share (tests/test_train_loop_host.py, test_gpu_optimizer_multi.py,
test_gpu_train_loop.py): small host models, the synthetic module of the optimizer tests, the float64 mirror of
AdamW + clip + EMA, and the batches and configurations of the resume runs."""
import copy

import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.synthetic import make_system
from adsorbdiff_amd.train_loop import TrainLoopMixin

NOISE = dict(ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55)


# ------------------------------------------------------------------------------------------------ host
class FiveTensors(torch.nn.Module):
    """Five parameter tensors; ``d`` never receives a gradient; ``b`` and ``e`` are named by no_weight_decay()."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(4, 3, generator=g))
        self.b = torch.nn.Parameter(torch.randn(3, generator=g))
        self.c = torch.nn.Parameter(torch.randn(2, 5, generator=g))
        self.d = torch.nn.Parameter(torch.randn(7, generator=g))
        self.e = torch.nn.Parameter(torch.randn(1, generator=g))

    def no_weight_decay(self):
        return {"b", "e"}

    def loss(self, k):
        return (self.a.sum() * (k + 1)) ** 2 + (self.b ** 2).sum() + self.c.sin().sum() * self.e.sum()


class HostTrainer(TrainLoopMixin):
    """The attributes ``TrainLoopMixin`` reads, on the CPU with torch's own AdamW."""

    name = "ocp"

    def __init__(self, directory, eval_metrics=None):
        from adsorbdiff_amd.exponential_moving_average import ExponentialMovingAverage
        from adsorbdiff_amd.train_step import reference_param_groups

        self.device = torch.device("cpu")
        self.model = FiveTensors()
        self.optimizer = torch.optim.AdamW(reference_param_groups(self.model, 0.01), lr=1e-3)
        self.ema = ExponentialMovingAverage(self.model.parameters(), 0.99)
        self.config = {"cmd": {"checkpoint_dir": str(directory)}, "optim": {"max_epochs": 2},
                       "eval_metrics": eval_metrics or {"primary_metric": "loss"}}
        self.scheduler = None
        self.step, self.epoch, self.noise_step = 3, 0.75, 11
        self.best_val_metric = 0.5

    @property
    def _unwrapped_model(self):
        return self.model


# ------------------------------------------------------------------------------------------------ optimizer on the device
class Synthetic(torch.nn.Module):
    """Tensors of 1, 63, 64, 65, 257, L-1, L, L+1 and 2L+3 elements.  ``p65`` sits one element into its buffer (its pointer
    is not 16-byte aligned), ``p63`` is named by no_weight_decay(), ``p257`` never receives a gradient."""

    SIZES = ("1", "63", "64", "65", "257", "Lm1", "L", "Lp1", "2Lp3")

    def __init__(self, L, device, extra=0):
        super().__init__()
        g = torch.Generator().manual_seed(17)
        sizes = dict(zip(self.SIZES, (1, 63, 64, 65, 257, L - 1, L, L + 1, 2 * L + 3)))
        for name, n in sizes.items():
            if name == "65":
                buf = torch.randn(n + 1, generator=g).to(device)
                p = torch.nn.Parameter(buf[1:])
                assert p.data_ptr() % 16 != 0
            else:
                p = torch.nn.Parameter(torch.randn(n, generator=g).to(device))
            self.register_parameter("p" + name, p)
        for k in range(extra):   # tensors that never receive a gradient, registered after the others
            self.register_parameter(f"x{k}", torch.nn.Parameter(torch.randn(5 + k, generator=g).to(device)))

    def no_weight_decay(self):
        return {"p63"}

    def set_grads(self, seed, scale=1.0, misalign=("p65",)):
        """Seeded gradients; those of ``misalign`` sit one element into their buffer (not 16-byte aligned)."""
        g = torch.Generator().manual_seed(seed)
        for name, p in self.named_parameters():
            if name == "p257" or name.startswith("x"):
                p.grad = None
                continue
            new = (torch.randn(p.shape, generator=g) * scale).to(p.device)
            if p.grad is None:
                if name in misalign:
                    buf = torch.empty(p.numel() + 1, device=p.device)
                    p.grad = buf[1:].view_as(p)
                    assert p.grad.data_ptr() % 16 != 0
                    p.grad.copy_(new)
                else:
                    p.grad = new
            else:
                p.grad.copy_(new)   # the same buffer: the tables need no rebuild


class ManySmall(torch.nn.Module):
    """``n`` tensors of 1 to 7 elements: more chunks than stage 2 of the norm takes in one tile of 256."""

    def __init__(self, n, device):
        super().__init__()
        g = torch.Generator().manual_seed(23)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(1 + k % 7, generator=g).to(device)) for k in range(n)])
        for p in self.ps:
            p.grad = torch.randn(p.shape, generator=g).to(device)


class Float64Mirror:
    """torch.optim.AdamW + clip_grad_norm_ + the EMA in float64 on a copy of a module's parameters."""

    def __init__(self, module, lr, weight_decay, max_norm, ema_decay, betas=(0.9, 0.999), eps=1e-8):
        from adsorbdiff_amd.exponential_moving_average import ExponentialMovingAverage

        self.names = [n for n, _ in module.named_parameters()]
        self.params = [torch.nn.Parameter(p.detach().double().cpu().clone()) for _, p in module.named_parameters()]
        skip = tuple(module.no_weight_decay())
        groups = [{"params": [p for n, p in zip(self.names, self.params) if any(n.endswith(s) for s in skip)], "weight_decay": 0},
                  {"params": [p for n, p in zip(self.names, self.params) if not any(n.endswith(s) for s in skip)],
                   "weight_decay": weight_decay}]
        self.opt = torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps)
        self.max_norm = max_norm
        self.ema = ExponentialMovingAverage(self.params, ema_decay)

    def step(self, module):
        for q, (_, p) in zip(self.params, module.named_parameters()):
            q.grad = p.grad.detach().double().cpu().clone() if p.grad is not None else None
        with_grad = [q for q in self.params if q.grad is not None]
        if self.max_norm:
            norm = torch.nn.utils.clip_grad_norm_(with_grad, max_norm=self.max_norm)
        else:
            norm = torch.sqrt(sum((q.grad ** 2).sum() for q in with_grad))
        self.opt.step()
        self.ema.update(self.params)
        return norm


# ------------------------------------------------------------------------------------------------ runs on the device
def denoising_batches(n=4, seed=900):
    """``n`` small batches of three ragged systems each, on the CPU, with ``pos_relaxed`` as the reference's loaders give it."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        systems = [make_system(g, n_slab, n_ads, sid=f"{i}_{j}") for j, (n_slab, n_ads) in enumerate(((36, 4), (7, 1), (20, 2)))]
        b = Batch.from_data_list(systems)
        b.pos_relaxed = b.pos.clone()   # what the steps noise: the noising replaces batch.pos, and every step starts from here
        out.append(b)
    return out


def s2ef_batches(n=4, seed=900):
    from tests.helpers_s2ef_train import NORMALIZERS

    g = torch.Generator().manual_seed(seed + 1)
    out = []
    for b in denoising_batches(n, seed):
        N, B = int(b.pos.shape[0]), int(b.natoms.numel())
        b.energy = NORMALIZERS["energy"]["mean"] + NORMALIZERS["energy"]["stdev"] * torch.randn(B, generator=g)
        b.forces = NORMALIZERS["forces"]["stdev"] * torch.randn(N, 3, generator=g)
        b.fixed = (torch.rand(N, generator=g) < 0.3).long()
        out.append(b)
    return out


def loop_config(directory, **optim):
    """cosine schedule over 2 epochs of 4 batches, validation at the end of each epoch, primary metric ``loss``."""
    cfg = {"cmd": {"checkpoint_dir": str(directory), "print_every": 100},
           "eval_metrics": {"primary_metric": "loss"},
           "optim": {"max_epochs": 2, "lr_initial": 2e-4, "scheduler": "LambdaLR", "checkpoint_every": 100,
                     "scheduler_params": {"lambda_type": "cosine", "warmup_factor": 0.2, "warmup_epochs": 0.5,
                                          "lr_min_factor": 0.01}}}
    cfg["optim"].update(optim)
    return cfg


def make_trainer(kind, directory, dev, **optim):
    """A fresh model and trainer of ``kind`` ("denoising" / "s2ef"), set up reproducibly with the loop configuration."""
    from adsorbdiff_amd.so3_tables import Igso3Tables   # the full tables: the device noising samples rotations from them
    from adsorbdiff_amd.trainer import DenoisingTrainer, ForcesTrainer
    from tests import helpers_s2ef_train as HS
    from tests import helpers_train as HT

    cfg = loop_config(directory, **optim)
    if kind == "denoising":
        tr = DenoisingTrainer(HT.make_config_model("ragged"), device=dev, config=cfg)
        tr.setup_training(NOISE, lr=2e-4, weight_decay=0.001, clip_grad_norm=100.0, ema_decay=0.999,
                          tables=Igso3Tables.shared(), noise_on_device=True, noise_seed=5, reproducible=True)
    else:
        tr = ForcesTrainer(HS.make_config_model("ragged"), device=dev, normalizers=copy.deepcopy(HS.NORMALIZERS), config=cfg)
        tr.setup_training(lr=2e-4, weight_decay=0.001, clip_grad_norm=10.0, ema_decay=0.999, reproducible=True,
                          **HS.COEFFICIENTS)
    return tr


def batches_for(kind, dev):
    return [b.to(dev) for b in (denoising_batches() if kind == "denoising" else s2ef_batches())]


def training_state(tr):
    """Everything a resumed run must reproduce, as CPU tensors / numbers."""
    sd = tr.optimizer.state_dict()
    out = {"step": tr.step, "lr": tr.optimizer.param_groups[0]["lr"], "noise_step": getattr(tr, "noise_step", 0),
           "best_val_metric": tr.best_val_metric, "applied": int(next(iter(sd["state"].values()))["step"])}
    for k, p in tr._unwrapped_model.named_parameters():
        out["p::" + k] = p.detach().cpu().clone()
    for i, e in sd["state"].items():
        out[f"m::{i}"], out[f"v::{i}"] = e["exp_avg"].cpu().clone(), e["exp_avg_sq"].cpu().clone()
    for i, s in enumerate(tr.ema.shadow_params):
        out[f"ema::{i}"] = s.cpu().clone()
    return out


def assert_same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
