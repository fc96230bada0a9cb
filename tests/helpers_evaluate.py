"""The evaluation metrics restated in plain torch on the inputs the kernels take (csrc/evaluate.hip): normalised predictions
with their normalisers, the ``fixed`` mask and the atoms per system.  tests/test_evaluate_host.py pins this restatement to
the reference's own ``Evaluator`` (tests/golden/evaluator.npz, tools/make_golden_evaluator.py); the GPU tests take the
fixture's inputs, names and bounds from here.

Every function returns ``{name: (total, numel)}`` and, under ``"abs::" + name``, the sum of the absolute per-element terms
(the scale of the float32 rounding bound)."""
import numpy as np
import torch

from tests.helpers import load_npz

S2EF_NAMES = ["energy_mae", "forcesx_mae", "forcesy_mae", "forcesz_mae", "forces_mae", "forces_cosine_similarity",
              "forces_magnitude_error", "energy_forces_within_threshold"]
IS2RS_NAMES = ["positions_average_distance_within_threshold", "positions_mae", "positions_mse"]
IS2RE_NAMES = ["energy_mae", "energy_mse", "energy_within_threshold"]
TASK_NAMES = {"s2ef": S2EF_NAMES, "is2rs": IS2RS_NAMES, "is2re": IS2RE_NAMES}
COUNTING = ("energy_forces_within_threshold", "positions_average_distance_within_threshold", "energy_within_threshold")
BATCHES = ("a", "b")
# Float totals against the reference's float64 totals: |ref32 - ref64| (the reference's own float32 noise on the same inputs)
# + K * 2^-24 * sum |term|.  The worst k measured on the MI355X over every float total of the fixture is 0.709
# (s2ef, first batch, forces_magnitude_error: two rounded norms and a rounded difference per term);
# K is 4 x that.
K_BOUND = 2.84
EPS32 = 2.0 ** -24


def _denorm(x, norm, dtype):
    return x.to(dtype) * torch.tensor(norm[1], dtype=dtype) + torch.tensor(norm[0], dtype=dtype)


def _systems(natoms):
    off = [0] + np.cumsum(np.asarray(natoms, dtype=np.int64)).tolist()
    return list(zip(off[:-1], off[1:]))


def s2ef(e_pred, f_pred, e_tgt, f_tgt, fixed, natoms, norm_energy, norm_forces, free_only=True, dtype=torch.float32):
    e = (e_tgt.to(dtype) - _denorm(e_pred, norm_energy, dtype)).abs()
    f = (f_tgt.to(dtype) - _denorm(f_pred, norm_forces, dtype)).abs()
    p, t = _denorm(f_pred, norm_forces, dtype), f_tgt.to(dtype)
    scope = (fixed == 0) if free_only else torch.ones_like(fixed, dtype=torch.bool)
    M = int(scope.sum())
    cos = torch.cosine_similarity(p[scope], t[scope]) if M else torch.zeros(0, dtype=dtype)
    mag = (p[scope].norm(dim=-1) - t[scope].norm(dim=-1)).abs()
    within = 0
    for b, (a0, a1) in enumerate(_systems(natoms)):
        fs = f[a0:a1][scope[a0:a1]]
        fmax = float(fs.max()) if fs.numel() else 0.0   # the departure: no atom in scope counts as 0
        within += int(bool(e[b] < 0.02) and fmax < 0.03)
    B = int(e.numel())
    out = {"energy_mae": (float(e.double().sum()), B)}
    for k, name in enumerate(("forcesx_mae", "forcesy_mae", "forcesz_mae")):
        out[name] = (float(f[scope][:, k].double().sum()), M)
    out["forces_mae"] = (float(f[scope].double().sum()), 3 * M)
    out["forces_cosine_similarity"] = (float(cos.double().sum()), M)
    out["forces_magnitude_error"] = (float(mag.double().sum()), M)
    out["energy_forces_within_threshold"] = (within, B)
    for name in S2EF_NAMES:
        out["abs::" + name] = out[name][0]
    out["abs::forces_cosine_similarity"] = float(cos.double().abs().sum())
    return out


def mean_min_image_distance(pos_pred, pos_tgt, cell, dtype=torch.float32):
    """Mean over the given atoms of the minimum-image distance: fractional = solve(cell^T, d^T)^T, % 1.0 twice, entries
    above 0.5 moved down by 1, back through the cell; NaN for no atom."""
    d = pos_pred.to(dtype) - pos_tgt.to(dtype)
    if d.shape[0] == 0:
        return float("nan")
    frac = torch.linalg.solve(cell.to(dtype).T, d.T).T
    frac = torch.remainder(torch.remainder(frac, 1.0), 1.0)
    frac = torch.where(frac > 0.5, frac - 1.0, frac)
    return float((frac @ cell.to(dtype)).norm(dim=1).double().mean())


def is2rs(pos_pred, pos_tgt, cell, fixed, natoms, thresholds, dtype=torch.float32):
    free = fixed == 0
    M = int(free.sum())
    e = (pos_tgt.to(dtype) - pos_pred.to(dtype))[free]
    below = 0
    for b, (a0, a1) in enumerate(_systems(natoms)):
        m = free[a0:a1]
        mean = mean_min_image_distance(pos_pred[a0:a1][m], pos_tgt[a0:a1][m], cell[b], dtype)
        below += int((mean < np.asarray(thresholds, dtype=np.float64)).sum())
    out = {"positions_average_distance_within_threshold": (below, len(natoms) * len(thresholds)),
           "positions_mae": (float(e.abs().double().sum()), 3 * M),
           "positions_mse": (float((e * e).double().sum()), 3 * M)}
    for name in IS2RS_NAMES:
        out["abs::" + name] = out[name][0]
    return out


def is2re(e_pred, e_tgt, dtype=torch.float32):
    e = e_tgt.to(dtype) - e_pred.to(dtype)
    B = int(e.numel())
    out = {"energy_mae": (float(e.abs().double().sum()), B), "energy_mse": (float((e * e).double().sum()), B),
           "energy_within_threshold": (int((e.abs() < 0.02).sum()), B)}
    for name in IS2RE_NAMES:
        out["abs::" + name] = out[name][0]
    return out


def add(first, second):
    """Two batches' results chained, as ``prev_metrics`` chains them."""
    out = {}
    for k, v in first.items():
        out[k] = v + second[k] if k.startswith("abs::") else (v[0] + second[k][0], v[1] + second[k][1])
    return out


# ------------------------------------------------------------------------------------------------ the fixture
def fixture():
    return load_npz("evaluator.npz")


def task_inputs(fx, task, batch):
    """The fixture's tensors of one batch ("a": five systems of 7, 61, 64, 65, 130 atoms; "b": one system)."""
    pre = f"{task}_{batch}_"
    return {k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)}


def restate(fx, task, batch, dtype):
    x = task_inputs(fx, task, batch)
    if task == "s2ef":
        return s2ef(x["e_pred"], x["f_pred"], x["e_tgt"], x["f_tgt"], x["fixed"], x["natoms"].tolist(),
                    tuple(fx["norm_energy"].tolist()), tuple(fx["norm_forces"].tolist()), True, dtype)
    if task == "is2rs":
        return is2rs(x["pos_pred"], x["pos_tgt"], x["cell"], x["fixed"], x["natoms"].tolist(), fx["thresholds"], dtype)
    return is2re(x["e_pred"], x["e_tgt"], dtype)


def reference(fx, task, upto, which):
    """{name: (total, numel)} recorded from the reference: ``upto`` "a" (the first batch) or "ab" (both, through
    ``prev_metrics``); ``which`` "32" / "64"; with the float64 run's sum of absolute terms under "abs::" + name."""
    out = {}
    for i, name in enumerate(TASK_NAMES[task]):
        t = fx[f"{task}_total{which}_{upto}"][i]
        out[name] = (int(t) if name in COUNTING else float(t), int(fx[f"{task}_numel_{upto}"][i]))
        out["abs::" + name] = float(fx[f"{task}_abs_{upto}"][i])
    return out


def bound(fx, task, upto, name, k=K_BOUND):
    r32, r64 = reference(fx, task, upto, "32"), reference(fx, task, upto, "64")
    return abs(r32[name][0] - r64[name][0]) + k * EPS32 * r64["abs::" + name]


def measured_k(fx, task, upto, name, total):
    """The k at which ``total`` would just meet the bound (negative: inside the reference's own float32 noise)."""
    r32, r64 = reference(fx, task, upto, "32"), reference(fx, task, upto, "64")
    return (abs(total - r64[name][0]) - abs(r32[name][0] - r64[name][0])) / (EPS32 * r64["abs::" + name])
