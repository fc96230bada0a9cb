"""Host side of the evaluation path: the plain-torch restatement of tests/helpers_evaluate.py against the reference's own
Evaluator (tests/golden/evaluator.npz, tools/make_golden_evaluator.py), the conditions that keep the fixture's counting
metrics exact, the slot table against the header's enum, and the Evaluator's names."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from adsorbdiff_amd import evaluator as EV
from tests import helpers_evaluate as HE

ROOT = Path(__file__).resolve().parent.parent
TASKS = ("s2ef", "is2rs", "is2re")


@pytest.fixture(scope="module")
def fx():
    return HE.fixture()


@pytest.mark.parametrize("task", TASKS)
def test_restatement_reproduces_the_reference(fx, task):
    """Counts and numels exactly; float totals in float64 to 1e-12 relative, in float32 within a few float32 roundings of the
    sum of absolute terms (the restatement sums in float64, the reference in float32)."""
    for which, dtype in (("32", torch.float32), ("64", torch.float64)):
        a, b = HE.restate(fx, task, "a", dtype), HE.restate(fx, task, "b", dtype)
        for upto, got in (("a", a), ("ab", HE.add(a, b))):
            ref = HE.reference(fx, task, upto, which)
            for name in HE.TASK_NAMES[task]:
                assert got[name][1] == ref[name][1], (task, upto, name)
                if name in HE.COUNTING:
                    assert got[name][0] == ref[name][0], (task, upto, which, name, got[name], ref[name])
                else:
                    tol = 1e-12 * abs(ref[name][0]) if which == "64" else 4 * HE.EPS32 * ref["abs::" + name]
                    assert abs(got[name][0] - ref[name][0]) <= tol, (task, upto, which, name, got[name][0], ref[name][0])
                    if which == "64":
                        assert abs(got["abs::" + name] - ref["abs::" + name]) <= 1e-12 * ref["abs::" + name], (task, name)


def test_fixture_shapes_and_outcomes(fx):
    """The shapes the kernels can go wrong at, and the cases the counting metrics must tell apart."""
    assert fx["s2ef_a_natoms"].tolist() == [7, 61, 64, 65, 130] and len(fx["s2ef_b_natoms"]) == 1
    x = HE.task_inputs(fx, "s2ef", "a")
    ne, nf = fx["norm_energy"], fx["norm_forces"]
    e = (x["e_tgt"].double() - (x["e_pred"].double() * ne[1] + ne[0])).abs()
    f = (x["f_tgt"].double() - (x["f_pred"].double() * nf[1] + nf[0])).abs()
    assert float((e - 0.02).abs().min()) >= 1e-4
    off = [0] + np.cumsum(fx["s2ef_a_natoms"]).tolist()
    outcomes = []
    for b in range(5):
        free = x["fixed"][off[b]:off[b + 1]] == 0
        fs = f[off[b]:off[b + 1]]
        assert 0 < int(free.sum()) < len(free)
        assert abs(float(fs[free].max()) - 0.03) >= 1e-4
        outcomes.append((bool(e[b] < 0.02), bool(fs[free].max() < 0.03), bool(fs.max() < 0.03)))
    # pass, energy only fails, force only fails, the largest force error sits on a fixed atom (passes), both fail
    assert outcomes == [(True, True, True), (False, True, True), (True, False, False), (True, True, False), (False, False, False)]
    free = x["fixed"] == 0
    assert bool((x["f_tgt"][free] == 0).all(dim=1).any())
    y = HE.task_inputs(fx, "is2rs", "a")
    d = (y["pos_pred"] - y["pos_tgt"]).double()
    wrapped = 0
    for b in range(5):
        cell = y["cell"][b].double()
        assert float((cell - torch.diag(torch.diag(cell))).abs().max()) > 0.1      # not orthogonal
        frac = torch.linalg.solve(cell.T, d[off[b]:off[b + 1]][y["fixed"][off[b]:off[b + 1]] == 0].T).T
        wrapped += int((frac.abs() > 0.5).sum())
        assert float((torch.remainder(frac, 1.0) - 0.5).abs().min()) >= 1e-3
    assert wrapped >= 2
    assert np.array_equal(fx["thresholds"], EV.distance_thresholds()) and len(fx["thresholds"]) == 490
    assert not np.array_equal(fx["thresholds"], 0.01 + 0.001 * np.arange(490))      # arange's rounding, not the formula's


def test_slot_table_matches_the_header():
    hdr = (ROOT / "include" / "adsorbdiff_hip.h").read_text()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bADF_EVAL_([A-Z0-9_]+) = (\d+)", hdr)}
    assert enum.pop("slots") == EV.NUM_SLOTS == len(EV.SLOTS)
    assert enum == EV.SLOTS
    assert sorted(EV.SLOTS.values()) == list(range(EV.NUM_SLOTS))


def test_evaluator_names_are_the_reference_s(fx):
    for task in TASKS:
        ev = EV.Evaluator(task)
        assert ev.metric_names() == [str(n) for n in fx[f"{task}_names"]] == HE.TASK_NAMES[task]
        assert str(EV.Evaluator.task_primary_metric[task]) == str(fx[f"{task}_primary"])
        assert all(n in EV.SLOTS for n in ev.metric_names())
    # the task the denoising trainer evaluates under: a primary-metric entry (None) and no metrics
    assert "ocp" in EV.Evaluator.task_primary_metric and str(EV.Evaluator.task_primary_metric["ocp"]) == str(fx["ocp_primary"])
    assert ("ocp" in EV.Evaluator.task_metrics) == bool(fx["ocp_has_metrics"]) and EV.Evaluator("ocp").metric_names() == []
    assert EV.Evaluator("ocp").eval({}, {}, {}) == {}


def test_unsupported_eval_metrics_raise_with_the_name():
    with pytest.raises(NotImplementedError, match="forcesx_mse"):
        EV.Evaluator("s2ef", eval_metrics={"energy": ["mae"], "forces": ["forcesx_mse"]})
    with pytest.raises(NotImplementedError, match="energy_mse"):
        EV.Evaluator("s2ef", eval_metrics={"energy": ["mae", "mse"]})
    EV.Evaluator("s2ef", eval_metrics=EV.Evaluator.task_metrics["s2ef"])   # the default set, spelled out: accepted


def test_update_chains_like_the_reference():
    ev = EV.Evaluator("is2re")
    m = ev.update("loss", 0.5, {})
    m = ev.update("loss", 1.5, m)
    assert m["loss"] == {"metric": 1.0, "total": 2.0, "numel": 2}
    m = ev.update("energy_mae", {"total": 3.0, "numel": 4}, m)
    m = ev.update("energy_mae", {"total": 1.0, "numel": 4}, m)
    assert m["energy_mae"] == {"metric": 0.5, "total": 4.0, "numel": 8}


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EV.DeviceMetrics("cpu")
