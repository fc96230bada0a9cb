"""The evaluation kernels (csrc/evaluate.hip), ``Evaluator`` / ``DeviceMetrics`` and the trainers' ``validate`` /
``evaluate_relaxed`` on the GPU, against the reference's own Evaluator (tests/golden/evaluator.npz: float32 and float64
runs over two chained batches of 5 and 1 systems of 7, 61, 64, 65, 130 and 23 atoms).

Bounds.  Counts and numels: exact.  Float totals against the reference's FLOAT64 totals: |ref32 - ref64| (the reference's own
float32 noise on the same inputs) + K * 2^-24 * sum |term| with K = tests/helpers_evaluate.K_BOUND; every case prints the k
it measures."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.evaluator import NUM_SLOTS, SLOTS, DeviceMetrics, Evaluator, atom_offsets
from adsorbdiff_amd.trainer import DenoisingTrainer, ForcesTrainer
from tests import helpers_evaluate as HE

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TASKS = ("s2ef", "is2rs", "is2re")


@pytest.fixture(scope="module")
def fx():
    return HE.fixture()


def add_batch(dm, fx, task, batch):
    """One fixture batch through the task's kernel entry, with the inputs the kernels take."""
    x = {k: v.to(DEV) for k, v in HE.task_inputs(fx, task, batch).items()}
    if task == "is2re":
        return dm.add_is2re(x["e_pred"], x["e_tgt"])
    off, fixed = atom_offsets(x["natoms"], DEV), x["fixed"].to(torch.int32)
    if task == "s2ef":
        return dm.add_s2ef(x["e_pred"], x["f_pred"], x["e_tgt"], x["f_tgt"], off, fixed=fixed, free_only=True,
                           norm_energy=tuple(fx["norm_energy"].tolist()), norm_forces=tuple(fx["norm_forces"].tolist()))
    return dm.add_is2rs(x["pos_pred"], x["pos_tgt"], x["cell"], off, fixed=fixed)


def check_against_reference(fx, task, upto, got, label):
    r64 = HE.reference(fx, task, upto, "64")
    worst = 0.0
    for name in HE.TASK_NAMES[task]:
        assert got[name]["numel"] == r64[name][1], (label, name, got[name], r64[name])
        if name in HE.COUNTING:
            assert got[name]["total"] == r64[name][0], (label, name, got[name], r64[name])
            continue
        k = HE.measured_k(fx, task, upto, name, got[name]["total"])
        worst = max(worst, k)
        print(f"{label} {name}: total {got[name]['total']:.12g} reference64 {r64[name][0]:.12g} k {k:.3f}")
        assert abs(got[name]["total"] - r64[name][0]) <= HE.bound(fx, task, upto, name), (label, name, k)
        assert got[name]["metric"] == got[name]["total"] / got[name]["numel"]
    return worst


# ------------------------------------------------------------------------------------------------ kernels vs the fixture
@pytest.mark.parametrize("task", TASKS)
def test_kernels_against_the_reference_over_two_batches(fx, task):
    """Integer slots exact, float totals within the bound, after the first batch and after both (the reference's
    ``prev_metrics`` chain); slots of other tasks stay untouched."""
    dm = DeviceMetrics(DEV)
    add_batch(dm, fx, task, "a")
    first = dm.result(HE.TASK_NAMES[task])
    add_batch(dm, fx, task, "b")
    both = dm.result(HE.TASK_NAMES[task])
    k = max(check_against_reference(fx, task, "a", first, f"{task} a"), check_against_reference(fx, task, "ab", both, f"{task} ab"))
    print(f"{task}: worst measured k {k:.3f} (bound {HE.K_BOUND})")
    written = {SLOTS[n] for n in HE.TASK_NAMES[task]}
    numel = dm.numel.cpu().tolist()
    assert all((numel[i] > 0) == (i in written) for i in range(NUM_SLOTS))
    assert set(dm.result()) == set(HE.TASK_NAMES[task])


@pytest.mark.parametrize("task", TASKS)
def test_same_bits_on_a_second_run_and_after_a_fresh_zero(fx, task):
    def run(dm):
        add_batch(dm, fx, task, "a")
        add_batch(dm, fx, task, "b")
        return dm.total.clone(), dm.numel.clone()

    dm = DeviceMetrics(DEV)
    t1, n1 = run(dm)
    t2, n2 = run(DeviceMetrics(DEV))
    assert torch.equal(t1.view(torch.int64), t2.view(torch.int64)) and torch.equal(n1, n2)
    t3, n3 = run(dm.zero())   # the used accumulator, zeroed: as a fresh one
    assert torch.equal(t1.view(torch.int64), t3.view(torch.int64)) and torch.equal(n1, n3)
    # and the order of the batches is part of the result's definition, not of its value here: b then a sums the same terms
    dm.zero()
    add_batch(dm, fx, task, "b")
    add_batch(dm, fx, task, "a")
    assert torch.equal(dm.numel, n1) and torch.allclose(dm.total, t1, rtol=1e-14, atol=0)


@pytest.mark.parametrize("task", TASKS)
def test_evaluator_eval_takes_what_the_reference_s_callers_pass(fx, task):
    """``Evaluator(task).eval`` on denormalised tensors already cut to the free atoms, chained through ``prev_metrics``."""
    ev, metrics = Evaluator(task), {}
    for batch in HE.BATCHES:
        x = {k: v.to(DEV) for k, v in HE.task_inputs(fx, task, batch).items()}
        if task == "is2re":
            pred, tgt = {"energy": x["e_pred"]}, {"energy": x["e_tgt"]}
        else:
            mask = x["fixed"] == 0
            nfree = torch.zeros(len(x["natoms"]), dtype=torch.int64, device=DEV).index_add_(
                0, torch.repeat_interleave(torch.arange(len(x["natoms"]), device=DEV), x["natoms"]), mask.long())
            if task == "s2ef":
                ne, nf = fx["norm_energy"], fx["norm_forces"]
                pred = {"energy": x["e_pred"] * float(ne[1]) + float(ne[0]), "forces": (x["f_pred"] * float(nf[1]) + float(nf[0]))[mask],
                        "natoms": nfree}
                tgt = {"energy": x["e_tgt"], "forces": x["f_tgt"][mask], "natoms": nfree}
            else:
                pbc = torch.tensor([True, True, True])
                pred = {"positions": x["pos_pred"][mask], "cell": x["cell"], "pbc": pbc, "natoms": nfree}
                tgt = {"positions": x["pos_tgt"][mask], "cell": x["cell"], "pbc": pbc, "natoms": nfree}
        metrics = ev.eval(pred, tgt, prev_metrics=metrics)
        assert list(metrics) == HE.TASK_NAMES[task]
        check_against_reference(fx, task, "a" if batch == "a" else "ab", metrics, f"eval {task} {batch}")
    # the same bits as the kernels on the undenormalised, unmasked inputs: the cut and the denorm round alike
    dm = DeviceMetrics(DEV)
    add_batch(dm, fx, task, "a")
    add_batch(dm, fx, task, "b")
    direct = dm.result(HE.TASK_NAMES[task])
    for name in HE.TASK_NAMES[task]:
        assert metrics[name]["numel"] == direct[name]["numel"]
        assert abs(metrics[name]["total"] - direct[name]["total"]) <= 1e-15 * abs(direct[name]["total"]), name


def test_a_system_without_free_atoms_by_hand():
    """Two systems, the first with every atom fixed.  s2ef: its force maximum counts as 0, so its energy error 0.015625
    alone makes it pass (the reference raises there); is2rs: its mean distance is NaN and lies below no threshold.  The
    second system's numbers are worked out by hand:
      forces  atom 2: prediction (3, 4, 0), target (0, 0, 0): errors 3, 4, 0; cosine 0 (zero row); magnitudes |5 - 0| = 5
              atom 3: prediction (0, 0, 2), target (0, 0, 1): errors 0, 0, 1; cosine 1; magnitudes |2 - 1| = 1
      energy  errors 0.015625 and 0.5
      positions in a cubic cell of 10: displacements (0.301, 0, 0) and (9.9, 0, 0); minimum image 0.301 and 0.1, mean
              0.2005: below the thresholds 0.201 ... 0.499, which are 299 of the 490."""
    off = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    fixed = torch.tensor([1, 1, 0, 0], dtype=torch.int32, device=DEV)
    f_pred = torch.tensor([[9.0, 9.0, 9.0], [-9.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 2.0]], device=DEV)
    f_tgt = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], device=DEV)
    e_pred, e_tgt = torch.tensor([1.0, 2.0], device=DEV), torch.tensor([1.015625, 2.5], device=DEV)
    dm = DeviceMetrics(DEV)
    dm.add_s2ef(e_pred, f_pred, e_tgt, f_tgt, off, fixed=fixed, free_only=True)
    got = {k: (v["total"], v["numel"]) for k, v in dm.result(HE.S2EF_NAMES).items()}
    assert got == {"energy_mae": (0.515625, 2), "forcesx_mae": (3.0, 2), "forcesy_mae": (4.0, 2), "forcesz_mae": (1.0, 2),
                   "forces_mae": (8.0, 6), "forces_cosine_similarity": (1.0, 2), "forces_magnitude_error": (6.0, 2),
                   "energy_forces_within_threshold": (1, 2)}
    # without the mask the first system's forces fail it
    dm.zero().add_s2ef(e_pred, f_pred, e_tgt, f_tgt, off, fixed=fixed, free_only=False)
    assert dm.result(["energy_forces_within_threshold", "forces_mae"]) == {
        "energy_forces_within_threshold": {"metric": 0.0, "total": 0, "numel": 2},
        "forces_mae": {"metric": 44.0 / 12, "total": 44.0, "numel": 12}}

    cell = (10.0 * torch.eye(3, device=DEV)).repeat(2, 1, 1)
    pos_tgt = torch.tensor([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [4.0, 4.0, 4.0]], device=DEV)
    disp = torch.tensor([[0.7, 0.0, 0.0], [0.0, 0.9, 0.0], [0.301, 0.0, 0.0], [9.9, 0.0, 0.0]], device=DEV)
    dm.zero().add_is2rs(pos_tgt + disp, pos_tgt, cell, off, fixed=fixed)
    got = dm.result(HE.IS2RS_NAMES)
    assert got["positions_average_distance_within_threshold"] == {"metric": 299 / 980, "total": 299, "numel": 980}
    assert got["positions_mae"]["numel"] == got["positions_mse"]["numel"] == 6
    assert abs(got["positions_mae"]["total"] - 10.201) < 1e-5 and abs(got["positions_mse"]["total"] - 98.100601) < 1e-4
    # every atom of the batch fixed: nothing but the numels of the per-system metrics
    dm.zero().add_is2rs(pos_tgt + disp, pos_tgt, cell, off, fixed=torch.ones_like(fixed))
    assert {k: (v["total"], v["numel"]) for k, v in dm.result(HE.IS2RS_NAMES).items()} == {
        "positions_average_distance_within_threshold": (0, 980), "positions_mae": (0.0, 0), "positions_mse": (0.0, 0)}


def test_add_value_counts_one_per_call():
    dm = DeviceMetrics(DEV)
    for v in (0.5, 1.25, 3.0):
        dm.add_value("loss", torch.tensor([v, 77.0], device=DEV))
    assert dm.result(["loss"]) == {"loss": {"metric": 4.75 / 3, "total": 4.75, "numel": 3}}


# ------------------------------------------------------------------------------------------------ ForcesTrainer.validate
def _forces_case():
    """The 2-layer H = 128 model of tests/helpers_s2ef_train.py, three batches of 4, 3 and 1 systems with targets."""
    from tests import helpers_s2ef_train as HS

    fx, m, b, kw = HS.fixture_case()
    batches = [b, HS.make_config_batch("odd_width", seed=41), HS.make_config_batch("single", seed=42)]
    for extra in batches[1:]:   # targets of the fixture's normalisers' magnitude
        extra.energy = extra.energy * 0.5 - 1.0
    return m, batches, kw


def test_forces_trainer_validate():
    """Every metric equals the kernels applied to ``predict``'s outputs (bit for bit: ``predict``'s denorm and the kernel's
    round alike); ``loss`` is the mean of the training engine's loss on the same batches with the same (EMA) weights, within
    the 1e-5 the training forward is held to; the parameters are bit-unchanged although the EMA shadow differs from them."""
    m, batches, kw = _forces_case()
    tr = ForcesTrainer(m, device=DEV, normalizers=kw["normalizers"])
    tr.setup_training(1e-3, energy_coefficient=kw["energy_coefficient"], force_coefficient=kw["force_coefficient"])
    with torch.no_grad():
        for s in tr.ema.shadow_params:
            s.mul_(1.02)
    before = [p.detach().clone() for p in m.parameters()]
    got = tr.validate([b.clone() for b in batches])
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert list(got) == HE.S2EF_NAMES + ["loss"] and not m.training

    dm = DeviceMetrics(DEV)
    for b in batches:
        bd = b.clone().to(DEV)
        out = tr.predict(bd)
        dm.add_s2ef(out["energy"], out["forces"], bd.energy, bd.forces, atom_offsets(bd.natoms, DEV),
                    fixed=bd.fixed.to(torch.int32), free_only=True)
    want = dm.result(HE.S2EF_NAMES)
    for name in HE.S2EF_NAMES:
        assert got[name] == want[name], (name, got[name], want[name])
    assert got["energy_mae"]["numel"] == 8 and got["forces_mae"]["numel"] == 3 * sum(int((b.fixed == 0).sum()) for b in batches)

    tr.ema.store()
    tr.ema.copy_to()
    try:
        losses = []
        for b in batches:
            tr.train_engine.zero_grad()
            losses.append(float(tr.train_engine.loss_and_grad(b.clone().to(DEV))[0]))
    finally:
        tr.ema.restore()
        tr.train_engine.zero_grad()
    mean = sum(losses) / len(losses)
    print(f"validate loss {got['loss']['metric']:.8f}, training engine's mean {mean:.8f}")
    assert got["loss"]["numel"] == 3 and abs(got["loss"]["metric"] - mean) < 1e-5 * abs(mean)
    # without setup_training: the objective's defaults (coefficients 1 and 30), the same metrics
    plain = ForcesTrainer(m, device=DEV, normalizers=kw["normalizers"], ema=tr.ema)
    again = plain.validate([b.clone() for b in batches])
    assert all(again[name] == got[name] for name in HE.S2EF_NAMES) and again["loss"]["metric"] != got["loss"]["metric"]


def test_forces_trainer_validate_with_energy_gradient_forces():
    """force_mode "energy_gradient": the forces are denormalised with the energy's std and no mean, as ``predict`` does."""
    m, batches, kw = _forces_case()
    m.force_mode = "energy_gradient"
    tr = ForcesTrainer(m, device=DEV, normalizers=kw["normalizers"])
    got = tr.validate([batches[0].clone()])
    bd = batches[0].clone().to(DEV)
    out = tr.predict(bd)
    dm = DeviceMetrics(DEV)
    dm.add_s2ef(out["energy"], out["forces"], bd.energy, bd.forces, atom_offsets(bd.natoms, DEV), fixed=bd.fixed.to(torch.int32))
    want = dm.result(HE.S2EF_NAMES)
    assert all(got[name] == want[name] for name in HE.S2EF_NAMES)


# ------------------------------------------------------------------------------------------------ DenoisingTrainer.validate
def test_denoising_trainer_validate_on_noised_batches():
    """``validate(noised=True)``: the mean over the batches of the score loss, equal to the mean of the training engine's
    ``loss_and_grad`` loss on the same pre-noised batches within the 1e-5 tests/test_gpu_training.py holds both forwards
    to; ``pos_relaxed`` stands in for the positions; the task "ocp" has no metrics, so ``loss`` is all there is."""
    from tests import helpers_train as HT

    m = HT.make_config_model("ragged").to(DEV)
    tables = HT.igso3_tables()[0]
    tr = DenoisingTrainer(m, device=DEV)
    tr.setup_training(dict(ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55), ema_decay=0, tables=tables)
    batches, losses = [], []
    for name, seed in (("ragged", 5), ("single", 6), ("big_adsorbate", 7)):
        b = HT.make_config_batch(name)
        targets = HT.make_targets(int(b.natoms.numel()), seed=seed)
        for k, v in targets.items():
            setattr(b, k, v)
        tr.train_engine.zero_grad()
        losses.append(float(tr.train_engine.loss_and_grad(b.clone().to(DEV), targets)[0]))
        batches.append(b)
    tr.train_engine.zero_grad()
    first = batches[0]
    first.pos_relaxed = first.pos.clone()
    first.pos = first.pos + 0.37   # must not be read
    before = [p.detach().clone() for p in m.parameters()]
    got = tr.validate([b.clone() for b in batches], noised=True)
    mean = sum(losses) / len(losses)
    print(f"denoising validate loss {got['loss']['metric']:.8f}, training engine's mean {mean:.8f}")
    assert list(got) == ["loss"] and got["loss"]["numel"] == 3
    assert abs(got["loss"]["metric"] - mean) < 1e-5 * abs(mean)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))


# ------------------------------------------------------------------------------------------------ evaluate_relaxed
def test_evaluate_relaxed_on_the_fixture_batches(fx):
    m, _, kw = _forces_case()
    tr = ForcesTrainer(m, device=DEV, normalizers=kw["normalizers"])
    metrics = None
    for batch in HE.BATCHES:
        x, y = HE.task_inputs(fx, "is2rs", batch), HE.task_inputs(fx, "is2re", batch)
        b = Batch()
        b.pos, b.pos_relaxed, b.cell, b.fixed, b.natoms = x["pos_pred"], x["pos_tgt"], x["cell"], x["fixed"].long(), x["natoms"]
        b.y, b.y_relaxed = y["e_pred"], y["e_tgt"]
        metrics = tr.evaluate_relaxed(b, metrics)
    is2rs, is2re = metrics
    check_against_reference(fx, "is2rs", "ab", is2rs.result(Evaluator("is2rs").metric_names()), "evaluate_relaxed is2rs")
    check_against_reference(fx, "is2re", "ab", is2re.result(Evaluator("is2re").metric_names()), "evaluate_relaxed is2re")


# ------------------------------------------------------------------------------------------------ two ranks
WORKER = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_s2ef_train as HS

rank = int(os.environ["RANK"])
dist.init_process_group("gloo")
fx, m, full, kw = HS.fixture_case()
tr = ForcesTrainer(m, device="cuda:0", normalizers=kw["normalizers"])
tr.setup_training(0.0, ema_decay=0.0, energy_coefficient=kw["energy_coefficient"], force_coefficient=kw["force_coefficient"])
data = full.to_data_list()
lo, hi = (0, 1) if rank == 0 else (1, len(data))          # one system on rank 0, three on rank 1
mine = Batch.from_data_list(data[lo:hi])
a0, a1 = int(full.natoms[:lo].sum()), int(full.natoms[:hi].sum())
mine.energy, mine.forces = full.energy[lo:hi].clone(), full.forces[a0:a1].clone()
out = tr.validate([mine])
if rank == 0:
    torch.save(out, sys.argv[2])
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_aggregate_to_the_one_rank_run(tmp_path):
    """Two gloo ranks on one GPU, one system on rank 0 and three on rank 1: after ``all_reduce`` every metric's total and
    numel equal the one-rank run over both parts (the same two float64 addends), and ``loss`` - whose divisors are the
    all-reduced system and atom counts, as in ``train_step`` - is the loss of the whole batch."""
    from tests import helpers_s2ef_train as HS

    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), str(ROOT), str(tmp_path / "v.pt")], env=env))
    assert [p.wait(timeout=600) for p in procs] == [0, 0]
    two = torch.load(tmp_path / "v.pt")

    fxs, m, full, kw = HS.fixture_case()
    tr = ForcesTrainer(m, device=DEV, normalizers=kw["normalizers"])
    tr.setup_training(0.0, ema_decay=0.0, energy_coefficient=kw["energy_coefficient"], force_coefficient=kw["force_coefficient"])
    data = full.to_data_list()
    parts = []
    for lo, hi in ((0, 1), (1, len(data))):
        p = Batch.from_data_list(data[lo:hi])
        a0, a1 = int(full.natoms[:lo].sum()), int(full.natoms[:hi].sum())
        p.energy, p.forces = full.energy[lo:hi].clone(), full.forces[a0:a1].clone()
        parts.append(p)
    one = tr.validate(parts)
    for name in HE.S2EF_NAMES:
        assert two[name] == one[name], (name, two[name], one[name])
    whole = tr.validate([full.clone()])
    assert two["loss"]["numel"] == 2
    assert abs(two["loss"]["metric"] - whole["loss"]["metric"]) < 1e-5 * abs(whole["loss"]["metric"])
