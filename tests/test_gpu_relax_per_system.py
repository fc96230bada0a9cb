"""GPU tests of the per-system L-BFGS mode (csrc/lbfgs.hip, lb_per_system_kernel): against the reference's one-system-alone
records (tools/make_golden_relax_per_system.py), against the float64 statement of the contract at the sizes where the
reduction changes shape, and the invariances the mode is for - alone equals in-batch, ml_relax's out-of-memory split,
shards."""
import ctypes as C

import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import sampler as S
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc
from adsorbdiff_amd.ml_relaxation import ml_relax
from adsorbdiff_amd.painn import PaiNN
from adsorbdiff_amd.synthetic import make_system
from adsorbdiff_amd.trainer import ForcesTrainer
from tests.helpers import batch_from_fixture, load_npz
from tests.helpers_lbfgs_per_system import OneSystemLBFGS, max_force, split_systems, ulp_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP_SMALL = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES_SMALL = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}


def _sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


class _Fixed:
    """A trainer whose predict returns whatever forces the test put there (teacher forcing)."""

    def __init__(self):
        self._unwrapped_model = type("M", (), {"otf_graph": True})()
        self.forces = None

    def predict(self, batch, per_image=False, disable_tqdm=True):
        return {"energy": torch.zeros(int(batch.natoms.shape[0]), device=DEV), "forces": self.forces.clone()}


def _optimizer(b, fx, tr, **kw):
    opt = LBFGS(b, TorchCalc(tr), maxstep=float(fx["maxstep"]), memory=int(fx["memory"]), damping=float(fx["damping"]),
                alpha=float(fx["alpha"]), device=DEV, per_system=True, **kw)
    opt.fmax = float(fx["fmax"])
    opt._setup()
    return opt


def _forced_step(opt, tr, k, f):
    tr.forces = f
    _, _, forces = opt.check_convergence(k)
    opt.step(k, forces)


@pytest.mark.parametrize("tag", ["ring", "skip"])
def test_teacher_forced_steps_vs_reference_alone(tag):
    fx = _sub(load_npz("relax_per_system.npz"), tag + "_")
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    tr = _Fixed()
    opt = _optimizer(b, fx, tr)
    taken = torch.zeros(4, dtype=torch.int32)
    for k in range(fx["forces"].shape[0]):
        _forced_step(opt, tr, k, torch.from_numpy(fx["forces"][k]).to(DEV))
        mask = torch.from_numpy(fx["masks"][k])
        assert torch.equal(opt.update_mask().cpu().bool(), mask), k
        steps, absmax = (t.cpu() for t in opt.step_state())
        taken += mask.int()
        assert torch.equal(steps, taken), (k, steps.tolist())
        assert torch.equal(absmax >= 0, mask), (k, absmax.tolist())                          # who attempted a step
        assert torch.equal((absmax >= 0) & (absmax < 1e-7), torch.from_numpy(fx["skipped"][k])), (k, absmax.tolist())
        assert float(opt.last_step_max()) == float(absmax.clamp(min=0).max()), k
        assert ulp_close(b.pos, fx["pos_after"][k]), (k, float((b.pos.cpu() - torch.from_numpy(fx["pos_after"][k])).abs().max()))
    assert torch.equal(opt.step_state()[0].cpu(), torch.from_numpy(fx["steps_taken"]))
    opt.close()


def test_alone_equals_in_batch_bit_for_bit():
    """Each `ring` system relaxed with a handle of its own under the same scripted forces: the same bits as its rows of the
    batch run after every iteration (the order of a dot product's sum depends on the system's atom count alone)."""
    fx = _sub(load_npz("relax_per_system.npz"), "ring_")
    natoms = fx["natoms"].tolist()
    K = fx["forces"].shape[0]
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    tr = _Fixed()
    opt = _optimizer(b, fx, tr)
    in_batch = []
    for k in range(K):
        _forced_step(opt, tr, k, torch.from_numpy(fx["forces"][k]).to(DEV))
        in_batch.append(split_systems(b.pos.clone(), natoms))
    opt.close()
    offs = [0] + torch.cumsum(torch.tensor(natoms), 0).tolist()
    for s, d in enumerate(batch_from_fixture(fx, pos_key="pos_in").to_data_list()):
        one = Batch.from_data_list([d]).to(DEV)
        o = _optimizer(one, fx, tr)
        for k in range(K):
            _forced_step(o, tr, k, torch.from_numpy(fx["forces"][k][offs[s]:offs[s + 1]]).to(DEV))
            assert torch.equal(one.pos, in_batch[k][s]), (s, k)
        assert int(o.step_state()[0][0]) == int(fx["steps_taken"][s])
        o.close()


class _HarmonicBySystem:
    """F = -k_s (x - x*), evaluated system by system (a system's forces come from its own rows alone)."""

    def __init__(self, xstar, k, natoms):
        self._unwrapped_model = type("M", (), {"otf_graph": True})()
        self.xstar, self.k, self.natoms = xstar, k, natoms

    def predict(self, batch, per_image=False, disable_tqdm=True):
        f = [-(self.k[s] * (p - x)) for s, (p, x) in enumerate(zip(split_systems(batch.pos, self.natoms),
                                                                  split_systems(self.xstar, self.natoms)))]
        return {"energy": torch.zeros(len(self.natoms), device=DEV), "forces": torch.cat(f)}


SHAPE_ATOMS = (1, 2, 85, 7, 86, 171, 300)     # 3 n = 3, 6, 255, 258, 513, 900: either side of 256 and of 512; 7: all fixed
FIXED_SYS = 3


@pytest.mark.parametrize("memory", [1, 3])
def test_reduction_shapes_vs_contract_statement(memory):
    """12 iterations on the device's own trajectory; at every iteration the float64 statement of the contract takes the
    same step for each system from the same positions and forces (its history is the device's history), and the new
    positions agree within 1 f32 ulp.  One system has every atom fixed: its mask is never set, nothing of it moves, its
    step counter stays 0 and no NaN reaches its neighbours."""
    gen = torch.Generator().manual_seed(91)
    systems = [make_system(gen, n - 1, 1, sid=str(i)) for i, n in enumerate(SHAPE_ATOMS)]
    systems[FIXED_SYS].fixed = torch.ones_like(systems[FIXED_SYS].fixed)
    b = Batch.from_data_list(systems).to(DEV)
    natoms = list(SHAPE_ATOMS)
    xstar = (b.pos + 0.3 * torch.randn(b.pos.shape, generator=gen).to(DEV)).float()
    tr = _HarmonicBySystem(xstar, [2.0, 5.0, 9.0, 4.0, 3.0, 7.0, 6.0], natoms)
    fmax = 1e-3
    opt = LBFGS(b, TorchCalc(tr), maxstep=0.04, memory=memory, damping=1.0, alpha=70.0, device=DEV, per_system=True)
    opt.fmax = fmax
    opt._setup()
    ref = [OneSystemLBFGS(memory) for _ in natoms]
    pos_in = b.pos.clone()
    taken = [0] * len(natoms)
    for k in range(12):
        before = [p.cpu().clone() for p in split_systems(b.pos, natoms)]
        _, _, forces = opt.check_convergence(k)
        opt.step(k, forces)
        fs = split_systems(forces.cpu(), natoms)
        mask = opt.update_mask().cpu().bool().tolist()
        steps, absmax = (t.cpu() for t in opt.step_state())
        for s, o in enumerate(ref):
            on = bool(max_force(fs[s]) >= fmax)
            assert on == mask[s], (k, s)
            taken[s] += on
            skipped = o.step(before[s], fs[s], on)       # moves before[s]
            assert (skipped is None) == (float(absmax[s]) == -1.0) and bool(skipped) == (0 <= float(absmax[s]) < 1e-7), (k, s)
        assert steps.tolist() == taken, k
        assert ulp_close(b.pos, torch.cat(before)), (k, float((b.pos.cpu() - torch.cat(before)).abs().max()))
        assert bool(torch.isfinite(b.pos).all()), k
    assert taken[FIXED_SYS] == 0 and min(t for s, t in enumerate(taken) if s != FIXED_SYS) > memory + 1
    assert torch.equal(split_systems(b.pos, natoms)[FIXED_SYS], split_systems(pos_in, natoms)[FIXED_SYS])
    assert not torch.equal(b.pos, pos_in)
    opt.close()


def _painn():
    fx = load_npz("relax_run.npz")
    torch.manual_seed(int(fx["seed"]))
    m = PaiNN(None, 50, 1, scale_file=dict(SCALES_SMALL), **HP_SMALL).to(DEV).eval()
    return fx, ForcesTrainer(m, device=DEV)


def _relax(fx, tr, per_system, batch=None):
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV) if batch is None else batch
    opt = {"memory": int(fx["memory"]), "per_system": per_system}
    return ml_relax(b, tr, steps=int(fx["steps"]), fmax=float(fx["fmax"]), relax_opt=opt, save_full_traj=False, device=DEV)


def _same(a, b):
    return torch.equal(a.pos, b.pos) and torch.equal(a.y, b.y) and torch.equal(a.force, b.force)


@pytest.fixture(scope="module")
def painn_runs():
    """The small S2EF PaiNN on the relax_run.npz batch: the default-mode run, then the per-system run, computed once."""
    fx, tr = _painn()
    default = _relax(fx, tr, False)
    per_system = _relax(fx, tr, True)
    return fx, tr, default, per_system


def test_default_mode_untouched_by_a_per_system_run(painn_runs):
    fx, tr, default, per_system = painn_runs
    again = _relax(fx, tr, False)          # after a per-system relaxation has run in this process
    assert _same(again, default)
    assert not torch.equal(per_system.pos, default.pos)      # the two modes are different optimizers


class _TwoAtMost:
    """A trainer that does not fit more than two systems (ml_relax then relaxes the halves)."""

    def __init__(self, tr):
        self.tr, self._unwrapped_model, self.refused = tr, tr._unwrapped_model, 0

    def predict(self, batch, per_image=False, disable_tqdm=True):
        if int(batch.natoms.shape[0]) > 2:
            self.refused += 1
            raise RuntimeError("HIP out of memory (stand-in)")
        return self.tr.predict(batch, per_image=per_image, disable_tqdm=disable_tqdm)


def test_ml_relax_split_invariance(painn_runs):
    fx, tr, _, whole = painn_runs
    # the precondition: a system's forces do not depend on the other systems of its batch
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    natoms = fx["natoms"].tolist()
    full = {k: v.clone() for k, v in tr.predict(b, per_image=False, disable_tqdm=True).items()}
    data = b.to_data_list()
    for half in ([2, 3], [0, 1]):
        part = tr.predict(Batch.from_data_list([data[i] for i in half]), per_image=False, disable_tqdm=True)
        want = torch.cat([split_systems(full["forces"], natoms)[i] for i in half])
        rows = (part["forces"] != want).any(1).nonzero().reshape(-1).tolist()
        assert not rows, f"forces of systems {half} alone differ from the four-system forward at rows {rows}"
        assert torch.equal(part["energy"], full["energy"][half])
    small = _TwoAtMost(tr)
    split = _relax(fx, small, True)
    assert small.refused == 1 and split.sid == ["2", "3", "0", "1"]
    back = [split.sid.index(s) for s in whole.sid]
    sp, sf = split_systems(split.pos, split.natoms.tolist()), split_systems(split.force, split.natoms.tolist())
    assert torch.equal(torch.cat([sp[i] for i in back]), whole.pos)
    assert torch.equal(split.y[back], whole.y)
    assert torch.equal(torch.cat([sf[i] for i in back]), whole.force)


def test_two_shards_merge_to_the_single_run(painn_runs):
    fx, tr, _, whole = painn_runs
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    natoms = fx["natoms"].tolist()
    bounds = S.relaxed_bounds(natoms, 2)
    msgs, dealt = [], []
    for r in range(2):
        mine, ids = S.shard_batch(b, r, 2)
        msgs.append(S.pack_relaxed(_relax(fx, tr, True, batch=mine), ids, bounds))
        dealt += ids
    assert sorted(dealt) == [0, 1, 2, 3]
    pos, y, force = S.merge_packed_relaxed(torch.stack(msgs), natoms)      # what the all-gather hands every rank
    assert torch.equal(pos, whole.pos) and torch.equal(y, whole.y) and torch.equal(force, whole.force)


def test_guards_and_reset():
    fx = _sub(load_npz("relax_per_system.npz"), "ring_")
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    tr = _Fixed()
    # the C entry refuses early_stop_batch handles
    lib, h = L.load(), C.c_void_p()
    L.check(lib.adf_lbfgs_create(int(b.pos.shape[0]), 4, 5, 0.04, 1.0, 70.0, 1, C.byref(h)))
    assert lib.adf_lbfgs_set_per_system(h, 1) == L.ADF_EINVAL and b"early_stop_batch" in lib.adf_last_error()
    lib.adf_lbfgs_destroy(h)
    with pytest.raises(ValueError, match="early_stop_batch"):
        LBFGS(b, TorchCalc(tr), memory=5, device=DEV, early_stop_batch=True, per_system=True)
    # a default-mode handle has no step state; the mode cannot change after a step
    plain = LBFGS(b, TorchCalc(tr), maxstep=0.04, memory=5, damping=1.0, alpha=70.0, device=DEV)
    plain.fmax = float(fx["fmax"])
    plain._setup()
    with pytest.raises(ValueError, match="per-system"):
        plain.step_state()
    _forced_step(plain, tr, 0, torch.from_numpy(fx["forces"][0]).to(DEV))
    with pytest.raises(ValueError, match="stepped"):
        plain.set_per_system(True)
    plain.close()
    b.pos.copy_(torch.from_numpy(fx["pos_in"]).to(DEV))
    opt = _optimizer(b, fx, tr)
    for k in range(8):
        _forced_step(opt, tr, k, torch.from_numpy(fx["forces"][k]).to(DEV))
    with pytest.raises(ValueError, match="stepped"):
        opt.set_per_system(False)
    assert opt.step_state()[0].tolist() == fx["masks"][:8].sum(0).tolist()
    # reset: counters back to zero, and the first fixture steps replay
    opt.reset()
    assert opt.step_state()[0].tolist() == [0, 0, 0, 0]
    b.pos.copy_(torch.from_numpy(fx["pos_in"]).to(DEV))
    for k in range(4):
        _forced_step(opt, tr, k, torch.from_numpy(fx["forces"][k]).to(DEV))
        assert ulp_close(b.pos, fx["pos_after"][k]), k
    opt.close()


SHARD_WORKER = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from adsorbdiff_amd.ml_relaxation import ml_relax_sharded
from tests.helpers import batch_from_fixture
from tests.test_gpu_relax_per_system import _painn

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", timeout=__import__("datetime").timedelta(seconds=120))
fx, tr = _painn()
b = batch_from_fixture(fx, pos_key="pos_in", device="cuda:0")
calls = []
real = dist.all_gather
dist.all_gather = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
out = ml_relax_sharded(b, tr, int(fx["steps"]), float(fx["fmax"]), {"memory": int(fx["memory"]), "per_system": True}, False,
                       rank=rank, world=world, device="cuda:0")
dist.all_gather = real
torch.save({"pos": out.pos.cpu(), "y": out.y.cpu(), "force": out.force.cpu(), "sid": out.sid, "collectives": len(calls),
            "untouched": bool(torch.equal(b.pos.cpu(), torch.from_numpy(fx["pos_in"])))}, sys.argv[2] + str(rank))
dist.barrier()
dist.destroy_process_group()
"""


def test_ml_relax_sharded_two_ranks_on_one_gpu(tmp_path, painn_runs):
    """Two processes share cuda:0 (gloo: RCCL refuses two ranks on one device), each relaxes its shard and ONE all-gather
    hands both the whole batch in global order: the bits of the single per-system run."""
    import os
    import socket
    import subprocess
    import sys
    from pathlib import Path

    _, _, _, whole = painn_runs
    script = tmp_path / "worker.py"
    script.write_text(SHARD_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), str(Path(__file__).resolve().parent.parent),
                                       str(tmp_path / "out")], env=env))
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    for r in range(2):
        got = torch.load(tmp_path / f"out{r}")
        assert got["collectives"] == 1 and got["sid"] == whole.sid and got["untouched"]
        assert torch.equal(got["pos"], whole.pos.cpu()) and torch.equal(got["y"], whole.y.cpu())
        assert torch.equal(got["force"], whole.force.cpu())


def test_nan_force_stays_inside_its_system():
    """A NaN force clears its system's mask, as in the default mode; here that system is then left alone and, since no dot
    product crosses systems, the others step exactly as they do without it (the coupled recursion would hand them NaN)."""
    fx = _sub(load_npz("relax_per_system.npz"), "ring_")
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    tr = _Fixed()
    opt = _optimizer(b, fx, tr)
    n0 = int(fx["natoms"][0])
    for k in range(3):
        f = torch.from_numpy(fx["forces"][k]).to(DEV)
        if k > 0:
            f[n0 - 1, 1] = float("nan")       # the last atom of system 0 (a free adsorbate atom)
        _forced_step(opt, tr, k, f)
        assert opt.update_mask().tolist() == [int(k == 0), 1, 1, 1], k
        if k == 0:
            first = b.pos[:n0].clone()
        assert torch.equal(b.pos[:n0], first), k      # system 0 took its one step and is left alone afterwards
        assert ulp_close(b.pos[n0:], fx["pos_after"][k][n0:]), k
    steps, absmax = (t.cpu() for t in opt.step_state())
    assert steps.tolist() == [1, 3, 3, 3] and float(absmax[0]) == -1.0
    assert bool(torch.isfinite(opt.last_step_max())) and bool(torch.isfinite(b.pos).all())
    opt.close()
