"""CPU tests of the per-system L-BFGS mode: the float64 statement of its contract (tests/helpers_lbfgs_per_system.py)
against the reference's one-system-alone records (tools/make_golden_relax_per_system.py), the keyword plumbing and the
exchange of a sharded relaxation (sampler.pack_relaxed / merge_packed_relaxed / gather_relaxed)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from adsorbdiff_amd import ml_relaxation as MR
from adsorbdiff_amd import sampler as S
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.lbfgs_torch import LBFGS
from adsorbdiff_amd.synthetic import make_batch
from tests.helpers import batch_from_fixture, load_npz
from tests.helpers_lbfgs_per_system import OneSystemLBFGS, max_force, split_systems, ulp_close


def _sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


@pytest.mark.parametrize("tag", ["ring", "skip"])
def test_contract_statement_reproduces_reference_alone(tag):
    """Every system stepped by the helper at the iterations where its own mask is set: the reference's masks, skip table,
    step counts, and positions within 1 f32 ulp after every iteration."""
    fx = _sub(load_npz("relax_per_system.npz"), tag + "_")
    b = batch_from_fixture(fx, pos_key="pos_in")
    natoms = fx["natoms"].tolist()
    pos = [p.clone() for p in split_systems(b.pos, natoms)]
    opts = [OneSystemLBFGS(int(fx["memory"]), float(fx["maxstep"]), float(fx["damping"]), float(fx["alpha"])) for _ in natoms]
    for k in range(fx["forces"].shape[0]):
        fs = split_systems(torch.from_numpy(fx["forces"][k]), natoms)
        for s, opt in enumerate(opts):
            on = bool(max_force(fs[s]) >= float(fx["fmax"]))
            assert on == bool(fx["masks"][k, s]), (k, s)
            assert bool(opt.step(pos[s], fs[s], on)) == bool(fx["skipped"][k, s]), (k, s)
        assert ulp_close(torch.cat(pos), fx["pos_after"][k]), k
    assert [o.t for o in opts] == fx["steps_taken"].tolist()


def test_fixture_holds_the_events_it_is_for():
    fx = load_npz("relax_per_system.npz")
    m = fx["ring_masks"]
    assert fx["ring_natoms"].tolist() == [12, 7, 1, 33] and int(fx["ring_memory"]) == 5 and m.shape == (20, 4)
    assert int(fx["ring_steps_taken"].max()) >= 7                                  # a ring wrapped
    assert any(m[0, s] and not m[10:, s].any() for s in range(4))                  # converged early for good
    assert any((not m[k, s]) and m[k + 1:, s].any() for s in range(4) for k in range(19))   # clear, then set again
    sk = fx["skip_skipped"]
    assert sk.sum() == 1 and sk[12, 1] and fx["skip_masks"].all()


class _StubLBFGS:
    seen = []

    def __init__(self, batch, calc, **kw):
        self.batch = batch
        _StubLBFGS.seen.append(kw)

    def run(self, fmax, steps):
        self.batch.y = torch.zeros(len(self.batch.sid))
        self.batch.force = torch.zeros_like(self.batch.pos)
        return self.batch


def test_relax_opt_per_system_reaches_the_optimizer(monkeypatch):
    monkeypatch.setattr(MR, "LBFGS", _StubLBFGS)
    b = make_batch(2, n_slab=4, n_ads=1, seed=3)
    _StubLBFGS.seen = []
    MR.ml_relax(b, None, 5, 0.05, {"memory": 7, "per_system": True}, False, device="cpu")
    assert _StubLBFGS.seen[-1]["per_system"] is True
    MR.ml_relax(b, None, 5, 0.05, {"memory": 7}, False, device="cpu")
    assert "per_system" not in _StubLBFGS.seen[-1]        # the default passes the reference's keywords only
    MR.ml_relax(b, None, 5, 0.05, {"memory": 7, "per_system": False}, False, device="cpu")
    assert "per_system" not in _StubLBFGS.seen[-1]


class _Calc:
    model = type("T", (), {"_unwrapped_model": type("M", (), {"otf_graph": True})()})()


def test_per_system_is_the_last_keyword_and_refuses_early_stop_batch():
    import inspect

    params = list(inspect.signature(LBFGS.__init__).parameters)
    assert params[-1] == "per_system" and params[-2] == "early_stop_batch"
    assert inspect.signature(LBFGS.__init__).parameters["per_system"].default is False
    b = make_batch(1, n_slab=4, n_ads=1, seed=3)
    with pytest.raises(ValueError, match="early_stop_batch"):
        LBFGS(b, _Calc(), memory=5, device="cpu", early_stop_batch=True, per_system=True)
    assert LBFGS(b, _Calc(), memory=5, device="cpu", per_system=True).per_system is True
    assert LBFGS(b, _Calc(), memory=5, device="cpu").per_system is False


def test_ml_relax_sharded_needs_per_system():
    b = make_batch(2, n_slab=4, n_ads=1, seed=3)
    for opt in ({"memory": 5}, {"memory": 5, "per_system": False}):
        with pytest.raises(ValueError, match="per_system"):
            MR.ml_relax_sharded(b, None, 5, 0.05, opt, False, rank=0, world=2, device="cpu")


def test_ml_relax_sharded_single_rank_undoes_the_split_order(monkeypatch):
    """world 1, a stand-in optimizer that fails above two systems: ml_relax returns its halves in the reference's order and
    ml_relax_sharded hands the batch back in the order it came in."""
    class Stub(_StubLBFGS):
        def run(self, fmax, steps):
            if len(self.batch.sid) > 2:
                raise RuntimeError("HIP out of memory")
            self.batch.pos = self.batch.pos + 1.0
            self.batch.y = torch.tensor([float(s) for s in self.batch.sid])
            self.batch.force = -self.batch.pos
            return self.batch

    monkeypatch.setattr(MR, "LBFGS", Stub)
    b = Batch.from_data_list(make_batch(3, n_slab=4, n_ads=1, seed=3).to_data_list()
                             + make_batch(2, n_slab=7, n_ads=2, seed=4, sid_offset=3).to_data_list())
    out = MR.ml_relax_sharded(b, None, 5, 0.05, {"memory": 5, "per_system": True}, False, rank=0, world=1, device="cpu")
    assert out.sid == b.sid and torch.equal(out.natoms, b.natoms)
    assert torch.equal(out.pos, b.pos + 1.0) and torch.equal(out.force, -(b.pos + 1.0))
    assert out.y.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


def _ragged_batch():
    """Five systems of 5, 5, 5, 9 and 9 atoms with relaxed-looking pos / y / force."""
    b = Batch.from_data_list(make_batch(3, n_slab=4, n_ads=1, seed=7).to_data_list()
                             + make_batch(2, n_slab=7, n_ads=2, seed=8).to_data_list())
    g = torch.Generator().manual_seed(5)
    b.y = torch.randn(5, generator=g)
    b.force = torch.randn(b.pos.shape[0], 3, generator=g)
    b.force[3, 1] = float("nan")           # a NaN payload must survive the bit-pattern transport
    return b


def _shard(full, ids):
    data = full.to_data_list()
    sub = Batch.from_data_list([data[i] for i in ids])
    offs = [0] + torch.cumsum(full.natoms, 0).tolist()
    sub.y = full.y[ids]
    sub.force = torch.cat([full.force[offs[i]:offs[i + 1]] for i in ids])
    return sub


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_pack_and_merge_round_trip_ragged_three_ranks_with_an_empty_one():
    full = _ragged_batch()
    natoms = full.natoms.tolist()
    bounds = (3, 9)
    deal = [[4, 0, 2], [], [3, 1]]         # ragged, out of order, one rank without systems
    msgs = [S.pack_relaxed(_shard(full, ids) if ids else None, ids, bounds) for ids in deal]
    for m in msgs:
        assert m.shape == (3, 2 + 6 * 9) and m.dtype == torch.int32
    assert msgs[1][:, 0].tolist() == [-1, -1, -1] and msgs[0][:, 0].tolist() == [4, 0, 2] and msgs[2][:, 0].tolist() == [3, 1, -1]
    # the padding of a 5-atom system's row is NaN
    assert bool(torch.isnan(msgs[0][1, 2 + 15:2 + 27].view(torch.float32)).all())
    pos, y, force = S.merge_packed_relaxed(torch.stack(msgs), natoms)
    assert _same_bits(pos, full.pos) and _same_bits(y, full.y) and _same_bits(force, full.force)
    with pytest.raises(ValueError, match="every system"):
        S.merge_packed_relaxed(torch.stack(msgs[:2]), natoms)
    with pytest.raises(ValueError, match="bounds"):
        S.pack_relaxed(_shard(full, [3, 4]), [3, 4], (2, 5))
    assert S.relaxed_bounds(natoms, 2) == (3, 9) and S.relaxed_bounds(natoms, 7) == (1, 9)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = _ragged_batch()
    mine, ids = S.shard_batch(full, rank, world)
    calls = {"n": 0}
    real = dist.all_gather

    def counting(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    dist.all_gather = counting
    pos, y, force = S.gather_relaxed(_shard(full, ids), ids, full.natoms.tolist(), world)
    dist.all_gather = real
    torch.save({"pos": pos, "y": y, "force": force, "ids": ids, "collectives": calls["n"]}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_relaxed_is_one_collective_in_global_order(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    full = _ragged_batch()
    res = [torch.load(tmp_path / f"r{r}.pt") for r in range(world)]
    assert sorted(res[0]["ids"] + res[1]["ids"]) == [0, 1, 2, 3, 4] and res[0]["ids"] and res[1]["ids"]
    for r in res:
        assert r["collectives"] == 1
        assert _same_bits(r["pos"], full.pos) and _same_bits(r["y"], full.y) and _same_bits(r["force"], full.force)
