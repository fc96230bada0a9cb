"""train() on the device: a run stopped, saved and resumed retraces the uninterrupted run to the bit (both trainers), the
reproducible step gives bit-equal gradients, the defaults still build FusedAdamW and run the parent's code path, and two
ranks on one GPU end with the same parameters while only rank 0 writes."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd.train_step import FusedAdamW, MultiTensorAdamW, PaiNNTrainStep
from tests import helpers_train as HT
from tests import helpers_train_loop as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent


def test_reproducible_step_gives_bit_equal_gradients_embedding_included():
    m = HT.make_config_model("ragged").to(DEV)
    b = HT.make_config_batch("ragged").to(DEV)
    targets = HT.make_targets(int(b.natoms.numel()))
    step = PaiNNTrainStep(m, DEV, igso3=HT.igso3_tables()[0])
    assert step.ordered_embedding_backward is False
    step.zero_grad()
    step.loss_and_grad(b, targets)
    atomic = m.atom_emb.embeddings.weight.grad.clone()
    step.ordered_embedding_backward = True
    runs = []
    for _ in range(2):
        step.zero_grad()
        step.loss_and_grad(b, targets)
        runs.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert "atom_emb.embeddings.weight" in runs[0]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    # the same gradient as the atomic kernel's up to summation order, and nothing in the rows of absent elements
    emb = runs[0]["atom_emb.embeddings.weight"]
    assert float((emb - atomic).abs().max()) <= 1e-5 * float(atomic.abs().max())
    absent = HT.absent_embedding_rows(m, b)
    assert int(absent.sum()) > 0 and float(emb.cpu()[absent].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["denoising", "s2ef"])
def test_resumed_run_retraces_the_uninterrupted_run_bit_for_bit(kind, tmp_path):
    def batches():   # fresh objects for every run, as a loader hands them out
        train = H.batches_for(kind, DEV)
        return train, H.batches_for(kind, DEV)[:2]

    # run A: all 8 steps
    a = H.make_trainer(kind, tmp_path / "a", DEV)
    assert isinstance(a.optimizer, MultiTensorAdamW) and a.train_engine.ordered_embedding_backward
    a.train(*batches())
    want = H.training_state(a)
    assert want["step"] == 8 and want["applied"] == 8
    # run B: stops after 5 steps and saves; a new trainer and model load the file and train to the end
    b = H.make_trainer(kind, tmp_path / "b", DEV, max_steps=5)
    b.train(*batches())
    assert b.step == 5 and b.optimizer.counters()["applied"] == 5
    path = b.save()
    mid = H.training_state(b)
    del b
    c = H.make_trainer(kind, tmp_path / "b", DEV)
    c.load_checkpoint(path)
    H.assert_same_state(H.training_state(c), mid)
    c.train(*batches())
    got = H.training_state(c)
    assert got["lr"] != mid["lr"] and got["best_val_metric"] is not None and got["best_val_metric"] > 0
    if kind == "denoising":
        assert got["noise_step"] == 8 + 2 * 2   # 8 training steps and two validations of two batches
    H.assert_same_state(got, want)
    assert (tmp_path / "a" / "best_checkpoint.pt").exists()


def test_defaults_build_fused_adamw_and_run_the_same_code_path():
    from adsorbdiff_amd.exponential_moving_average import ExponentialMovingAverage
    from adsorbdiff_amd.trainer import DenoisingTrainer

    tables = HT.igso3_tables()[0]
    batch = HT.make_config_batch("ragged").to(DEV)
    targets = HT.make_targets(int(batch.natoms.numel()))
    for k, v in targets.items():
        setattr(batch, k, v.to(DEV))
    tr = DenoisingTrainer(HT.make_config_model("ragged"), device=DEV)
    tr.setup_training(H.NOISE, lr=1e-3, clip_grad_norm=1e9, tables=tables)
    assert type(tr.optimizer) is FusedAdamW and tr.train_engine.ordered_embedding_backward is False
    # the same step driven by hand: the step object and FusedAdamW, as before this loop existed
    m2 = HT.make_config_model("ragged").to(DEV)
    eng = PaiNNTrainStep(m2, DEV, igso3=tables)
    ema2 = ExponentialMovingAverage(m2.parameters(), 0.999)
    opt2 = FusedAdamW(m2, lr=1e-3, weight_decay=0.001, max_grad_norm=1e9, ema=ema2)
    # one step: the embedding gradient of this path is summed with float atomics, so a second step starts from weights
    # that may differ in their last bits
    out = tr.train_step(batch.clone(), noised=True)
    eng.zero_grad()
    loss2 = eng.loss_and_grad(batch.clone(), {k: getattr(batch, k) for k in HT.TARGET_KEYS})
    norm2 = opt2.step()
    assert not out["skipped"] and torch.equal(out["loss"], loss2)
    # clipping inactive: the other quantity summed with float atomics (the norm) does not reach the parameters
    assert abs(float(out["grad_norm"]) - float(norm2)) <= 1e-5 * float(norm2)
    emb = "atom_emb.embeddings.weight"
    for (k, p), q in zip(tr.model.named_parameters(), m2.parameters()):
        if k == emb:
            assert float((p - q).abs().max()) <= 1e-6 * float(q.abs().max())
        else:
            assert torch.equal(p, q), k
    assert tr.step == 1
    for s1, s2 in zip(tr.ema.shadow_params, ema2.shadow_params):
        assert float((s1 - s2).abs().max()) <= 1e-6 * float(s2.abs().max())


WORKER = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from tests import helpers_train_loop as H

rank = int(os.environ["RANK"])
dist.init_process_group("gloo")
tr = H.make_trainer("denoising", sys.argv[2], "cuda:0", max_steps=3, checkpoint_every=3, max_epochs=1)
batches = H.batches_for("denoising", "cuda:0")
tr.train(batches[rank::2] + batches[rank::2], None)     # two ranks, each its own batches: 4 per epoch
assert tr.step == 3
torch.save({k: p.detach().cpu() for k, p in tr.model.named_parameters()}, os.path.join(sys.argv[2], f"params{rank}.pt"))
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_on_one_gpu_train_to_equal_parameters_and_rank_zero_writes(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    out = tmp_path / "run"
    out.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), str(ROOT), str(out)], env=env))
    assert [p.wait(timeout=600) for p in procs] == [0, 0]
    p0, p1 = torch.load(out / "params0.pt"), torch.load(out / "params1.pt")
    assert set(p0) == set(p1)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    assert sorted(f.name for f in out.iterdir()) == ["checkpoint.pt", "params0.pt", "params1.pt"]   # one file, from rank 0
    ckpt = torch.load(out / "checkpoint.pt", map_location="cpu", weights_only=False)
    assert ckpt["step"] == 3 and float(ckpt["optimizer"]["state"][0]["step"]) == 3.0
