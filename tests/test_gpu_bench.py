"""bench.py's command line: a plain run reports the timed passes only and `--dump-outputs` writes what the last of them
returned; `--full` adds the measurements that take runs of their own."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def _bench(*args):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--systems", "6", "--num-steps", "3"] + list(args)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_sites(tmp_path):
    a = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["higher_is_better"] is True
    assert abs(a["value"] - 6 * 1e3 / a["ms_per_step"]) < 1e-6 * a["value"]
    for key in ("roofline", "measured_peaks", "cpu_baseline", "eqv2", "train", "exact_f32", "b1_latency"):
        assert key not in a, key
    sites = np.load(tmp_path / "a" / "sites.npy")
    assert sites.dtype == np.float32 and sites.shape == (6, 4, 3)
    assert hashlib.sha256(np.nan_to_num(sites).tobytes()).hexdigest()[:16] == a["sites_sha256_16"]
    # seeded inputs: another run (other step counts) returns the same sites bit for bit
    b = _bench("--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "b"))
    assert b["steps"] == 1 and np.array_equal(np.load(tmp_path / "b" / "sites.npy"), sites)


def test_full_line_carries_the_roofline():
    f = _bench("--steps", "1", "--warmup", "1", "--full", "--no-secondary", "--no-cpu-baseline")
    assert f["roofline"]["bound"] == "mfma" and f["roofline"]["achieved"] > 0 and f["measured_peaks"]["mfma_f16_tflops"] > 0
    assert f["recomputed_row_fraction_per_step"] is not None
