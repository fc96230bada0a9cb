#!/usr/bin/env python
"""Benchmark of the hot path: diffusion-sampled adsorbate sites per second.

One bench "step" = one complete pass of the sampler over the rank's batch of synthetic
OC20-Dense-shaped systems: initial placement, then `--num-steps` (50) reverse steps of
(periodic graph build -> PaiNN forward -> ODE update), i.e. BASELINE.json configs[1]
("PaiNN denoiser, 50-step sampling on 1000 synthetic OC20-Dense systems (~200 atoms, 10 A
cutoff), 1xMI355X").  Inputs are resident in HBM before the timed region starts.

    python bench.py --gpus 1 --steps 2 --warmup 1
    python bench.py --gpus 8                      # starts its own 8 ranks (one process per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Multi-GPU (BASELINE.json configs[2]: "the same 1000-system batch sharded 8 ways"): systems are independent, so
every rank samples its shard with no data-path collective; the only exchange is one all_gather of the sampled
adsorbate sites at the end of every pass (inside the timed region; RCCL over xGMI).  Default `--scaling strong`:
the `--systems` systems are dealt to the ranks by atom count (`sampler.shard_batch`, the reference's
balanced_partition, datasets/data_parallel.py:32-48) and the gathered sites come back in global system order;
`--scaling weak` gives every rank `--systems` systems of its own.  When WORLD_SIZE is not set and --gpus N > 1,
this process never touches the GPU: it starts N children (RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* set), relays rank 0's
JSON line and exits non-zero if any child fails.

Rank 0 prints ONE JSON line.  A plain run only sets up, warms up, times the `--steps` passes and reports them
(`value`, `ms_per_step`, the site digest, per-category GPU time of the timed passes).  `--full` adds everything else
the benchmark measures or checks, each with runs of its own:
  "roofline":     dominant kernel (fused message kernel, f32 MFMA bound), timed live with HIP
                  events on the launch stream inside the library (adf_profile_*), against on-box peaks
                  and the HBM traffic of two `rocprofv3 --pmc` child runs,
  secondaries:    default API, incremental layers off, trajectory sink, 125 systems, B = 1 latency,
                  exact f32 (N=1 only), and the EquiformerV2 and training lines of the same build,
  "cpu_baseline": the CPU oracle (oracle/painn_oracle.py, a PyTorch restatement of the
                  reference path) timed on the host cores on a bounded sample (N=1 only).

    python bench.py --gpus 1 --steps 2 --warmup 1 --full

`--dump-outputs DIR` writes what the last timed step returned (the sampled sites; for `--mode train` the loss, the
gradient norm and a fixed sample of the updated parameters) as DIR/<name>.npy; the inputs are seeded, so two builds
can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

METRIC = "sampled adsorbate sites/sec (50 denoise steps, ~200-atom slabs)"
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: Peak FP32 (matrix), dense
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: Peak BF16/FP16 MFMA, dense
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("painn", "eqv2"), default="painn",
                    help="painn = BASELINE config 2/3 (the headline); eqv2 = config 4 (EquiformerV2 denoiser, L_max = 6)")
    ap.add_argument("--mode", choices=("sample", "train"), default="sample",
                    help="sample = the headline (reverse-diffusion sampling); train = BASELINE config 5: one score-matching "
                         "training step (PaiNN, --systems graphs per GPU, weak scaling, gradient all-reduce over RCCL)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 2 sampling passes; 10 training steps)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps before them (default 1; 3 training steps)")
    ap.add_argument("--systems", type=int, default=None,
                    help="systems per rank (weak) or in total (strong); default 1000 (painn) / 128 (eqv2)")
    ap.add_argument("--num-steps", type=int, default=50, help="reverse-diffusion steps per sample")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="strong")
    ap.add_argument("--gather", choices=("torch", "rccl"), default="torch",
                    help="exchange step: torch.distributed.all_gather (nccl backend = RCCL) or the library's own "
                         "C-ABI adf_allgather_sites (RCCL communicator created by the library)")
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: roofline (live traffic probe, on-box peaks), the secondary passes, the "
                         "embedded EquiformerV2 and training lines and the CPU baseline (off: only what `value` needs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the default-API (adsorbate-only outputs), exact-f32 and other extra passes")
    ap.add_argument("--no-incremental", action="store_true",
                    help="PaiNN: recompute every node row of every layer at every step, as the reference does "
                         "(denoising_pos_params['incremental_layers']=False) - timed like the default, warm-up included")
    ap.add_argument("--cpu-full", action="store_true",
                    help="CPU baseline at SURVEY 8d's sizes (8 systems x 50 steps and 64 x 1 step; ~10 min); implies --full")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-traffic-probe", action="store_true",
                    help="skip the two rocprofv3 --pmc child runs that measure roofline.traffic (then the committed "
                         "profiles/message_kernel_pmc.json value is reported and labelled static)")
    ap.add_argument("--traffic-probe-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--random-init-heads", action="store_true",
                    help="PaiNN: keep the heads' last linear map at its random-init scale (rounds 1-3 headline: most "
                         "adsorbates stop moving after step ~33 and the incremental layers skip them)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for "
                                                      "testing the N>1 path with several ranks on one GPU)")
    a = ap.parse_args()
    if a.cpu_full:
        a.full = True
    if a.systems is None:
        a.systems = 256 if a.mode == "train" else (1000 if a.model == "painn" else 128)
    if a.mode == "train":
        if a.model != "painn":
            raise SystemExit("bench.py --mode train: the training step exists for the PaiNN denoiser (config 5)")
    if a.steps is None:
        a.steps = 10 if a.mode == "train" else 2
    if a.warmup is None:
        a.warmup = 3 if a.mode == "train" else 1
    return a


def launch_ranks(args) -> int:
    """Parent of an N-rank run.  Must not initialise the GPU (no torch.cuda call, no exec): it only starts one
    child per rank and waits.  Rank 0's stdout (the JSON line) is relayed; any failing child fails the run."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve())] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out0, _ = procs[0].communicate()
    codes = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out0.decode())
    sys.stdout.flush()
    if any(codes):
        print(f"bench.py: rank exit codes {codes}", file=sys.stderr)
        return 1
    return 0


def cpu_baseline(model_sd, scale_factors, params, full=False):
    """Time the CPU oracle (kind "port": oracle/painn_oracle.py, checked equal to the imported reference by
    oracle/make_golden.py) on bounded samples of the same workload: a throughput sample (many systems, 1 reverse
    step) and a loop sample (few systems, consecutive steps).  SURVEY 8d's sizes (64 x 1 and 8 x 50) with --cpu-full."""
    import torch

    from adsorbdiff_amd.synthetic import make_batch
    from oracle import painn_oracle as O

    def run(n_sys, n_steps):
        b = make_batch(n_sys, seed=1000)
        torch.manual_seed(0)
        noise = torch.rand(n_sys, 3)
        pos = O.initial_placement(b.pos.clone(), b.cell, b.tags, b.batch, noise)
        t0 = time.perf_counter()
        for t in range(n_steps):
            f1, f2 = O.painn_forward(model_sd, pos, b.atomic_numbers, b.cell, b.natoms, cutoff=10.0, max_neighbors=50,
                                     scale_factors=scale_factors)
            pos, _, _, _ = O.reverse_step(pos, b.cell, b.tags, b.batch, f1, f2, b.fixed, t, params)
        dt = time.perf_counter() - t0
        return {"systems": n_sys, "reverse_steps": n_steps, "seconds": round(dt, 2),
                "system_steps_per_s": n_sys * n_steps / dt}

    # SURVEY 8d names 64 x 1 and 8 x 50 (about 10 min on the box's host cores: --cpu-full, committed once per round under
    # profiles/); the default run is bounded to ~35 s of CPU work so that the whole bench line stays within a few minutes:
    # 16 systems x 1 step and 2 systems x 6 consecutive steps (the rate of 16 x 1 equals that of 32 x 1 to 1 %: BENCH_r04 / r05).  BOTH rates are reported; `value` is the throughput
    # sample's (the batched workload), not the better of the two.
    wide = run(64, 1) if full else run(16, 1)
    loop = run(8, params["num_steps"]) if full else run(2, 6)
    return {
        "value": wide["system_steps_per_s"] / params["num_steps"],
        "unit": "sites/s",
        "cores": torch.get_num_threads(),
        "kind": "port",
        "throughput_sample_sites_per_s": wide["system_steps_per_s"] / params["num_steps"],
        "loop_sample_sites_per_s": loop["system_steps_per_s"] / params["num_steps"],
        "sample": "%d systems x 1 reverse step in %.1f s (%.3f system-steps/s) and %d systems x %d consecutive steps "
                  "in %.1f s (%.3f system-steps/s); value = the FIRST rate / %d steps per site, i.e. LINEARLY "
                  "EXTRAPOLATED to the 1000-system x %d-step workload (SURVEY 8d's sizes, 64 x 1 and 8 x 50: --cpu-full)" % (
                      wide["systems"], wide["seconds"], wide["system_steps_per_s"], loop["systems"],
                      loop["reverse_steps"], loop["seconds"], loop["system_steps_per_s"], params["num_steps"],
                      params["num_steps"]),
        "samples": [wide, loop],
    }


TRAFFIC_PROBE = {}


def traffic_probe(args):
    """roofline.traffic, measured for THIS build on THIS box: two child runs of this file under `rocprofv3 --pmc`
    (FETCH_SIZE and WRITE_SIZE need separate passes; no tracing flags beside --pmc), each sampling the first two reverse
    steps of the same 1000-system batch (12 message launches, those of the cold first step at full size).  HBM bytes per
    full-size launch of the message kernel = 2 x FETCH_SIZE + WRITE_SIZE (MI355X_MICROARCH.md, HBM: FETCH_SIZE counts
    half the bytes of wide reads on gfx950; the unit is KB), calibrated in the same runs on the library's 1 GiB stream
    copy (adf_measure_peaks).  Runs BEFORE this process touches the GPU (children are started, never exec'ed into)."""
    import csv
    import glob
    import shutil
    import tempfile

    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if Path("/opt/rocm/bin/rocprofv3").exists() else None)
    if exe is None:
        TRAFFIC_PROBE["error"] = "rocprofv3 not found"
        return
    if os.environ.get("ROCP_TOOL_LIBRARIES") or "rocprof" in os.environ.get("LD_PRELOAD", "") or \
            os.environ.get("ROCPROFILER_REGISTER_FORCE_LOAD"):
        # this process itself runs under a profiler: its children would inherit the tool environment and nest profilers
        TRAFFIC_PROBE["error"] = "skipped: bench.py itself runs under rocprofv3 (static figure reported)"
        return
    t_start = time.perf_counter()
    res = {}
    tmp = tempfile.mkdtemp(prefix="adf_pmc_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--pmc", counter, "-d", d, "-o", "p", "--output-format", "csv", "--", sys.executable,
                   str(Path(__file__).resolve()), "--traffic-probe-child", "--systems", str(args.systems)]
            env = dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp"))
            r = subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                TRAFFIC_PROBE["error"] = "%s pass failed (rc %d): %s" % (counter, r.returncode, r.stderr.decode()[-300:])
                return
            msg, cal = [], []
            for f in files:
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        if row["Counter_Name"] != counter:
                            continue
                        if "adf_message_kernel" in row["Kernel_Name"] and "<true, false" in row["Kernel_Name"].replace("(bool)1, (bool)0", "true, false"):
                            msg.append(float(row["Counter_Value"]))
                        elif "adf_peak_copy_kernel" in row["Kernel_Name"]:
                            cal.append(float(row["Counter_Value"]))
            if not msg:
                TRAFFIC_PROBE["error"] = "no message-kernel dispatches in the %s pass" % counter
                return
            full = [v for v in msg if v > 0.5 * max(msg)]
            res[counter] = (sum(full) / len(full) * 1024.0, len(full), (sum(cal) / len(cal) * 1024.0) if cal else None)
    except Exception as e:
        TRAFFIC_PROBE["error"] = repr(e)
        return
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fr, wr = res["FETCH_SIZE"], res["WRITE_SIZE"]
    TRAFFIC_PROBE.update(
        hbm_bytes_per_launch=2.0 * fr[0] + wr[0], fetch_size_bytes_raw=fr[0], write_size_bytes=wr[0], full_size_launches=fr[1],
        calibration_copy_1GiB={"fetch_raw_bytes": fr[2], "write_bytes": wr[2]}, seconds=round(time.perf_counter() - t_start, 1),
        source="live: two `rocprofv3 --pmc` child runs of this command's first two reverse steps (FETCH_SIZE, WRITE_SIZE in "
               "separate passes), 2*FETCH_SIZE + WRITE_SIZE averaged over the %d full-size launches of "
               "adf_message_kernel<f16x3, vec != 0>; FETCH_SIZE doubled per MI355X_MICROARCH.md (the 1 GiB stream copy of the "
               "same runs reads FETCH %.3g / WRITE %.3g bytes)" % (fr[1], fr[2] or 0.0, wr[2] or 0.0))


def dump_outputs(directory, arrays):
    """--dump-outputs: every array as DIR/<name>.npy, float64 kept, anything else as float32."""
    import numpy as np

    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        np.save(d / f"{name}.npy", a if a.dtype == np.float64 else a.astype(np.float32))


def traffic_probe_child(args):
    """The program rocprofv3 runs for traffic_probe(): the first two reverse steps of the benchmark batch + the peak kernels."""
    import torch

    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.synthetic import make_batch
    from adsorbdiff_amd.trainer import DenoisingTrainer

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = bench_painn_model(args)
    trainer = DenoisingTrainer(model, device=dev)
    b = make_batch(args.systems, seed=1000).to(dev)
    torch.manual_seed(0)
    params = dict(num_steps=2, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                  early_stop=False, placement_noise=torch.rand(args.systems, 3))
    Denoiser(b, DiffTorchCalc(trainer), params, device=str(dev)).run()
    model.engine(dev).measure_peaks()
    torch.cuda.synchronize(dev)


HEAD_GAIN = 100.0


def bench_painn_model(args=None):
    """The benchmark's PaiNN: reference architecture and initialisers under seed 0 + the shipped scale factors.  With the
    bare random-init heads the scores are so small that, as sigma shrinks along the schedule, most adsorbates stop moving
    by a representable amount after step ~33 and the incremental layers then skip those systems - which a trained model
    would not allow.  Since round 4 the HEADLINE therefore uses the stall-free workload: the last linear map of both
    heads (out_forces / out_forces2 .output_network[1].vec2_proj) scaled by HEAD_GAIN, so that every system keeps moving
    through step 49 (the per-step recomputed-row fraction is printed in the JSON line).  --random-init-heads restores
    the rounds 1-3 workload."""
    import torch

    from adsorbdiff_amd.painn_denoising import PaiNN
    from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS

    torch.manual_seed(0)
    model = PaiNN(None, 50, 1, hidden_channels=512, num_layers=6, num_rbf=128, cutoff=10.0, max_neighbors=50,
                  scale_file=PAINN_NB6_SCALE_FACTORS, so3_denoising=True).eval()
    if args is None or not args.random_init_heads:
        with torch.no_grad():
            for hname in ("out_forces", "out_forces2"):
                getattr(model, hname).output_network[1].vec2_proj.weight.mul_(HEAD_GAIN)
    return model


def painn_roofline(prof, counters, f16, useful_rows, measured):
    """--full: the roofline of the message kernel over the timed passes (`prof`, `counters`: the library's HIP-event
    profile and device counters of those passes) against the nominal and the on-box peaks (`measured`)."""
    H, R = 512, 128
    E = counters.num_edges
    N_atoms = counters.num_atoms
    msg_ms, msg_launches = prof["message"]
    products = 3 if f16 else 1  # f16x3 split issues three MFMA products per contraction step
    peak = PEAK_F16_MFMA_TFLOPS if f16 else PEAK_F32_MFMA_TFLOPS
    # incremental layers: a launch evaluates only the targets whose inputs changed; per-launch averages of the
    # edges and targets actually evaluated (device-side totals of the last pass, adf_get_counters)
    inc_on = counters.inc_msg_launches > 0
    E_launch = counters.inc_msg_edges / counters.inc_msg_launches if inc_on else float(E)
    T_launch = counters.inc_rows / counters.inc_msg_launches if inc_on else float(N_atoms)
    dense_flops_per_launch = 2.0 * R * 3 * H * E_launch
    # message_ksteps = sum over 32-edge blocks of (contracted k length x 32-column blocks that ran: 6, or 4 in the vec == 0
    # launches of layer 0, whose xb columns are skipped)
    issued_flops_per_launch = prof["message_ksteps"] * 32 * 32 * 2.0 * products / max(msg_launches, 1)
    avg_s = msg_ms * 1e-3 / max(msg_launches, 1)
    issued = issued_flops_per_launch / avg_s / 1e12 if avg_s > 0 else 0.0
    dense_equiv = dense_flops_per_launch / avg_s / 1e12 if avg_s > 0 else 0.0
    gathered_bytes = E_launch * 5 * H * 4.0  # per edge: the source's gather record (xa, xc, P0, P1, P2 per channel), from L2
    # fused kernel (no rbfh): per edge geometry + index, per target x / vec in and out
    hbm_alg_bytes = E_launch * (12 + 8) + T_launch * (4 * H * 4.0 + 4 * H * 4.0)
    traffic = traffic_src = None
    pmc = ROOT / "profiles" / "message_kernel_pmc.json"
    if TRAFFIC_PROBE.get("hbm_bytes_per_launch"):
        traffic = TRAFFIC_PROBE["hbm_bytes_per_launch"]
        traffic_src = TRAFFIC_PROBE["source"]
    elif pmc.exists():  # no live probe (rocprofv3 missing / --no-traffic-probe): the committed result, labelled static
        try:
            traffic = json.loads(pmc.read_text()).get("hbm_bytes_per_launch")
            traffic_src = "static: profiles/message_kernel_pmc.json (separate rocprofv3 --pmc FETCH_SIZE / " \
                          "WRITE_SIZE passes of this command, 2*FETCH+WRITE per full-size launch); not measured in this run"
        except Exception:
            traffic = None
    peak_meas = measured["mfma_f16_tflops"] if f16 else measured["mfma_f32_tflops"]
    roofline = {
        "kernel": "adf_message_kernel (fused rbf-projection MFMA + gather + segmented sum), %s mode"
                  % ("f16x3-split" if f16 else "exact-f32"),
        "bound": "mfma",
        "achieved": issued,
        "peak": peak,
        "unit": "TFLOP/s",
        "frac": issued / peak,
        "useful_row_share": useful_rows,
        "achieved_useful_rows": issued * useful_rows if useful_rows else None,
        "frac_useful_rows": issued * useful_rows / peak if useful_rows else None,
        "measured_peak": peak_meas,
        "frac_of_measured_peak": issued / peak_meas if peak_meas > 0 else None,
        "traffic": traffic,
        "traffic_source": traffic_src,
        "traffic_probe_seconds": TRAFFIC_PROBE.get("seconds"),
        "avg_launch_ms": avg_s * 1e3,
        "launches": msg_launches,
        "flops_per_launch": issued_flops_per_launch,
        "dense_equivalent_tflops": dense_equiv,
        "algorithmic_f16x3_tflops": dense_equiv * products,
        "l2_gather_tbps": gathered_bytes / avg_s / 1e12 if avg_s > 0 else 0.0,
        "hbm_algorithmic_gbps": hbm_alg_bytes / avg_s / 1e9 if avg_s > 0 else 0.0,
        "hbm_algorithmic_frac": (hbm_alg_bytes / avg_s / 1e9) / PEAK_HBM_GBS if avg_s > 0 else 0.0,
        "note": "achieved = matrix-core flops the kernel issues (k-window x 32 rows x the 32-column blocks that run x 2 "
                "per 32-edge row block, padded rows and the 3 split products included) / launch time from HIP events on the "
                "launch stream. This is the conservative count: the algorithm's dense contraction (SURVEY 8d: "
                "2*R*3H*E per layer, x3 products in this arithmetic = algorithmic_f16x3_tflops) is ~1.9x larger, "
                "the k-window skips Gaussian terms below 1.5e-8 of the leading one. useful_row_share = edges / (32 x "
                "row blocks) of this batch's graph (the last block of a target is padded to 32 rows); "
                "achieved_useful_rows / frac_useful_rows count only the real rows of the issued products. Timed on the "
                "launch stream; measured_peak = the same MFMA instruction in a register-resident loop on this "
                "box (non-zero operands). rbfh is never materialised, so neither SURVEY 8d roofline binds alone: "
                "per 32-edge block the kernel issues ~560 vector instructions (8 FMA per gathered channel-row) "
                "beside ~54 MFMAs and 10 KB/edge of L2-served record gathers (l2_gather_tbps); on gfx950 the "
                "matrix-pipe time and the vector-issue time of the two waves of a SIMD ADD "
                "(profiles/r05_mfma_valu_overlap.txt), which puts this formulation's floor at ~0.42 of nominal - "
                "see DESIGN.md 4.",
    }
    if TRAFFIC_PROBE.get("error"):
        roofline["traffic_probe_error"] = TRAFFIC_PROBE["error"]
    return {"roofline": roofline, "measured_peaks": measured}


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args))  # before anything touches the GPU
    if args.traffic_probe_child:
        return traffic_probe_child(args)
    if (args.full and args.gpus == 1 and args.model == "painn" and args.mode == "sample" and not args.no_traffic_probe
            and not args.no_secondary and "ADF_GEMM" not in os.environ and "ADF_MSG" not in os.environ):
        traffic_probe(args)  # children under rocprofv3 --pmc, before this process touches the GPU
    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (the HIP path has no CPU fallback)")
    ndev = torch.cuda.device_count()
    if args.backend == "nccl" and local_rank >= ndev:
        raise SystemExit(f"LOCAL_RANK={local_rank} but only {ndev} GPU(s) visible")
    dev = torch.device("cuda", local_rank % ndev)
    torch.cuda.set_device(dev)
    import torch.distributed as dist

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    if args.mode == "train":
        return main_train(args, rank, world, dev)
    if args.model == "eqv2":
        return main_eqv2(args, rank, world, dev)

    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.painn_denoising import PaiNN
    from adsorbdiff_amd.sampler import gather_sites, shard_batch, shard_bounds
    from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS
    from adsorbdiff_amd.synthetic import make_batch
    from adsorbdiff_amd.trainer import DenoisingTrainer

    # random-init weights of the reference architecture under seed 0 (+ shipped scale factors)
    model = bench_painn_model(args)
    cpu_sd = {k: v.clone() for k, v in model.state_dict().items()} if rank == 0 and args.full else None
    scale_factors = model.scale_factors()
    trainer = DenoisingTrainer(model, device=dev)

    bounds = None
    if args.scaling == "weak":
        n_local = args.systems
        batch0 = make_batch(n_local, seed=1000 + rank, sid_offset=rank * args.systems).to(dev)
        my_ids = [rank * args.systems + i for i in range(n_local)]
        bounds = (n_local, 4)  # every rank: the same number of systems, 4-atom adsorbates
    else:
        # the SAME synthetic batch on every rank count (seed 1000), dealt by atom count like the reference does
        full = make_batch(args.systems, seed=1000)
        if world > 1:
            batch0, my_ids = shard_batch(full, rank, world)
            bounds = shard_bounds(full, world)  # every rank derives the exchange buffer's shape locally: ONE all_gather
        else:
            batch0, my_ids = full, list(range(args.systems))
        n_local = len(my_ids)
        batch0 = batch0.to(dev) if n_local else None   # (more ranks than systems: this rank only joins the exchange)
    total_systems = args.systems * world if args.scaling == "weak" else args.systems
    # `value` stays on the full-output path (every atom's model outputs at every step) for round-to-round comparability;
    # what Denoiser.run() does without options since round 5 (outputs of the adsorbate atoms only inside the fused loop:
    # nothing else is observable there) is timed as the secondary `value_default_api`
    params = dict(num_steps=args.num_steps, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55,
                  ode=True, early_stop=False, scores_on_adsorbate_only=False)
    if args.no_incremental:
        params["incremental_layers"] = False
    eng = model.engine(dev)
    # initial-placement uniforms keyed by global system id: an N-rank strong-scaling run samples exactly the sites
    # of the 1-rank run (the reference draws torch.rand(B,3) per process, denoising_torch.py:215)
    torch.manual_seed(0)
    placement = torch.rand(total_systems, 3)[torch.tensor(my_ids, dtype=torch.long)]

    def one_pass(extra=None):
        if batch0 is None:
            empty = torch.empty(0, 1, 3, device=dev)
            return gather_sites(None, world, via=args.gather, system_ids=my_ids, bounds=bounds, local=empty)
        b = batch0.clone()
        torch.manual_seed(0)
        den = Denoiser(b, DiffTorchCalc(trainer), dict(params, placement_noise=placement, **(extra or {})),
                       device=str(dev))
        live["den"] = den
        out = den.run()
        assert den.steps_applied == args.num_steps, den.steps_applied
        return gather_sites(out, world, via=args.gather, system_ids=my_ids, bounds=bounds)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    rows_log = []
    live = {}
    # reverse steps after which the hooked warm-up passes keep the adsorbate sites (f16x3 here, exact f32 below): the
    # divergence curve of the two arithmetics along the schedule (`exact_f32.site_difference_curve`)
    CURVE_STEPS = sorted({s_ for s_ in (1, 2, 5, 10, 20, 30, 40, args.num_steps) if s_ <= args.num_steps})
    curve16, curve32 = {}, {}

    def keep_sites(t, store):
        if t + 1 in CURVE_STEPS:
            bb = live["den"].batch
            store[t + 1] = bb.pos[bb.tags == 2].detach().clone()

    def hook(t):  # diagnostic (untimed warm-up pass only): per-step host read of the incremental layers' totals
        c_ = eng.counters()
        rows_log.append((int(c_.inc_rows), int(c_.inc_rows_full)))
        keep_sites(t, curve16)

    for i in range(args.warmup):
        one_pass({"step_hook": hook} if args.full and i == 0 and rank == 0 and not args.no_incremental else None)
    row_frac = []
    for i, (r, f) in enumerate(rows_log):
        r0, f0 = rows_log[i - 1] if i and rows_log[i - 1][0] <= r else (0, 0)
        row_frac.append(round((r - r0) / max(f - f0, 1), 3))
    eng.profile_enable(True)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sites = one_pass()
    fence()
    elapsed = time.perf_counter() - t0
    rank_ms = None
    if world > 1:
        # every rank's own time over the timed passes (its clock stops when ITS last all_gather returned) and its GPU-busy
        # time: the first real multi-GPU run then shows the curve and where its imbalance comes from in one line
        busy = sum(v[0] for v in eng.profile_read().values() if isinstance(v, tuple))
        t = torch.tensor([elapsed * 1e3 / args.steps, busy / args.steps, float(n_local), float(batch0.pos.shape[0] if batch0 is not None else 0)],
                         dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        rank_ms = [[round(float(v), 2) for v in a.tolist()] for a in allt]
        elapsed = max(a[0] for a in rank_ms) * args.steps / 1e3
    prof = eng.profile_read()
    eng.profile_enable(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"sites": sites})
    counters = eng.counters() if batch0 is not None else None   # (rank 0 always holds systems)
    # share of the message kernel's 32-row blocks that are real edges (a target's in-edges are processed 32 rows at a
    # time; the last block of a target is padded): from the in-degrees of the batch's own graph
    useful_rows = None
    if args.full and rank == 0 and batch0 is not None:
        try:
            eng.build_graph(batch0)
            ed_ = eng.export_graph()[4]
            deg_ = torch.bincount(ed_.long(), minlength=int(batch0.pos.shape[0]))
            useful_rows = float(deg_.sum()) / float(32 * ((deg_ + 31) // 32).sum())
            del ed_, deg_
        except Exception as e:   # diagnostics only
            useful_rows = None
            print(f"bench.py: useful-row share not measured ({e!r})", file=sys.stderr)

    # Secondary measurement, N = 1 only, never `value`: the same pass with the model outputs evaluated on the
    # adsorbate atoms only (the stepper reads nothing else; sampled positions are bit-identical, checked here).
    ads_only = exact_f32 = all_rows = small = traj_sink = b1_latency = None
    if args.full and world == 1 and not args.no_secondary:
        one_pass({"incremental_layers": False})   # untimed: the switch frees the 22 GB of kept layer state
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        sites_full = one_pass({"incremental_layers": False})
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t1
        all_rows = {"value": total_systems / dt, "unit": "sites/s", "ms_per_step": dt * 1e3,
                    "identical_sites": bool(torch.equal(sites_full, sites)),
                    "note": "denoising_pos_params['incremental_layers']=False: every node row of every layer recomputed "
                            "at every step, as the reference does; one timed pass after one untimed (the first pass after "
                            "the switch also frees the 22 GB of kept layer state; timed alone it read 192-216 sites/s over "
                            "the boxes of round 5), not part of `value` (`--no-incremental` times it like the default)"}
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        one_pass({"scores_on_adsorbate_only": None})   # untimed: back to incremental layers (kept state re-allocated)
        eng.profile_enable(True)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(2):
            sites_ads = one_pass({"scores_on_adsorbate_only": None})
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t1) / 2
        prof_ads = eng.profile_read()
        eng.profile_enable(False)
        ads_only = {"value": total_systems / dt, "unit": "sites/s", "ms_per_step": dt * 1e3,
                    "identical_sites": bool(torch.equal(sites_ads, sites)),
                    "gpu_ms_per_pass": {k: round(v[0] / 2, 2) for k, v in prof_ads.items() if isinstance(v, tuple)},
                    "note": "Denoiser(...).run() WITHOUT options, as a caller of the reference's API invokes it: inside the fused "
                            "loop (adf_sample / adf_sample_traj) the per-atom model outputs never leave the library, so since "
                            "round 5 the last layer's message targets, its update and the heads are evaluated for the tag-2 "
                            "atoms only (adf_painn_forward_subset; bit-identical sites, checked here); 2 timed passes after 1 "
                            "untimed; `value` itself stays on the full-output path (scores_on_adsorbate_only=False)"}
        # The reference's default call keeps every frame (ml_relaxation.py:134-149: save_full_traj=True + traj_dir): one pass
        # with the asynchronous sink (csrc/frames.hip + trajectory.py), timed until run() returns (every file written).
        import shutil
        import tempfile

        tdir = tempfile.mkdtemp(prefix="adf_traj_", dir=os.environ.get("TMPDIR", "/tmp"))
        try:
            b = batch0.clone()
            torch.manual_seed(0)
            den = Denoiser(b, DiffTorchCalc(trainer), dict(params, placement_noise=placement, trajectory_async=True),
                           device=str(dev), traj_dir=tdir, traj_names=[str(i) for i in my_ids], save_full_traj=True)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            sites_tr = gather_sites(den.run(), 1)
            torch.cuda.synchronize(dev)
            dt_sample = time.perf_counter() - t1
            den.wait_for_trajectories()
            dt_all = time.perf_counter() - t1
            nbytes = sum(f.stat().st_size for f in Path(tdir).iterdir())
            traj_sink = {"value": total_systems / dt_sample, "unit": "sites/s", "ms_per_step": dt_sample * 1e3,
                         "value_until_files_complete": total_systems / dt_all, "ms_until_files_complete": dt_all * 1e3,
                         "frames": args.num_steps, "files": len(list(Path(tdir).iterdir())), "bytes_written": nbytes,
                         "identical_sites": bool(torch.equal(sites_tr, sites)),
                         "note": "save_full_traj=True + traj_dir: adf_sample_traj pushes the positions after every reverse "
                                 "step through a pinned host ring to a writer thread (one batch file streamed during the "
                                 "loop, then <sid>.npz per system); value = until the sampler returns (frames still being "
                                 "written behind it), value_until_files_complete = until every file exists; one pass, not "
                                 "part of `value`"}
        finally:
            shutil.rmtree(tdir, ignore_errors=True)
        # What one GPU of an 8-way strong-scaling run of the 1000-system batch sees: 125 systems (same generator).
        if args.systems >= 250:
            b125 = make_batch(125, seed=1000).to(dev)
            pl125 = placement[:125]

            def pass125():
                b = b125.clone()
                torch.manual_seed(0)
                den = Denoiser(b, DiffTorchCalc(trainer), dict(params, placement_noise=pl125), device=str(dev))
                return gather_sites(den.run(), 1)

            pass125()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(2):
                pass125()
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t1) / 2
            small = {"value": 125 / dt, "unit": "sites/s", "ms_per_step": dt * 1e3, "systems": 125,
                     "note": "the per-GPU share of an 8-way split of the 1000-system batch (BASELINE config 3) run on this one "
                             "GPU: 2 timed passes after 1 warm-up; 8 x this value / `value` = the strong-scaling efficiency to "
                             "expect at 8 GPUs (the only collective is one all_gather of 60 KB per pass)"}
        # The reference's only PUBLISHED number is a latency: reverse steps per second of one structure through its
        # calculator (examples/valID_sample/val_sample.ipynb:191: 100/100 steps at 36.9 it/s; NRR_example-gemnet.ipynb:
        # 31-41 it/s; hardware not named there).  The same call here: Denoiser.run() without options on ONE system of the
        # benchmark batch, 100-step schedule, early stop off and on (the reference's default), and on 64 systems.
        def latency(nsys, early):
            bl = make_batch(nsys, seed=1000).to(dev)
            pl = dict(num_steps=100, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, ode=True,
                      early_stop=early)

            def run_l():
                torch.manual_seed(0)
                d_ = Denoiser(bl.clone(), DiffTorchCalc(trainer), pl, device=str(dev))
                d_.run()
                torch.cuda.synchronize(dev)
                return d_.steps_applied

            run_l()
            t1_ = time.perf_counter()
            n_ = run_l() + run_l()
            dt_ = time.perf_counter() - t1_
            return {"reverse_steps_per_s": round(n_ / dt_, 1), "ms_per_step": round(dt_ / max(n_, 1) * 1e3, 3),
                    "steps_applied_per_run": n_ // 2, "systems": nsys, "early_stop": bool(early)}

        b1_latency = {"B1": latency(1, False), "B1_early_stop": latency(1, True), "B64": latency(64, False),
                      "unit": "reverse steps/s (it/s) through Denoiser.run(), 100-step schedule, benchmark model "
                              "(H=512 x 6, 10 A, K=50), 200-atom systems; 2 timed runs after 1 warm-up each",
                      "reference_published": "36.9 it/s at B = 1 (examples/valID_sample/val_sample.ipynb:191, 100 steps; "
                                             "hardware unnamed), 31-41 it/s (examples/NRR/NRR_example-gemnet.ipynb:124-197)"}
        # Reference-width arithmetic: every matrix-core product in exact f32 (v_mfma_f32_32x32x2_f32; ADF_GEMM=f32 is read
        # when a handle is created, so a second model + engine with the same weights).  Warm: 1 untimed + 2 timed passes.
        if "ADF_GEMM" not in os.environ and "ADF_MSG" not in os.environ:
            os.environ["ADF_GEMM"] = "f32"
            try:
                model32 = bench_painn_model(args)
                trainer32 = DenoisingTrainer(model32, device=dev)

                def pass32(extra=None):
                    b = batch0.clone()
                    torch.manual_seed(0)
                    den = Denoiser(b, DiffTorchCalc(trainer32), dict(params, placement_noise=placement, **(extra or {})),
                                   device=str(dev))
                    live["den"] = den
                    return gather_sites(den.run(), 1)

                # the untimed warm-up pass runs step by step and keeps the sites after CURVE_STEPS, like the f16x3 warm-up did
                pass32({"step_hook": (lambda t: keep_sites(t, curve32))} if curve16 else None)
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                for _ in range(2):
                    sites32 = pass32()
                torch.cuda.synchronize(dev)
                dt = (time.perf_counter() - t1) / 2
                # Sites are compared under the MINIMUM-IMAGE convention: the stepper wraps the centre of mass into the cell
                # (reference denoising_torch.py:298-309, `fractional %= 1`), so two arithmetics that differ by 1e-6 A next
                # to a cell face land one lattice vector apart - the same site.  The raw difference is printed beside it.
                bsys = batch0.batch[batch0.tags == 2]
                cell_a = batch0.cell.reshape(-1, 3, 3)[bsys].double()

                def min_image(d):   # d [n_ads, 3] -> the shortest equivalent vector (the cells are far from skewed enough
                    fr = torch.linalg.solve(cell_a.transpose(1, 2), d.double().unsqueeze(-1)).squeeze(-1)   # to need a search)
                    fr = fr - torch.round(fr)
                    return torch.einsum("ni,nij->nj", fr, cell_a)

                def wrap_image(d):   # modulo the vectors the STEPPER wraps by: the reference solves cell . f = com and maps f % 1
                    # back with cell . f (denoising_torch.py:298-309), i.e. it wraps along the COLUMNS of `cell` - for the
                    # benchmark's skewed cells ([a,0,0],[0.3a,0.95a,0],[0,0,35]) not lattice vectors: a wrap that one arithmetic
                    # takes and the other does not (centre of mass within 1e-6 of f = 0) leaves (0, 0.3 a, 0) = 4.6 A modulo
                    # the true lattice.  Quirk reproduced on purpose; this metric removes exactly those vectors.
                    fr = torch.linalg.solve(cell_a, d.double().unsqueeze(-1)).squeeze(-1)
                    fr = fr - torch.round(fr)
                    return torch.einsum("nij,nj->ni", cell_a, fr)

                d_end = sites32.reshape(-1, 3).to(dev) - sites.reshape(-1, 3).to(dev)
                dev_max = float(d_end.abs().max())
                dev_max_mi = float(min_image(d_end).abs().max())
                curve = {}
                for st in CURVE_STEPS:
                    if st in curve16 and st in curve32:
                        dd = curve32[st] - curve16[st]
                        mi = min_image(dd).abs().amax(dim=1)
                        wi = wrap_image(dd).abs().amax(dim=1)
                        curve[str(st)] = {"max_minimum_image": float(mi.max()), "max_modulo_wrap_vectors": float(wi.max()),
                                          "median": float(mi.median()),
                                          "p99": float(torch.quantile(mi, 0.99)),
                                          "sites_above_1e-3": int((mi > 1e-3).sum()),
                                          "worst_system": int(bsys[int(mi.argmax())]),
                                          "max_raw": float(dd.abs().max())}
                exact_f32 = {"value": total_systems / dt, "unit": "sites/s", "ms_per_step": dt * 1e3,
                             "max_abs_site_difference_vs_f16x3_angstrom": dev_max_mi,
                             "max_abs_site_difference_raw_angstrom": dev_max,
                             "max_abs_site_difference_modulo_wrap_vectors_angstrom": float(wrap_image(d_end).abs().max()),
                             "site_difference_curve": curve,
                             "site_difference_note": "per reverse step (key): |site(exact f32) - site(f16x3)| over the 4000 "
                                 "adsorbate atoms of the batch, both runs free-running from the same placement; minimum image "
                                 "= modulo the cell's lattice vectors (the stepper wraps the centre of mass into the cell, so "
                                 "a 1e-6 A difference next to a cell face is one lattice vector, ~14.5 A, in the raw number); "
                                 "modulo_wrap_vectors = modulo the COLUMNS of the cell, the vectors the reference's wrap actually "
                                 "shifts by (denoising_torch.py:298-309; not lattice vectors of the skewed benchmark cells): a wrap "
                                 "taken by one arithmetic only leaves (0, 0.3 a, 0) = 4.6 A under the minimum image and ~0 here",
                             "note": "ADF_GEMM=f32: exact-f32 MFMA (v_mfma_f32_32x32x2_f32) in every GEMM and in the "
                                     "message kernel; 2 timed passes after 1 untimed warm-up pass (weight packing and "
                                     "allocation excluded, like `value`); not part of `value`"}
                model32.engine(dev).close()
                del model32, trainer32
            finally:
                del os.environ["ADF_GEMM"]

    if rank == 0:
        assert sites.shape[0] == total_systems, (sites.shape, total_systems)
        assert bool(torch.isfinite(sites).all())
        E = counters.num_edges
        f16 = os.environ.get("ADF_MSG", os.environ.get("ADF_GEMM", "f16")) != "f32"
        inc_on = counters.inc_msg_launches > 0
        gpu_ms = {k: round(v[0] / args.steps, 2) for k, v in prof.items() if isinstance(v, tuple)}
        import hashlib

        sites_digest = hashlib.sha256(torch.nan_to_num(sites).cpu().numpy().tobytes()).hexdigest()[:16]
        out = {
            "metric": METRIC,
            "value": total_systems * args.steps / elapsed,
            "unit": "sites/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32" if not f16 else "f32 (f16x3-split MFMA, fp32 accumulate; ADF_GEMM=f32 selects exact f32)",
            "data": "synthetic",
            "config": {
                "workload": "PaiNN denoiser (H=512, 6 layers, R=128, K=50), %d-step ODE sampling on %d synthetic "
                            "OC20-Dense systems (200 atoms, 10 A cutoff) per GPU" % (args.num_steps, n_local),
                "systems_total": total_systems,
                "systems_per_gpu": n_local,
                "num_reverse_steps": args.num_steps,
                "atoms_per_system": 200,
                "edges_per_system": round(E / max(n_local, 1), 1),
                "weights": ("reference initialisers, seed 0, shipped scale factors" if args.random_init_heads else
                            "reference initialisers, seed 0, shipped scale factors; last linear map of both heads x %g so that "
                            "every adsorbate keeps moving through the last step (stall-free workload, see "
                            "recomputed_row_fraction_per_step)" % HEAD_GAIN),
                "parallelism": "systems sharded over %d GPU(s) by atom count, no data-path collective, one all_gather "
                               "of sites per pass (%s)" % (world, "adf_allgather_sites, RCCL" if args.gather == "rccl"
                                                           else "torch.distributed %s" % args.backend),
                "loop_invariant_reuse": "slab-slab top-K candidates and layer-0 gather records (functions of the static "
                                        "slab / atomic numbers only) are computed at the first of the 50 steps of each "
                                        "pass and reused; every pass starts cold; bit-identical to recomputing "
                                        "(denoising_pos_params['static_atom_cache']=False)",
                "incremental_layers": ("on: per-layer node state is kept across the steps of a pass and a row is recomputed "
                                       "only if one of its inputs changed (new graph compared bit for bit with the previous "
                                       "one, flags propagated along the edges); %.1f %% of the layer x atom rows were "
                                       "recomputed in the last pass; bit-identical sites (see incremental_layers_off)"
                                       % (100.0 * counters.inc_rows / max(counters.inc_rows_full, 1))) if inc_on else "off",
            },
            "sites_sha256_16": sites_digest,  # equal for every --gpus N under --scaling strong (same systems, same noise)
            "per_rank": None if rank_ms is None else {
                "ms_per_step": [a[0] for a in rank_ms], "gpu_busy_ms_per_step": [a[1] for a in rank_ms],
                "systems": [int(a[2]) for a in rank_ms], "atoms": [int(a[3]) for a in rank_ms],
                "imbalance_max_over_mean": round(max(a[0] for a in rank_ms) / (sum(a[0] for a in rank_ms) / len(rank_ms)), 4),
                "note": "wall time of each rank over the timed passes (barrier to its own last all_gather), the GPU time of its "
                        "kernels (HIP events), and its share of the batch; `ms_per_step` of the line is the maximum"},
            "system_steps_per_s": total_systems * args.steps * args.num_steps / elapsed,
            "gpu_ms_per_pass": gpu_ms,
        }
        if args.full:
            out.update(painn_roofline(prof, counters, f16, useful_rows, eng.measure_peaks()))
            out.update({
                "recomputed_row_fraction_per_step": row_frac or None,  # warm-up pass: layer x atom rows recomputed / all rows
                "incremental_layers_off": all_rows,
                "value_at_125_systems": small,
                "with_trajectory_sink": traj_sink,
                "value_default_api": ads_only,
                "exact_f32": exact_f32,
                "b1_latency": b1_latency,
            })
        if args.full and world == 1 and not args.no_secondary:
            # BASELINE configs 4 and 5 in the same line (bounded: 64 systems x 50 steps; 5 training steps), so that one
            # `bench.py --gpus 1 --full` run times them too.  Each is the object its own mode prints with --full.
            eng.close()
            del trainer
            torch.cuda.empty_cache()
            import copy

            a4 = copy.copy(args)
            a4.model, a4.systems, a4.steps, a4.warmup, a4.no_secondary, a4.no_cpu_baseline = "eqv2", 64, 1, 1, True, args.no_cpu_baseline
            a4.scaling, a4.warmup_num_steps, a4.dump_outputs = "strong", 3, None
            try:
                out["eqv2"] = main_eqv2(a4, rank, world, dev, emit=False)
            except Exception as e:  # never lose the headline to a secondary
                out["eqv2"] = {"error": repr(e)}
            torch.cuda.empty_cache()
            a5 = copy.copy(args)
            a5.mode, a5.systems, a5.steps, a5.warmup, a5.dump_outputs = "train", 256, 5, 2, None
            try:
                out["train"] = main_train(a5, rank, world, dev, emit=False)
            except Exception as e:
                out["train"] = {"error": repr(e)}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cpu_sd, scale_factors, params, full=args.cpu_full)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main_train(args, rank, world, dev, emit=True):
    """BASELINE config 5: conditional-training step of the PaiNN denoiser (score-matching loss, forward + backward) on
    OC20-IS2RE-shaped graphs, one process per GPU (weak scaling: `--systems` ~200-atom graphs per GPU and step), gradients
    averaged by a bucketed all-reduce (backend nccl = RCCL over xGMI).  A "step" = noising + forward + loss + backward +
    all-reduce + clip + AdamW + EMA on one synthetic batch resident in HBM."""
    import torch
    import torch.distributed as dist

    from adsorbdiff_amd.painn_denoising import PaiNN
    from adsorbdiff_amd.scaling import PAINN_NB6_SCALE_FACTORS
    from adsorbdiff_amd.so3_tables import Igso3Tables
    from adsorbdiff_amd.synthetic import make_batch
    from adsorbdiff_amd.trainer import DenoisingTrainer

    torch.manual_seed(0)
    model = PaiNN(None, 50, 1, hidden_channels=512, num_layers=6, num_rbf=128, cutoff=10.0, max_neighbors=50,
                  scale_file=PAINN_NB6_SCALE_FACTORS, so3_denoising=True)
    tr = DenoisingTrainer(model, device=dev)
    tr.setup_training(dict(ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55), lr=1e-4,
                      tables=Igso3Tables.shared())
    batch = make_batch(args.systems, seed=2000 + rank).to(dev)
    import numpy as np

    np.random.seed(2000 + rank)  # the rotation noise of every step draws from numpy's global stream: same inputs every run

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        out = tr.train_step(batch.clone())
    tr.allreduce_wait_events = []
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = tr.train_step(batch.clone())
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ar_events = getattr(tr, "allreduce_wait_events", [])
    ar_ms = sum(a.elapsed_time(b) for a, b in ar_events) / max(len(ar_events), 1)
    if args.dump_outputs and rank == 0:
        # the updated parameters (21 M values) through a fixed, seeded sample of 2^20 of them, in storage order
        flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
        pick = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(0))[:1 << 20].sort().values
        arrays = {"loss": out["loss"], "parameters_sample": flat[pick.to(flat.device)]}
        if out.get("grad_norm") is not None:
            arrays["grad_norm"] = out["grad_norm"]
        dump_outputs(args.dump_outputs, arrays)
    if rank == 0:
        H, R, L, n, E = 512, 128, 6, 200, 10100  # per graph: 200 atoms, ~10.1 k symmetrised edges
        fwd = L * (30 * H * H * n + 2 * R * 3 * H * E) + 2 * 1.6e9 / 2  # 34.6 GFLOP per graph forward
        step_flops = 3.0 * fwd * args.systems  # forward + data-gradient + weight-gradient products
        rbf_flops = L * 2 * R * 3 * H * E * args.systems   # rbf_proj's contraction over the edges (69 % of the forward's flops)
        # issued matrix-core products per dense product: forward 3 (f16x3), data gradients 3, weight gradients 6 (three-term
        # bf16 split) except rbf_proj's, which runs as two fp16 terms with column lifts (3) since round 5
        issued_flops = (3.0 + 3.0 + 6.0) * fwd * args.systems - 3.0 * rbf_flops
        graphs = args.systems * world * args.steps
        grad_bytes = sum(p.numel() for p in model.parameters() if p.requires_grad) * 4
        train_traffic = train_traffic_src = None
        pmc = ROOT / "profiles" / "train_step_pmc.json"
        if pmc.exists():  # separate rocprofv3 --pmc passes of this command (profiles/scripts): bytes per graph x this batch
            try:
                j = json.loads(pmc.read_text())
                train_traffic = j["hbm_bytes_per_step_and_graph"] * args.systems
                train_traffic_src = "static: profiles/train_step_pmc.json (%s); not measured in this run" % j.get("source", "")
            except Exception:
                train_traffic = None
        out_line = {
            "metric": "score-matching training graphs/sec (PaiNN H=512 x 6, ~200-atom OC20-shaped graphs, forward + backward + "
                      "all-reduce + AdamW + EMA)",
            "value": graphs / elapsed, "unit": "graphs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (forward and data-gradient products f16x3-split MFMA with per-row lifts, weight-gradient products "
                     "three-term bf16 split, 6 MFMA products - rbf_proj's: two fp16 terms with per-column lifts, 3 products; "
                     "ADF_WGRAD=f32: exact-f32 MFMA for the node weight gradients)", "data": "synthetic",
            "config": {"workload": "BASELINE config 5: PaiNN score-matching step, %d graphs x 200 atoms per GPU and step"
                                   % args.systems,
                       "graphs_per_gpu_and_step": args.systems,
                       "parallelism": "one process per GPU; gradient all-reduce (%s) in buckets issued from inside the backward "
                                      "(heads, then layer by layer) and overlapped with it, %d ranks" % (args.backend, world)},
            "loss": float(out["loss"].reshape(-1)[0]),
            "grad_norm": float(out["grad_norm"]) if out.get("grad_norm") is not None else None,
            "allreduce_wait_ms_per_step": ar_ms if world > 1 else 0.0,  # what the backward did not hide
            "gradient_bytes": grad_bytes,
            "roofline": {"kernel": "whole step: dense products of forward + backward",
                         "bound": "mfma",
                         "achieved": issued_flops * args.steps / elapsed / 1e12,
                         "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": issued_flops * args.steps / elapsed / 1e12 / PEAK_F16_MFMA_TFLOPS,
                         "dense_equivalent_tflops": step_flops * args.steps / elapsed / 1e12,
                         "traffic": train_traffic, "traffic_source": train_traffic_src,
                         "note": "achieved = issued split products per GPU: 3 x the forward's dense flops (SURVEY 8d: 34.6 GFLOP "
                                 "per graph; forward + data-gradient + weight-gradient products) x the MFMA products per dense "
                                 "product (f16x3: 3; weight gradients bf16x6: 6, rbf_proj's two-term fp16 with column lifts: 3) "
                                 "/ wall time per step, priced against the f16 matrix "
                                 "peak the products run on - an UPPER bound of what is issued (the message block's contraction "
                                 "skips the Gaussian terms outside its k-window).  dense_equivalent_tflops is the reference's "
                                 "dense f32 arithmetic over the same time (not a fraction of any peak: the split products run "
                                 "on the f16-rate cores).  Per kernel: profiles/r0*_train_* (MfmaUtil, HBM bytes)"},
        }
        if not emit:
            return out_line
        print(json.dumps(out_line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


EQV2_HP = dict(max_neighbors=20, max_radius=12.0, max_num_elements=90, num_layers=8, sphere_channels=128,
               attn_hidden_channels=64, num_heads=8, attn_alpha_channels=64, attn_value_channels=16,
               ffn_hidden_channels=128, norm_type="layer_norm_sh", lmax_list=[6], mmax_list=[2], grid_resolution=18,
               edge_channels=128, attn_activation="silu", ffn_activation="silu", use_grid_mlp=True, use_sep_s2_act=True,
               alpha_drop=0.0, drop_path_rate=0.0, weight_init="uniform", so3_denoising=True, FOR_denoising=True)


def eqv2_batch(n, seed, sid_offset=0):
    """The synthetic OC20-Dense batch of the PaiNN bench; slab elements without a tabulated atomic radius (Kr, Xe: the
    reference's EquiformerV2 returns NaN for them, equiformer_v2_denoising.py:165-213) are replaced by Ag."""
    from adsorbdiff_amd.synthetic import make_batch

    b = make_batch(n, seed=seed, sid_offset=sid_offset)
    z = b.atomic_numbers.clone()
    z[(z == 36) | (z == 54)] = 47.0
    b.atomic_numbers = z
    return b


def eqv2_cpu_baseline(model, params):
    """CPU oracle of the EquiformerV2 forward (oracle/eqv2_oracle.py, kind "port") on ONE system x ONE reverse step."""
    import torch

    from oracle import eqv2_oracle as Q

    b = eqv2_batch(1, seed=1000)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    hp = dict(lmax=6, mmax=2, num_layers=EQV2_HP["num_layers"], sphere_channels=128, attn_hidden_channels=64, num_heads=8,
              attn_alpha_channels=64, attn_value_channels=16, ffn_hidden_channels=128, grid_resolution=18,
              max_radius=12.0, max_neighbors=20)
    t0 = time.perf_counter()
    with torch.no_grad():
        Q.eqv2_forward(sd, hp, b.pos, b.atomic_numbers, b.cell, b.natoms)
    dt = time.perf_counter() - t0
    return {"value": 1.0 / dt / params["num_steps"], "unit": "sites/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": "1 system x 1 reverse step (model forward only) in %.1f s = %.3f system-steps/s; value = that rate / "
                      "%d steps per site, LINEARLY EXTRAPOLATED" % (dt, 1.0 / dt, params["num_steps"])}


def eqv2_roofline(prof, c, f16, forwards, dev):
    """--full: the roofline of the SO(2) convolution products over the timed passes (`prof`, `c`: the library's HIP-event
    profile and device counters of those passes) against the nominal and the on-box peaks."""
    import ctypes as C

    import torch

    from adsorbdiff_amd import lib as _lib

    conv_ms, conv_groups = prof["so2_conv"]
    products = 3 if f16 else 1
    conv_s = conv_ms * 1e-3
    # summed by the library over the profiled forwards (incremental blocks: a forward's convolutions run on the edges of
    # the targets it recomputes, which differs from forward to forward)
    assert c.forwards_total == forwards, (c.forwards_total, forwards)
    issued = c.conv_flops_total * products / conv_s / 1e12 if conv_s > 0 else 0.0
    pk = (C.c_float * 3)()   # (peaks come from the library, any handle)
    _lib.check(_lib.load().adf_measure_peaks(pk, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    measured = {"hbm_copy_gbps": float(pk[0]), "mfma_f16_tflops": float(pk[1]), "mfma_f32_tflops": float(pk[2])}
    total_gpu_s = sum(v[0] for v in prof.values()) * 1e-3
    conv_traffic = conv_traffic_src = None
    pmc = ROOT / "profiles" / "eqv2_conv_pmc.json"
    if pmc.exists():  # PMC counters need their own rocprofv3 passes: the committed result scaled to this run's edge count
        try:
            chunk = int(os.environ.get("ADF_EQV2_CHUNK_EDGES", 1 << 19))  # edges per launch: the engine's chunking
            per_launch = c.num_edges / max(1, -(-c.num_edges // chunk))
            conv_traffic = json.loads(pmc.read_text())["hbm_bytes_per_conv_launch_and_edge"] * per_launch
            conv_traffic_src = ("static: profiles/eqv2_conv_pmc.json (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes at "
                                "64 systems, 2*FETCH+WRITE per launch of the convolution product kernels and per edge) x this "
                                "run's edges per launch; not measured in this run")
        except Exception:
            conv_traffic = None
    return {
        "roofline": {
            "kernel": "eq_gemm16pw_kernel + eq_gemm16_256_kernel (SO(2) convolution products of the %d attention blocks, f16x3 split)"
                      % (EQV2_HP["num_layers"] + 2),
            "bound": "mfma",
            "achieved": issued, "peak": PEAK_F16_MFMA_TFLOPS if f16 else PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": issued / (PEAK_F16_MFMA_TFLOPS if f16 else PEAK_F32_MFMA_TFLOPS),
            "measured_peak": measured["mfma_f16_tflops"] if f16 else measured["mfma_f32_tflops"],
            "traffic": conv_traffic,
            "traffic_source": conv_traffic_src,
            "flops_per_forward": c.conv_flops_total * products / max(forwards, 1),
            "share_of_gpu_time": conv_s / total_gpu_s if total_gpu_s > 0 else None,
            "note": "achieved = 2 x multiply-adds of the SO(2) convolutions (5.83 M + 2.40 M per edge and block at this "
                    "configuration) x 3 split products / HIP-event time of the convolution launches on the launch "
                    "stream (includes the row-lift passes that feed them)",
        },
        "measured_peaks": measured,
    }


def main_eqv2(args, rank, world, dev, emit=True):
    """BASELINE config 4: EquiformerV2 denoiser (L_max = 6, M_max = 2, C = 128, 8 blocks, K = 20, 12 A: the shipped
    configs/denoising/eqv2_so3.yml with lmax 6), `--num-steps`-step ODE sampling on `--systems` synthetic systems."""
    import torch
    import torch.distributed as dist

    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.equiformer_v2_denoising import EquiformerV2S_OC20_DenoisingPos
    from adsorbdiff_amd.sampler import gather_sites, shard_batch, shard_bounds
    from adsorbdiff_amd.trainer import DenoisingTrainer

    torch.manual_seed(0)
    model = EquiformerV2S_OC20_DenoisingPos(None, None, None, **EQV2_HP).eval()
    trainer = DenoisingTrainer(model, device=dev)
    bounds = None
    if args.scaling == "weak":
        batch0 = eqv2_batch(args.systems, seed=1000 + rank, sid_offset=rank * args.systems).to(dev)
        my_ids = [rank * args.systems + i for i in range(args.systems)]
        bounds = (args.systems, 4)
    else:
        full = eqv2_batch(args.systems, seed=1000)
        batch0, my_ids = shard_batch(full, rank, world) if world > 1 else (full, list(range(args.systems)))
        bounds = shard_bounds(full, world) if world > 1 else None
        batch0 = batch0.to(dev) if len(my_ids) else None   # (more ranks than systems: this rank only joins the exchange)
    n_local = len(my_ids)
    total_systems = args.systems * world if args.scaling == "weak" else args.systems
    # (`value`: full per-atom outputs, as in the PaiNN line; the default call is the `value_default_api` secondary)
    params = dict(num_steps=args.num_steps, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55,
                  ode=True, early_stop=False, scores_on_adsorbate_only=False)
    eng = model.engine(dev)
    torch.manual_seed(0)
    placement = torch.rand(total_systems, 3)[torch.tensor(my_ids, dtype=torch.long)]

    def one_pass(extra=None):
        if batch0 is None:
            return gather_sites(None, world, via=args.gather, system_ids=my_ids, bounds=bounds,
                                local=torch.empty(0, 1, 3, device=dev))
        b = batch0.clone()
        torch.manual_seed(0)
        den = Denoiser(b, DiffTorchCalc(trainer), dict(params, placement_noise=placement, **(extra or {})), device=str(dev))
        out = den.run()
        assert den.steps_applied == args.num_steps, den.steps_applied
        return gather_sites(out, world, via=args.gather, system_ids=my_ids, bounds=bounds)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    wsteps = getattr(args, "warmup_num_steps", None)  # embedded in the PaiNN line: a short warm-up pass
    for _ in range(args.warmup):
        if wsteps and batch0 is not None:
            b_ = batch0.clone()
            torch.manual_seed(0)
            Denoiser(b_, DiffTorchCalc(trainer), dict(params, num_steps=wsteps, placement_noise=placement), device=str(dev)).run()
        else:
            one_pass()
    # secondary (one pass): Denoiser.run() without options = the force blocks evaluated for the adsorbate atoms only
    # inside the fused loop (adf_eqv2_forward_subset)
    sites_ads, ads_s = None, 0.0
    if args.full and not args.no_secondary:
        fence()
        t0 = time.perf_counter()
        sites_ads = one_pass({"scores_on_adsorbate_only": None})
        fence()
        ads_s = time.perf_counter() - t0
    # secondary (one pass): every row of every block recomputed at every step, as the reference does
    sites_full, full_s = None, 0.0
    if args.full and not args.no_secondary:
        fence()
        t0 = time.perf_counter()
        sites_full = one_pass({"incremental_layers": False})
        fence()
        full_s = time.perf_counter() - t0
    eng.profile_enable(True)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sites = one_pass()
    fence()
    elapsed = time.perf_counter() - t0
    rank_ms = None
    if world > 1:
        # every rank's own time over the timed passes (its clock stops when ITS last all_gather returned) and its GPU-busy
        # time: the first real multi-GPU run then shows the curve and where its imbalance comes from in one line
        busy = sum(v[0] for v in eng.profile_read().values() if isinstance(v, tuple))
        t = torch.tensor([elapsed * 1e3 / args.steps, busy / args.steps, float(n_local), float(batch0.pos.shape[0] if batch0 is not None else 0)],
                         dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        rank_ms = [[round(float(v), 2) for v in a.tolist()] for a in allt]
        elapsed = max(a[0] for a in rank_ms) * args.steps / 1e3
    prof = eng.profile_read()
    eng.profile_enable(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"sites": sites})
    c = eng.counters() if batch0 is not None else None
    if rank == 0:
        assert sites.shape[0] == total_systems and bool(torch.isfinite(sites).all())
        forwards = args.steps * args.num_steps
        f16 = os.environ.get("ADF_GEMM") != "f32"
        gpu_ms = {k: round(v[0] / args.steps, 2) for k, v in prof.items()}
        import hashlib

        out = {
            "metric": METRIC,
            "value": total_systems * args.steps / elapsed,
            "unit": "sites/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32 (f16x3-split MFMA with per-row power-of-two lifts, fp32 accumulate)" if f16 else "f32",
            "data": "synthetic",
            "config": {
                "workload": "EquiformerV2 denoiser (BASELINE config 4: L_max=6, M_max=2, C=128, 8 blocks, 8 heads, K=20, "
                            "12 A), %d-step ODE sampling on %d synthetic OC20-Dense systems (200 atoms) per GPU"
                            % (args.num_steps, n_local),
                "systems_total": total_systems, "systems_per_gpu": n_local, "num_reverse_steps": args.num_steps,
                "atoms_per_system": 200, "edges_per_system": round(c.num_edges / max(n_local, 1), 1),
                "weights": "reference initialisers (uniform), seed 0",
                "parity": "unpinned S2-grid normalisation (e3nn stand-in), see DESIGN.md",
                "parallelism": "systems sharded over %d GPU(s) by atom count, one all_gather of sites per pass" % world,
            },
            "sites_sha256_16": hashlib.sha256(torch.nan_to_num(sites).cpu().numpy().tobytes()).hexdigest()[:16],
            "per_rank": None if rank_ms is None else {
                "ms_per_step": [a[0] for a in rank_ms], "gpu_busy_ms_per_step": [a[1] for a in rank_ms],
                "systems": [int(a[2]) for a in rank_ms], "atoms": [int(a[3]) for a in rank_ms],
                "imbalance_max_over_mean": round(max(a[0] for a in rank_ms) / (sum(a[0] for a in rank_ms) / len(rank_ms)), 4)},
            "system_steps_per_s": total_systems * forwards / elapsed,
            "dense_tflops_f32_equivalent": c.dense_flops * forwards / elapsed / 1e12,
            "gpu_ms_per_pass": gpu_ms,
            "recomputed_block_rows_fraction": round(c.inc_rows / c.inc_rows_full, 4) if c.inc_rows_full else 1.0,
        }
        if args.full:
            out.update(eqv2_roofline(prof, c, f16, forwards, dev))
        if sites_ads is not None:
            out["value_default_api"] = {
                "value": total_systems / ads_s, "unit": "sites/s", "identical_sites": bool(torch.equal(sites_ads, sites)),
                "note": "Denoiser(...).run() without options: inside the fused loop the two force blocks run for the tag-2 "
                        "target atoms only (adf_eqv2_forward_subset; the per-atom outputs never leave the library); one "
                        "pass, this rank's clock; `value` stays on the full-output path",
            }
        if sites_full is not None:
            out["incremental_layers_off"] = {
                "value": total_systems / full_s, "unit": "sites/s", "identical_sites": bool(torch.equal(sites_full, sites)),
                "note": "denoising_pos_params['incremental_layers']=False: every block recomputes every row at every step, as "
                        "the reference does; one pass, this rank's clock",
            }
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = eqv2_cpu_baseline(model, params)
        if not emit:
            eng.close()
            return out
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
