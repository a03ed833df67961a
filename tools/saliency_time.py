#!/usr/bin/env python3
"""Cost of the gradient x input attributions (paths_amd.saliency.input_gradients, csrc/path_rows.hip) at the headline shape: 8
slides at K = 2048 x 5 levels, dropout off.  One JSON line:

    input_gradients_ms      one whole pass (forward recursion, backward without weight gradients, dX, row reductions)
    forward_backward_ms     utils.forward_backward (forward + the full training backward) on the same batch, same process,
                            alternating rounds (A/B/A/B); ratio = input_gradients / forward_backward
    rows_us_per_level       paths_saliency_rows of every level alone, event-timed on an otherwise idle device, with its algorithmic
                            bytes (2 M D 4 in, 8 M out) and the rate they give
    dx_gemm_us_per_level    the dX = dG W_gates[:, :D] + dY product of every level's shape alone, event-timed

    python tools/saliency_time.py [--limit 420] [--steps 10] [--rounds 4]

The measurement runs in a fresh child process under ``timeout -k 10 <limit>``."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attribution_timing as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--limit", type=int, default=420, help="seconds for the child process")
ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
ap.add_argument("--steps", type=int, default=10, help="passes per timed run")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

if not args.child:
    T.run_in_child(__file__, args.limit, ["--steps", args.steps, "--rounds", args.rounds, "--warmup", args.warmup])

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import backward as bw  # noqa: E402
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch  # noqa: E402
from paths_amd.saliency import input_gradients  # noqa: E402

K, SPG = 2048, 8
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, 0.0)
keep, L = cfg.top_k_patches, cfg.num_levels
slides = [DeviceSlide.synthetic(bench.CPU_DSEED, i, bench.BASE_SHAPES[K], device=dev) for i in bench.CPU_SLIDE_IDS[K][:SPG]]
sb = DeviceSlideBatch(slides)
labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
batch = {"slide": sb, "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
D = sb.dim


def run_saliency(steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out, trace = input_gradients(model, sb, keep, L)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run_train(steps):
    model.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.zero_grad(set_to_none=True)
        putils.forward_backward(model, batch, L, keep)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    model.zero_grad(set_to_none=True)
    model.eval()
    return ms


runs = {"input_gradients": run_saliency, "forward_backward": run_train}
for name in runs:
    runs[name](args.warmup)
ms = T.alternating(runs, args.rounds, lambda run: run(args.steps))

# --- the row kernel of every level alone: a pass whose paths_saliency_rows calls are bracketed by events on an idle device
per_level = []
for rep in range(5):
    with T.event_timed(("paths_saliency_rows",), dev) as seen:
        out, trace = input_gradients(model, sb, keep, L)
    assert len(seen) == L and int(out["status"].item()) == 0
    per_level.append([us for _, _, us in seen])
Ms = [int(t["grad_norm"].numel()) for t in trace]
rows_med = [statistics.median(r[l] for r in per_level) for l in range(L)]
rows = [{"level": l, "M": Ms[l], "MB": round((2 * Ms[l] * D * 4 + 8 * Ms[l]) / 1e6, 1), "us": round(rows_med[l], 1),
         "GB_per_s": round((2 * Ms[l] * D * 4 + 8 * Ms[l]) / (rows_med[l] * 1e-6) / 1e9, 1)} for l in range(L)]
del out, trace

# --- the dX product of every level's shape alone
from paths_amd import ops  # noqa: E402
lp = ops.pack_lstm(model.lstm)
G = lp["w_gates"].shape[0]
gemm = []
for l in range(L):
    M = Ms[l]
    dG, dy, dx = torch.randn((M, G), device=dev), torch.randn((M, D), device=dev), torch.empty((M, D), device=dev)
    ts = []
    for rep in range(7):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        bw.gemm_nt(dG, G, bw.Transposed(lp["w_gates"], G, D, ld=2 * D, offset=0), dx, D, M, D, G, residual=dy, ldr=D)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    gemm.append({"level": l, "M": M, "us": round(statistics.median(ts), 1),
                 "TFLOP_per_s": round(2.0 * M * D * G / (statistics.median(ts) * 1e-6) / 1e12, 1)})
    del dG, dy, dx

summ = T.summ
a, b = statistics.median(ms["input_gradients"]), statistics.median(ms["forward_backward"])
print(json.dumps({
    "workload": f"K = {K} x {L} levels, {SPG} slides per batch, fp32 grids, dropout off", "device": torch.cuda.get_device_name(dev),
    "input_gradients_ms": summ(ms["input_gradients"]), "forward_backward_ms": summ(ms["forward_backward"]),
    "input_gradients_over_forward_backward": round(a / b, 4), "rows_us_per_level": rows, "rows_us_total": round(sum(rows_med), 1),
    "dx_gemm_us_per_level": gemm, "dx_gemm_us_total": round(sum(g["us"] for g in gemm), 1),
    "steps_per_run": args.steps, "rounds": args.rounds}), flush=True)
