#!/usr/bin/env python3
"""Cost of integrated gradients along the frozen path (paths_amd.saliency.integrated_gradients, csrc/path_rows.hip) for ONE slide at
K = 2048 x 5 levels, dropout off.  One JSON line:

    ig_chunk<c>_ms           integrated_gradients(steps = 32) with chunk = c for every c in --chunks (default 8, 1): the path pass,
                             ceil(32 / c) frozen passes of c virtual slides, the baseline forward
    input_gradients_x32_ms   32 calls of input_gradients on the same slide (what a Python loop around it would cost per map)
    points_us_per_level /    paths_path_points / paths_path_accumulate of every level alone at chunk = 8, event-timed on an otherwise
    accumulate_us_per_level  idle device, with their algorithmic bytes and the rate they give

All whole-call figures come from one process, alternating rounds (A/B/.., then reversed) after warm-up, a host clock around calls
that end in a device synchronise.

    python tools/path_attribution_time.py [--limit 420] [--rounds 4] [--chunks 8,1]

The measurement runs in a fresh child process under ``timeout -k 10 <limit>``."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attribution_timing as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--limit", type=int, default=420, help="seconds for the child process")
ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--chunks", default="8,1", help="chunk sizes to time, e.g. 1,2,4,8")
args = ap.parse_args()

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--warmup", args.warmup, "--chunks", args.chunks])

import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch  # noqa: E402
from paths_amd.saliency import input_gradients, integrated_gradients  # noqa: E402

K, STEPS = 2048, 32
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, 0.0)
keep, L = cfg.top_k_patches, cfg.num_levels
sb = DeviceSlideBatch([DeviceSlide.synthetic(bench.CPU_DSEED, bench.CPU_SLIDE_IDS[K][0], bench.BASE_SHAPES[K], device=dev)])
D = sb.dim
chunks = [int(c) for c in args.chunks.split(",")]


def loop32():
    for _ in range(STEPS):
        input_gradients(model, sb, keep, L)


runs = {f"ig_chunk{c}": (lambda c=c: integrated_gradients(model, sb, keep, L, steps=STEPS, chunk=c)) for c in chunks}
runs["input_gradients_x32"] = loop32
for name in runs:
    for _ in range(args.warmup):
        runs[name]()
ms = T.alternating(runs, args.rounds)

# --- the two row kernels of every level alone: a call whose launches of them are bracketed by events on an idle device
with T.event_timed(("paths_path_points", "paths_path_accumulate"), dev) as raw:
    out, trace = integrated_gradients(model, sb, keep, L, steps=STEPS, chunk=8)
seen = [(name, a[7], a[10], us) for name, a, us in raw]     # (both entry points: ..., rows_per_slide, D, B, C at positions 7..10)
Ns = [int(t["grad_norm"].shape[1]) for t in trace]
valid = [int(t["num_ims"].sum()) for t in trace]


def per_level(name, nbytes):
    rows = []
    for l in range(L):
        us = [u for n, N, C, u in seen if n == name and N == Ns[l] and C == 8]
        # (levels can share a padded length: their launches are pooled)
        med = statistics.median(us)
        rows.append({"level": l, "rows": Ns[l], "valid": valid[l], "launches": len(us), "MB": round(nbytes(valid[l]) / 1e6, 1),
                     "us": round(med, 1), "GB_per_s": round(nbytes(valid[l]) / (med * 1e-6) / 1e9, 1)})
    return rows


points = per_level("paths_path_points", lambda m: (1 + 8) * m * D * 4)
accum = per_level("paths_path_accumulate", lambda m: (8 + 1) * m * D * 4 + 16 * m)
summ = T.summ
res = {"workload": f"one slide, K = {K} x {L} levels, fp32 grids, dropout off, steps = {STEPS}, gausslegendre",
       "device": torch.cuda.get_device_name(dev), "rounds": args.rounds}
for name in runs:
    res[name + "_ms"] = summ(ms[name])
base = statistics.median(ms["input_gradients_x32"])
for c in chunks:
    res[f"input_gradients_x32_over_ig_chunk{c}"] = round(base / statistics.median(ms[f"ig_chunk{c}"]), 2)
res["completeness_gap_over_target_change"] = float((out["completeness_gap"] / (out["target"] - out["target_baseline"])).abs().max())
res["points_us_per_level"], res["accumulate_us_per_level"] = points, accum
print(json.dumps(res), flush=True)
