#!/usr/bin/env python3
"""Dense against packed (tissue-only) slides on the headline workload: K = 2048 x 5 levels, 8 slides per batch, 3 distinct resident
batches rotated, one recorded launch tape per batch (bench.py's default infer mode), at the bench's background share and at
--p-bg (default 0.6).  The two forms hold the same values (the packed batches are slide.pack() of the dense ones), run in ONE
process, timed alternately in pairs after a warm-up, so drift of the box's clocks lands on both sides.  Per background share it
prints one line per pair and a JSON summary: slides/s per form (median / min / max), the per-pair ratio, the dense runs' own
run-to-run ratios (the noise the ratio is judged against), the pack time per slide and the exact resident bytes per slide.  One
more entry times paths_pack_rows alone on a level-4 grid (bytes read + written over device-event time).

    python tools/packed_slides_time.py [--pairs 7] [--steps 30] [--json out.json]

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats` with --pairs 1."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import _lib  # noqa: E402
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--steps", type=int, default=30, help="replays per timed run (rotating over the resident batches)")
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--rotate", type=int, default=3)
ap.add_argument("--p-bg", type=float, default=0.6, help="the second background share (the first is the bench's 0.1)")
ap.add_argument("--json", default=None)
args = ap.parse_args()
assert args.pairs >= 1

K, SPG, BENCH_P_BG = 2048, 8, 0.1
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, None)
summ = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def run(ts, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ts[i % len(ts)].replay()
    torch.cuda.synchronize()
    return SPG * steps / (time.perf_counter() - t0)


def measure(p_bg):
    dense = [[DeviceSlide.synthetic(1234, 100000 * r + i, bench.BASE_SHAPES[K], p_bg=p_bg, device=dev) for i in range(SPG)]
             for r in range(args.rotate)]
    torch.cuda.synchronize()
    packed, pack_s = [], []
    for b in dense:
        packed.append([])
        for s in b:
            t0 = time.perf_counter()
            packed[-1].append(s.pack())
            torch.cuda.synchronize()
            pack_s.append(time.perf_counter() - t0)
    nbytes = {"dense": [s.resident_bytes() for b in dense for s in b], "packed": [s.resident_bytes() for b in packed for s in b]}
    batches = {"dense": [DeviceSlideBatch(b) for b in dense], "packed": [DeviceSlideBatch(b) for b in packed]}
    tapes = {name: [putils.TapedRecursion(model, b, cfg.top_k_patches, cfg.num_levels).record() for b in bs] for name, bs in batches.items()}
    with torch.no_grad():           # the two forms compute the same thing: the tapes' outputs are bit-identical
        for a, b in zip(tapes["dense"], tapes["packed"]):
            oa, ob = a.replay(), b.replay()
            assert all(torch.equal(oa[k], ob[k]) for k in ("logits", "ctx_slide", "importance")), "packed / dense outputs differ"
            assert int(oa["status"].item()) == 0 and int(ob["status"].item()) == 0
    for name in tapes:
        run(tapes[name], args.warmup)
    rates, ratios = {"dense": [], "packed": []}, []
    for p in range(args.pairs):
        order = ("dense", "packed") if p % 2 == 0 else ("packed", "dense")
        got = {name: run(tapes[name], args.steps) for name in order}
        for name in got:
            rates[name].append(got[name])
        ratios.append(got["packed"] / got["dense"])
        print(f"p_bg {p_bg}: pair {p}: dense {got['dense']:.1f} slides/s, packed {got['packed']:.1f} slides/s, packed / dense {ratios[-1]:.4f}",
              flush=True)
    noise = [b / a for a, b in zip(rates["dense"], rates["dense"][1:])] or [1.0]
    res = {"p_bg": p_bg, "slides_per_s": {k: summ(v) for k, v in rates.items()}, "packed_over_dense": summ(ratios),
           "dense_run_to_run": summ(noise), "packed_median_inside_dense_spread": bool(min(noise) <= statistics.median(ratios) <= max(noise)),
           "pack_ms_per_slide": summ([1e3 * t for t in pack_s[1:]]),
           "resident_bytes_per_slide": {k: {"mean": round(statistics.mean(v)), "min": min(v), "max": max(v)} for k, v in nbytes.items()},
           "packed_over_dense_bytes": round(sum(nbytes["packed"]) / sum(nbytes["dense"]), 4)}
    for ts in tapes.values():
        for t in ts:
            t.close()
    return res


def pack_rows_rate(p_bg, reps=10):
    """paths_pack_rows alone on one level-4 grid (1024 x 2048 cells of 4 KiB): kept bytes read + written per device-event second."""
    s = DeviceSlide.synthetic(1234, 7, bench.BASE_SHAPES[K], p_bg=p_bg, device=dev)
    g, p = s.grids[4], s.pack()
    index, rows = p.index[4], torch.empty_like(p.rows[4])
    cells, n, D = g.shape[0] * g.shape[1], rows.shape[0], g.shape[2]
    call = lambda: _lib.call("paths_pack_rows", g.data_ptr(), cells, D, index.data_ptr(), n, rows.data_ptr(), _lib.stream())
    call()
    assert torch.equal(rows, p.rows[4])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    us = 1e3 * ev[0].elapsed_time(ev[1]) / reps
    moved = 2 * rows.numel() * rows.element_size() + 4 * cells
    return {"p_bg": p_bg, "cells": cells, "kept_rows": n, "us_per_launch": round(us, 1), "bytes_moved": moved,
            "TB_per_s": round(moved / us / 1e6, 3)}


out = {"workload": f"K = {K} x {cfg.num_levels} levels, {SPG} slides per batch, {args.rotate} resident batches rotated, taped",
       "pairs": args.pairs, "steps_per_run": args.steps, "device": torch.cuda.get_device_name(dev), "runs": [], "pack_rows": []}
for p_bg in (BENCH_P_BG, args.p_bg):
    out["runs"].append(measure(p_bg))
    out["pack_rows"].append(pack_rows_rate(p_bg))
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
