#!/usr/bin/env python3
"""On-demand slides (paths_amd.data_utils.slide.OnDemandSlide) at the headline shape: 8 slides at K = 2048 x 5 levels, served through
``OnDemandSlide.from_slide`` over resident slides (the encoder is a row lookup in the resident grids), against eager ``recurse()`` on
the same resident slides of the same build.  One JSON line:

    on_demand_slides_per_s   eager recurse() on the on-demand batch        } A/B/A/B rounds in one process after warm-up,
    resident_slides_per_s    eager recurse() on the resident slides        } host clock around work that ends in a device synchronise
    encode_ms_per_step       host time spent inside encode() (each call ends in a synchronise of its stream, so the stand-in's device
                             work is charged to it and not to the recursion), and the step time without it
    kernels_us_per_level     paths_candidate_children / paths_admit_children of every level, event-timed on an otherwise idle device
    requested_fraction       cells requested per pass / cells in the pyramids

    python tools/on_demand_time.py [--steps 20] [--rounds 5] [--warmup 5] [--limit 420]

The measurement runs in a fresh child process under ``timeout -k 10 <limit>``."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--limit", type=int, default=420, help="seconds for the child process")
ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
ap.add_argument("--steps", type=int, default=20, help="passes per timed run")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--k", type=int, default=2048, help="patches at level 0 (a bench.BASE_SHAPES key)")
args = ap.parse_args()

if not args.child:
    sys.exit(subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps),
                             "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--k", str(args.k)]).returncode)

import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import _lib  # noqa: E402
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch, OnDemandSlide, slide_batch  # noqa: E402

K, SPG = args.k, 8
assert torch.cuda.is_available(), "on_demand_time measures on the GPU"
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, None)
keep, L = cfg.top_k_patches, cfg.num_levels
res = [DeviceSlide.synthetic(1234, i, bench.BASE_SHAPES[K], device=dev) for i in range(SPG)]
od = [OnDemandSlide.from_slide(s) for s in res]
encode_s = [0.0]


def timed_encode(enc):
    def encode(level, cells):
        t0 = time.perf_counter()
        rows = enc(level, cells)
        torch.cuda.current_stream(dev).synchronize()
        encode_s[0] += time.perf_counter() - t0
        return rows
    return encode


for s in od:
    s.encode = timed_encode(s.encode)
rb, ob = DeviceSlideBatch(res), slide_batch(od)
pyramid = sum(s.shape(l)[0] * s.shape(l)[1] for s in res for l in range(L))

# --- the two new kernels of every level alone, bracketed by events on an idle device
real_call, kernel_us = _lib.call, {"paths_candidate_children": [], "paths_admit_children": []}


def timed_call(name, *a):
    if name not in kernel_us:
        return real_call(name, *a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.ExternalStream(a[-1], device=dev)
    e0.record(stream)
    real_call(name, *a)
    e1.record(stream)
    torch.cuda.synchronize()
    kernel_us[name].append(e0.elapsed_time(e1) * 1e3)


per_rep = []
with torch.no_grad():
    putils.recurse(model, ob, keep, L)                       # warm-up: packs, images
    out_r = putils.recurse(model, rb, keep, L)
    for rep in range(5):
        for v in kernel_us.values():
            v.clear()
        _lib.call = timed_call
        try:
            out_o = putils.recurse(model, ob, keep, L)
        finally:
            _lib.call = real_call
        assert all(len(v) == L - 1 for v in kernel_us.values()) and int(out_o["status"].item()) == 0
        per_rep.append({k: list(v) for k, v in kernel_us.items()})
    assert torch.equal(out_o["logits"], out_r["logits"]) and torch.equal(out_o["ctx_slide"], out_r["ctx_slide"]), "on-demand / resident outputs differ"
requested = [sum(int(s.requested[l].shape[0]) for s in od) for l in range(L)]
kernels = [{"level": l + 1, "cells_requested": requested[l + 1],
            **{k.replace("paths_", "") + "_us": round(statistics.median(r[k][l] for r in per_rep), 1) for k in kernel_us}} for l in range(L - 1)]


def run(name, steps):
    batch = ob if name == "on_demand" else rb
    encode_s[0] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for _ in range(steps):
            putils.recurse(model, batch, keep, L)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return SPG * steps / dt, dt / steps, encode_s[0] / steps


for name in ("on_demand", "resident"):
    run(name, args.warmup)
rates, step_ms, enc_ms = {"on_demand": [], "resident": []}, [], []
for r in range(args.rounds):
    for name in (("on_demand", "resident") if r % 2 == 0 else ("resident", "on_demand")):
        rate, step, enc = run(name, args.steps)
        rates[name].append(rate)
        if name == "on_demand":
            step_ms.append(step * 1e3)
            enc_ms.append(enc * 1e3)
summ = lambda v, nd=1: {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}
print(json.dumps({
    "workload": f"K = {K} x {L} levels, {SPG} slides per batch, fp32 rows, keep {list(keep)}", "device": torch.cuda.get_device_name(dev),
    "date": time.strftime("%Y-%m-%d"),
    "on_demand_slides_per_s": summ(rates["on_demand"]), "resident_slides_per_s": summ(rates["resident"]),
    "on_demand_over_resident": round(statistics.median(rates["on_demand"]) / statistics.median(rates["resident"]), 4),
    "step_ms": summ(step_ms, 3), "encode_ms_per_step": summ(enc_ms, 3),
    "step_without_encode_ms": summ([a - b for a, b in zip(step_ms, enc_ms)], 3),
    "kernels_us_per_level": kernels,
    "cells_requested_per_pass": sum(requested), "cells_in_the_pyramids": pyramid, "requested_fraction": round(sum(requested) / pyramid, 4),
    "steps_per_run": args.steps, "rounds": args.rounds}), flush=True)
