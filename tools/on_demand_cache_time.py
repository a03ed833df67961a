#!/usr/bin/env python3
"""The row cache of on-demand slides (paths_amd.data_utils.slide.CachedOnDemandSlide) at the headline shape: 8 slides at K = 2048 x 5
levels, four ways in one process, alternating:

    plain        OnDemandSlide.from_slide over the resident slides: every pass pays the encoder in full (the path without a cache)
    cache_cold   CachedOnDemandSlide.from_slide, cleared before every pass: all misses - the encoder in full plus probe, fill and the
                 stores' growth
    cache_warm   the same slides, cache filled: all hits - the encoder is not called
    resident     eager recurse() on the resident slides themselves

The stand-in encoder is a row lookup in the resident grids; its time is reported apart (each call ends in a synchronise of its stream,
as in tools/on_demand_time.py), so ``step_without_encode_ms`` is what the recursion and the cache cost around ANY encoder.
``kernels_per_level``: paths_cache_probe / paths_cache_fill of every level of a cold and of a warm pass, event-timed on an otherwise
idle device, with the bytes they move (probe: cells, index entries, src, miss cells; fill: source rows + buffer rows + stored rows).

    python tools/on_demand_cache_time.py [--steps 10] [--rounds 5] [--warmup 3] [--limit 420] [--out profiles/on_demand_cache_time.json]

The measurement runs in a fresh child process under ``timeout -k 10 <limit>``; the result is one JSON document, printed and written
to ``--out``."""
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
ap.add_argument("--steps", type=int, default=10, help="passes per timed run")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--k", type=int, default=2048, help="patches at level 0 (a bench.BASE_SHAPES key)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "on_demand_cache_time.json"))
args = ap.parse_args()

if not args.child:
    sys.exit(subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps),
                             "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--k", str(args.k), "--out", args.out]).returncode)

import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import _lib  # noqa: E402
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import CachedOnDemandSlide, DeviceSlide, DeviceSlideBatch, OnDemandSlide, slide_batch  # noqa: E402

K, SPG = args.k, 8
assert torch.cuda.is_available(), "on_demand_cache_time measures on the GPU"
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, None)
keep, L = cfg.top_k_patches, cfg.num_levels
res = [DeviceSlide.synthetic(1234, i, bench.BASE_SHAPES[K], device=dev) for i in range(SPG)]
plain = [OnDemandSlide.from_slide(s) for s in res]
cached = [CachedOnDemandSlide.from_slide(s) for s in res]
encode_s = [0.0]


def timed_encode(enc):
    def encode(level, cells):
        t0 = time.perf_counter()
        rows = enc(level, cells)
        torch.cuda.current_stream(dev).synchronize()
        encode_s[0] += time.perf_counter() - t0
        return rows
    return encode


for s in plain + cached:
    s.encode = timed_encode(s.encode)
batches = {"plain": slide_batch(plain), "cache_cold": slide_batch(cached), "cache_warm": slide_batch(cached), "resident": DeviceSlideBatch(res)}
D, row_bytes = res[0].dim, res[0].dim * 4

# --- the two kernels of every level alone, bracketed by events on an idle device
real_call, timed = _lib.call, {"paths_cache_probe": [], "paths_cache_fill": []}


def timed_call(name, *a):
    if name not in timed:
        return real_call(name, *a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.ExternalStream(a[-1], device=dev)
    e0.record(stream)
    real_call(name, *a)
    e1.record(stream)
    torch.cuda.synchronize()
    timed[name].append(e0.elapsed_time(e1) * 1e3)


def clear():
    for s in cached:
        s.clear()


def kernel_pass(cold: bool):
    """One pass with the two kernels timed: per level (probe us, fill us, cells requested, cells missed, buffer rows)."""
    if cold:
        clear()
    for v in timed.values():
        v.clear()
    _lib.call = timed_call
    try:
        with torch.no_grad():
            out = putils.recurse(model, batches["cache_cold"], keep, L)
    finally:
        _lib.call = real_call
    assert all(len(v) == L for v in timed.values()) and int(out["status"].item()) == 0
    asked = [sum(int(s.requested[l].shape[0]) for s in cached) for l in range(L)]
    missed = [sum(int(s.encoded[l].shape[0]) for s in cached) for l in range(L)]
    return list(timed["paths_cache_probe"]), list(timed["paths_cache_fill"]), asked, missed, out


sizes = putils._level_sizes(batches["resident"].n0, keep, L)
caps = [sizes[0]] + [4 * putils._child_capacity(sizes[l], int(keep[l]))[0] for l in range(L - 1)]      # rows per slide of each level's buffer
with torch.no_grad():
    for b in batches.values():                                 # warm-up: packs, images; the cache is filled
        putils.recurse(model, b, keep, L)
    out_r = putils.recurse(model, batches["resident"], keep, L)
reps = {True: [kernel_pass(True) for _ in range(5)], False: [kernel_pass(False) for _ in range(5)]}
for r in reps[True] + reps[False]:
    assert torch.equal(r[4]["logits"], out_r["logits"]) and torch.equal(r[4]["ctx_slide"], out_r["ctx_slide"]), "cached / resident outputs differ"
kernels = []
for cold in (True, False):
    _, _, asked, missed, _ = reps[cold][-1]
    assert missed == (asked if cold else [0] * L)
    for l in range(L):
        probe_us = statistics.median(r[0][l] for r in reps[cold])
        fill_us = statistics.median(r[1][l] for r in reps[cold])
        probe_bytes = asked[l] * (16 + 4 + 4) + missed[l] * 16
        # fill: every requested row is read once (store or encoder rows) and every buffer row written (the tail as zeros); a stored miss is written twice
        fill_bytes = asked[l] * row_bytes + SPG * caps[l] * row_bytes + missed[l] * row_bytes + asked[l] * 4
        kernels.append({"pass": "cold" if cold else "warm", "level": l, "cells_requested": asked[l], "cells_missed": missed[l],
                        "buffer_rows": SPG * caps[l], "probe_us": round(probe_us, 1), "probe_bytes": probe_bytes,
                        "fill_us": round(fill_us, 1), "fill_bytes": fill_bytes, "fill_gb_per_s": round(fill_bytes / fill_us / 1e3, 1)})


def run(name, steps):
    batch = batches[name]
    enc, dt = 0.0, 0.0
    for _ in range(steps):
        if name == "cache_cold":
            clear()
        encode_s[0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            putils.recurse(model, batch, keep, L)
        torch.cuda.synchronize()
        dt += time.perf_counter() - t0
        enc += encode_s[0]
    if name == "cache_warm":
        assert enc == 0.0, "a warm pass calls no encoder"
    return dt / steps * 1e3, enc / steps * 1e3


order = ["plain", "cache_cold", "cache_warm", "resident"]
for name in order:
    run(name, args.warmup)
step_ms, enc_ms = {n: [] for n in order}, {n: [] for n in order}
for r in range(args.rounds):
    for name in (order if r % 2 == 0 else order[::-1]):        # (cache_warm follows a cold pass either way: the cache is full again)
        if name == "cache_warm":
            run("cache_warm", 1)
        step, enc = run(name, args.steps)
        step_ms[name].append(step)
        enc_ms[name].append(enc)
summ = lambda v, nd=3: {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}
pyramid = sum(s.shape(l)[0] * s.shape(l)[1] for s in res for l in range(L))
doc = {
    "workload": f"K = {K} x {L} levels, {SPG} slides per batch, fp32 rows, keep {list(keep)}", "device": torch.cuda.get_device_name(dev),
    "date": time.strftime("%Y-%m-%d"), "tool": "tools/on_demand_cache_time.py",
    "step_ms": {n: summ(step_ms[n]) for n in order},
    "encode_ms_per_step": {n: summ(enc_ms[n]) for n in order if n != "resident"},
    "step_without_encode_ms": {n: summ([a - b for a, b in zip(step_ms[n], enc_ms[n])]) for n in order},
    "kernels_per_level": kernels,
    "cells_requested_per_pass": sum(reps[True][-1][2]), "cells_in_the_pyramids": pyramid,
    "stored_rows": sum(sum(s.count) for s in cached), "store_bytes": sum(s.capacity(l) for s in cached for l in range(L)) * row_bytes,
    "index_bytes": sum(s.index[l].numel() * 4 for s in cached for l in range(L) if s.index[l] is not None),
    "steps_per_run": args.steps, "rounds": args.rounds}
text = json.dumps(doc, indent=1)
print(text, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
