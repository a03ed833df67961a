#!/usr/bin/env python3
"""Cost of the resize in front of the encoder (paths_amd.pixels.encoder_input(resize=...); csrc/tile_resize.hip): 8,192 tiles
of 256 x 256 pixels, about two thirds of them with tissue, into ``[m, 3, 224, 224]`` fp16 encoder input in chunks of --batch tiles,
ImageNet normalisation:

    ours       pixels.encoder_input(..., resize=224): bytes in, Pillow's bicubic resize in integers, the table, fp16 out - one launch
               per chunk, the 256 x 256 float tensor never exists
    chain      what a caller writes today: pixels.encoder_input at 256, then torch.nn.functional.interpolate(x, size=224,
               mode="bicubic", antialias=True) on the same chunks (a float resize of normalised values: NOT the same result - the
               largest difference is reported, not bounded)

One JSON object, written to --out (default profiles/tile_resize_time.json) and printed: the median / min / max milliseconds of one
whole phase (all chunks) for both sides over --rounds alternating rounds in one process (A/B, then B/A; a host clock around --reps
phases that end in a device synchronise), ``chain_over_ours``, and for ``ours`` the whole-phase rate over the algorithmic bytes
(3 P^2 in and 3 C^2 x 2 out per tile) beside the 6.3 TB/s HBM rate the project measures against.  A whole-phase rate includes the
launches and the allocation of every chunk's output: it is not the kernel's share of peak.

    python tools/tile_resize_time.py [--limit 420] [--rounds 6] [--reps 5] [--tiles 8192] [--batch 256] [--out profiles/tile_resize_time.json]

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
ap.add_argument("--rounds", type=int, default=6, help="alternating rounds (at least 6)")
ap.add_argument("--reps", type=int, default=5, help="whole phases per timed window")
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--tiles", type=int, default=8192)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_resize_time.json"))
args = ap.parse_args()
assert args.rounds >= 6, "the medians are taken over at least 6 rounds"

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--reps", args.reps, "--warmup", args.warmup, "--tiles", args.tiles,
                                          "--batch", args.batch, "--out", args.out])

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from paths_amd import pixels  # noqa: E402

P, S, STRIDE, THR = 256, 224, 4, 0.1
HBM_GBS = 6300.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
dev = torch.device("cuda:0")
n = args.tiles
gen = torch.Generator(device=dev).manual_seed(0)
tiles = torch.randint(0, 200, (n, P, P, 3), dtype=torch.uint8, device=dev, generator=gen)
tiles[::3] = 255                                                      # a third of the tiles are blank
t = pixels.otsu_threshold([tiles[k] for k in range(0, n, max(1, n // 16))])
table = pixels.normalize_table(MEAN, STD, torch.float16).to(dev)
ts = pixels.tile_tissue(tiles, t, THR, STRIDE)
m = ts.m
chunks = [(first, min(args.batch, m - first)) for first in range(0, m, args.batch)]


def ours_chunk(first, count):
    return pixels.encoder_input(ts.tiles, ts.order, first, count, table, resize=S)


def chain_chunk(first, count):
    return F.interpolate(pixels.encoder_input(ts.tiles, ts.order, first, count, table), size=S, mode="bicubic", antialias=True)


def phase(chunk):
    def run():
        for _ in range(args.reps):
            for first, count in chunks:
                chunk(first, count)
    return run


first, count = chunks[len(chunks) // 2]
a, b = ours_chunk(first, count), chain_chunk(first, count)
assert a.shape == b.shape == (count, 3, S, S) and a.dtype == b.dtype == torch.float16
diff = (a.float() - b.float()).abs()
del a, b

runs = {"ours": phase(ours_chunk), "chain": phase(chain_chunk)}
for fn in runs.values():
    for _ in range(args.warmup):
        fn()
ms = {k: [x / args.reps for x in v] for k, v in T.alternating(runs, args.rounds).items()}
moved = m * (3 * P * P + 3 * S * S * 2)
rate = moved / (statistics.median(ms["ours"]) * 1e-3) / 1e9
res = {"workload": f"{n} tiles of {P} x {P} pixels ({n * P * P * 3 / 1e9:.2f} GB), {m} with tissue, resized to {S} x {S} (bicubic, antialiased), "
                   f"fp16 encoder input in chunks of {args.batch} tiles ({m * 3 * S * S * 2 / 1e9:.2f} GB)",
       "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "phases_per_window": args.reps, "tissue_tiles": m,
       "chain": "pixels.encoder_input at 256, then torch.nn.functional.interpolate(size=224, mode='bicubic', antialias=True)",
       "chain_differs_from_ours_by": {"max_abs": round(float(diff.max()), 4), "mean_abs": round(float(diff.mean()), 6),
                                      "note": "a float resize of normalised values against Pillow's integer resize of the bytes"},
       "ours_ms": T.summ(ms["ours"]), "chain_ms": T.summ(ms["chain"]),
       "chain_over_ours": round(statistics.median(ms["chain"]) / statistics.median(ms["ours"]), 2),
       "algorithmic_bytes_GB": round(moved / 1e9, 2), "whole_phase_GB_per_s": round(rate, 1), "hbm_rate_GB_per_s": HBM_GBS,
       "of_hbm_rate": round(rate / HBM_GBS, 3)}
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
