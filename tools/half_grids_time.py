#!/usr/bin/env python3
"""fp32 against fp16 feature grids on the headline workload: K = 2048 x 5 levels, 8 slides per batch, 3 distinct resident batches
rotated, one recorded launch tape per batch (bench.py's default infer mode).  The two dtypes hold the same values (the fp32 batches
are the fp16 grids widened), run in ONE process, timed alternately in pairs after a warm-up, so drift of the box's clocks lands on
both sides.  Prints one line per pair and a JSON summary (slides/s per dtype, median / min / max, the per-pair ratio spread).

    python tools/half_grids_time.py [--pairs 7] [--steps 30] [--json out.json]

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
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--steps", type=int, default=30, help="replays per timed run (rotating over the resident batches)")
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--rotate", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

K, SPG = 2048, 8
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, None)
half = [DeviceSlideBatch([DeviceSlide.synthetic(1234, 100000 * r + i, bench.BASE_SHAPES[K], device=dev, dtype=torch.float16)
                          for i in range(SPG)]) for r in range(args.rotate)]
full = [DeviceSlideBatch([DeviceSlide([g.float() for g in s.grids]) for s in b.slides]) for b in half]
torch.cuda.synchronize()
gib = lambda bs: sum(g.numel() * g.element_size() for b in bs for s in b.slides for g in s.grids) / 2**30
print(f"resident grids: fp32 {gib(full):.1f} GiB, fp16 {gib(half):.1f} GiB ({args.rotate} batches x {SPG} slides each)", flush=True)

tapes = {name: [putils.TapedRecursion(model, b, cfg.top_k_patches, cfg.num_levels).record() for b in bs]
         for name, bs in (("fp32", full), ("fp16", half))}
# the two dtypes compute the same thing: the tapes' outputs are bit-identical
with torch.no_grad():
    for a, b in zip(tapes["fp32"], tapes["fp16"]):
        oa, ob = a.replay(), b.replay()
        assert torch.equal(oa["logits"], ob["logits"]) and torch.equal(oa["ctx_slide"], ob["ctx_slide"]), "fp16 / fp32 outputs differ"
        assert int(oa["status"].item()) == 0 and int(ob["status"].item()) == 0


def run(name, steps):
    ts = tapes[name]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ts[i % len(ts)].replay()
    torch.cuda.synchronize()
    return SPG * steps / (time.perf_counter() - t0)


for name in ("fp32", "fp16"):
    run(name, args.warmup)
rates = {"fp32": [], "fp16": []}
ratios = []
for p in range(args.pairs):
    order = ("fp32", "fp16") if p % 2 == 0 else ("fp16", "fp32")
    got = {name: run(name, args.steps) for name in order}
    for name in got:
        rates[name].append(got[name])
    ratios.append(got["fp16"] / got["fp32"])
    print(f"pair {p}: fp32 {got['fp32']:.1f} slides/s, fp16 {got['fp16']:.1f} slides/s, fp16 / fp32 {ratios[-1]:.4f}", flush=True)

summ = lambda v: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
res = {"workload": f"K = {K} x {cfg.num_levels} levels, {SPG} slides per batch, {args.rotate} resident batches rotated, taped",
       "pairs": args.pairs, "steps_per_run": args.steps, "slides_per_s": {k: summ(v) for k, v in rates.items()},
       "fp16_over_fp32": summ(ratios), "device": torch.cuda.get_device_name(dev)}
print(json.dumps(res), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
for ts in tapes.values():
    for t in ts:
        t.close()
