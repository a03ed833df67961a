#!/usr/bin/env python3
"""Cost of the removal curves on the free path (paths_amd.saliency.removal_curves, csrc/perturb_rows.hip) for ONE slide and for EIGHT
slides at K = 2048 x 5 levels, dropout off, steps = 8, order = "both", scores = "importance".  One JSON line per batch size:

    curves_ms                removal_curves: the path pass, two joint rankings, the members' masks, 1 + 2 ceil(8 / chunk) free passes
                             of masked views with their overlap counts
    recurse_ms               one no-grad recurse() of the same batch (the unit the expectation "about 2 steps forwards plus the path
                             pass" is stated in)
    curves_over_recurse      the ratio of the two medians
    masks_us_per_level       paths_removal_masks of every level alone (the members' launches, C = steps), event-timed on an otherwise
                             idle device, with its algorithmic bytes ((1 + C) cells per slide) and the rate they give
    overlap_us_per_level     paths_visited_overlap of every level alone at the default chunk, event-timed

The whole-call figures come from one process, alternating rounds (A/B/A/B, then reversed) after warm-up, a host clock around calls
that end in a device synchronise.

    python tools/removal_time.py [--limit 420] [--rounds 4] [--batches 1,8]

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
ap.add_argument("--batches", default="1,8", help="batch sizes to time")
args = ap.parse_args()

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--warmup", args.warmup, "--batches", args.batches])

import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch  # noqa: E402
from paths_amd.saliency import removal_curves  # noqa: E402

K, STEPS = 2048, 8
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, 0.0)
model.eval()
keep, L = cfg.top_k_patches, cfg.num_levels
ids = bench.CPU_SLIDE_IDS[K]

for B in [int(b) for b in args.batches.split(",")]:
    sb = DeviceSlideBatch([DeviceSlide.synthetic(bench.CPU_DSEED, ids[i % len(ids)], bench.BASE_SHAPES[K], device=dev) for i in range(B)])

    def forward():
        with torch.no_grad():
            putils.recurse(model, sb, keep, L)

    runs = {"curves": lambda: removal_curves(model, sb, keep, L, "importance", steps=STEPS, order="both"), "recurse": forward}
    for name in runs:
        for _ in range(args.warmup):
            runs[name]()
    ms = T.alternating(runs, args.rounds)

    # --- the two kernels alone: a call whose launches of them are bracketed by events on an idle device
    with T.event_timed(("paths_removal_masks", "paths_visited_overlap"), dev) as raw:
        out, trace = removal_curves(model, sb, keep, L, "importance", steps=STEPS, order="both")
    chunk = max(1, 8 // B)
    cells = [max(s.shape(l)[0] * s.shape(l)[1] for s in sb.slides) for l in range(L)]
    masks, overlap = [], []
    for l in range(L):                                  # removal_masks: max_cells at 3, C at 12;  visited_overlap: C at 9
        us = [u for n, a, u in raw if n == "paths_removal_masks" and a[3] == cells[l] and a[12] == STEPS]
        if us:
            med, nbytes = statistics.median(us), (1 + STEPS) * cells[l] * B
            masks.append({"level": l, "cells": cells[l], "members": STEPS, "launches": len(us), "KB": round(nbytes / 1e3, 1),
                          "us": round(med, 1), "GB_per_s": round(nbytes / (med * 1e-6) / 1e9, 2)})
    seen = [(a[7], a[9], u) for n, a, u in raw if n == "paths_visited_overlap"]          # (rows per member, members, us)
    for Nm in sorted({s[0] for s in seen}):
        us = [u for n, c, u in seen if n == Nm and c == chunk]
        if us:
            overlap.append({"rows": Nm, "members": chunk, "launches": len(us), "us": round(statistics.median(us), 1)})
    res = {"workload": f"{B} slide(s), K = {K} x {L} levels, fp32 grids, dropout off, steps = {STEPS}, order = both, chunk = {chunk}",
           "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "curves_ms": T.summ(ms["curves"]), "recurse_ms": T.summ(ms["recurse"]),
           "curves_over_recurse": round(statistics.median(ms["curves"]) / statistics.median(ms["recurse"]), 2),
           "free_passes": 1 + 2 * -(-STEPS // chunk),
           "masks_us_per_level": masks, "overlap_us_per_level": overlap,
           "morf_auc": [round(float(v), 5) for v in out["morf_auc"]], "lerf_auc": [round(float(v), 5) for v in out["lerf_auc"]],
           "visited_last_point": {k: v[:, -1].sum(dim=0).tolist() for k, v in out["visited"].items()},
           "path_overlap_last_point": {k: v[:, -1].sum(dim=0).tolist() for k, v in out["path_overlap"].items()}}
    print(json.dumps(res), flush=True)
    del sb, out, trace
