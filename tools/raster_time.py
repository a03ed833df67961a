#!/usr/bin/env python3
"""Cost of a heat map per slide: the NumPy painters of paths_amd.heatmap against heatmap.rasterize (csrc/raster.hip) for EIGHT
synthetic slides at K = 2048 x 5 levels, for kind "importance" (one folded raster per slide) and "rollout" (five planes per slide).
One JSON object per kind, written to --out (default profiles/raster_time.json) and printed:

    numpy_ms                 hierarchy_from_trace + importance_map / rollout_map for all eight slides (the host copies and the per-patch
                             painting loop; float64 rasters)
    rasterize_f32_ms / _f64_ms   heatmap.rasterize for the whole batch, check=True (its one host synchronise included)
    numpy_over_f32 / _f64    ratios of the medians
    index_us                 paths_raster_index alone, per level, event-timed on an otherwise idle device
    maps_f32 / maps_f64      paths_raster_maps alone, event-timed: microseconds, the bytes it stores (the padded allocation) and the
                             rate they give against the 6.3 TB/s HBM rate the project measures against

The whole-call figures come from one process, alternating rounds (A/B/C, then reversed) after warm-up, a host clock around calls
that end in a device synchronise.

    python tools/raster_time.py [--limit 420] [--rounds 6] [--out profiles/raster_time.json]

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
ap.add_argument("--rounds", type=int, default=6, help="alternating rounds (at least 5)")
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_time.json"))
args = ap.parse_args()
assert args.rounds >= 5, "the medians are taken over at least 5 rounds"

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--warmup", args.warmup, "--out", args.out])

import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import heatmap as hm  # noqa: E402
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch  # noqa: E402

K, B = 2048, 8
HBM_GBS = 6300.0
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, 0.0)
model.eval()
keep, L = cfg.top_k_patches, cfg.num_levels
ids = bench.CPU_SLIDE_IDS[K]
sb = DeviceSlideBatch([DeviceSlide.synthetic(bench.CPU_DSEED, ids[i % len(ids)], bench.BASE_SHAPES[K], device=dev) for i in range(B)])
grids = [s.shape(0) for s in sb.slides]
trace = []
with torch.no_grad():
    putils.recurse(model, sb, keep, L, trace=trace, rollout=True)
torch.cuda.synchronize()
visited = [int(sum(int(lv["num_ims"][b]) for lv in trace)) for b in range(B)]

results = []
for kind in ("importance", "rollout"):
    paint = hm.importance_map if kind == "importance" else hm.rollout_map

    def numpy_path():
        return [paint(hm.hierarchy_from_trace(trace, b), grids[b]) for b in range(B)]

    runs = {"numpy": numpy_path,
            "rasterize_f32": lambda: hm.rasterize(trace, grids, kind, dtype=torch.float32),
            "rasterize_f64": lambda: hm.rasterize(trace, grids, kind, dtype=torch.float64)}
    for name in runs:
        for _ in range(args.warmup):
            runs[name]()
    ms = T.alternating(runs, args.rounds)

    # --- the two kernels alone: calls whose launches are bracketed by events on an idle device
    kernels = {}
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        with T.event_timed(("paths_raster_index", "paths_raster_maps"), dev) as raw:
            for _ in range(args.rounds):
                maps = hm.rasterize(trace, grids, kind, dtype=dtype)
        base = maps[0]._base if maps[0]._base is not None else maps[0]
        nbytes = base.numel() * base.element_size()
        us = [u for n, a, u in raw if n == "paths_raster_maps"]
        med = statistics.median(us)
        kernels["maps_" + tag] = {"us": T.summ(us), "stored_MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / (med * 1e-6) / 1e9, 1),
                                  "of_hbm_rate": round(nbytes / (med * 1e-6) / 1e9 / HBM_GBS, 3)}
        if tag == "f32":                                  # (paths_raster_index: level at argument 4)
            kernels["index_us"] = [{"level": l, "rows": int(trace[l]["locs"].shape[1]),
                                    "us": T.summ([u for n, a, u in raw if n == "paths_raster_index" and a[4] == l])} for l in range(L)]
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"workload": f"{B} slides, K = {K} x {L} levels, kind = {kind}, level-0 grids {sorted(set(grids))}, "
                       f"raster {grids[0][0] << (L - 1)} x {grids[0][1] << (L - 1)} cells per slide" + (f" x {L} planes" if kind != "importance" else ""),
           "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "visited_patches_per_slide": visited,
           "numpy_ms": T.summ(ms["numpy"]), "rasterize_f32_ms": T.summ(ms["rasterize_f32"]), "rasterize_f64_ms": T.summ(ms["rasterize_f64"]),
           "numpy_over_f32": round(med["numpy"] / med["rasterize_f32"], 1), "numpy_over_f64": round(med["numpy"] / med["rasterize_f64"], 1),
           "hbm_rate_GB_per_s": HBM_GBS, **kernels}
    print(json.dumps(res), flush=True)
    results.append(res)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(results, fh, indent=1)
    fh.write("\n")
