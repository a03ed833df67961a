#!/usr/bin/env python3
"""Cost of an overlay per batch: heatmap.render (csrc/raster.hip: paths_render_range / paths_render_rgb) for EIGHT synthetic slides at
K = 2048 x 5 levels, the folded importance map, at cell_px 4 and 16, with and without thumbnails, against what a user does without
it: ``rasterize`` -> ``.cpu()`` -> NumPy repeat / normalise / table / blend (no outlines, nothing fancier).  One JSON object per
(cell_px, thumbnails), written to --out (default profiles/render_time.json) and printed:

    render_ms            heatmap.render for the whole batch, check=True (its one host synchronise included)
    rgb_window_us        device time per call of ten render(vmin, vmax given, check=False) calls queued behind one another, between two
                         events: paths_render_rgb plus rasterize's six launches (0.02 - 0.03 ms, profiles/raster_time.json).  One pair of
                         events around a single launch is not used: on this runtime it reads anything from 6 us to the true time
    with_range_window_us / range_us_by_difference
                         the same with the automatic range, i.e. plus paths_render_range, and the difference of the medians
    rgb_stored_MB, rgb_GB_per_s, rgb_of_hbm_rate
                         the bytes paths_render_rgb stores (the padded allocation) over rgb_window_us - a lower bound of the kernel's own
                         rate - against the 6.3 TB/s HBM rate the project measures against
    numpy_one_slide_ms   the NumPy path for ONE slide (slide 0; its thumbnail already on the host), median of --numpy-rounds runs;
    numpy_batch_ms       eight times that: the slides are alike, and at cell_px 16 one slide alone is 402 MB of pixels
    numpy_over_render    numpy_batch_ms / render_ms

The render figures come from one process, alternating rounds (A/B, then reversed) after warm-up, a host clock around calls that end
in a device synchronise.

    python tools/render_time.py [--limit 420] [--rounds 6] [--numpy-rounds 3] [--out profiles/render_time.json]

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
ap.add_argument("--numpy-rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.json"))
args = ap.parse_args()
assert args.rounds >= 5, "the medians are taken over at least 5 rounds"

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--numpy-rounds", args.numpy_rounds, "--warmup", args.warmup, "--out", args.out])

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import colormaps  # noqa: E402
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
    putils.recurse(model, sb, keep, L, trace=trace)
torch.cuda.synchronize()
f = 1 << (L - 1)
table = colormaps.viridis()


def numpy_path(c, thumb):
    """What a user does without render, for slide 0: the folded raster to the host, nearest-neighbour upsampling, the reference's
    normalisation, the table, a blend where the map is positive."""
    m = hm.rasterize(trace, grids, "importance")[0].cpu().numpy().astype(np.float64)
    seen = m > 0
    lo, hi = m[seen].min(), m.max()
    k = np.clip(((np.where(seen, m, lo) - lo) / (hi - lo) * 256.0).astype(np.int64), 0, 255)
    up = lambda a: np.repeat(np.repeat(a, c, axis=0), c, axis=1)
    colour, mask = up(table[k]).astype(np.uint16), up(seen)[..., None]
    under = thumb.astype(np.uint16) if thumb is not None else np.uint16(255)
    return np.where(mask, (128 * colour + 127 * under + 127) // 255, under).astype(np.uint8)


def back_to_back(fn, n=10):
    """Milliseconds per call of n calls queued behind one another, between two events on an idle device: the launches of one call run
    while the host prepares the next, so this is device time per call once a call's kernels outlast its host work."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


results = []
for c in (4, 16):
    shape = lambda g: (g[0] * f * c, g[1] * f * c, 3)
    thumbs = [torch.randint(0, 256, shape(g), dtype=torch.uint8, device=dev) for g in grids]
    host_thumb = thumbs[0].cpu().numpy()
    runs = {"plain": lambda: hm.render(trace, grids, cell_px=c), "thumbnails": lambda: hm.render(trace, grids, cell_px=c, thumbnails=thumbs)}
    for name in runs:
        for _ in range(args.warmup):
            runs[name]()
    ms = T.alternating(runs, args.rounds)
    for name in runs:
        kw = {"thumbnails": thumbs} if name == "thumbnails" else {}
        fixed = lambda: hm.render(trace, grids, cell_px=c, vmin=0.0, vmax=1.0, check=False, **kw)      # rasterize's launches + paths_render_rgb
        auto = lambda: hm.render(trace, grids, cell_px=c, check=False, **kw)                          # ... + paths_render_range
        base = fixed()[0]
        while base._base is not None:
            base = base._base
        nbytes = base.numel()
        del base
        window = {"fixed": [], "auto": []}
        for r in range(args.rounds):
            for tag, fn in ((("fixed", fixed), ("auto", auto)) if r % 2 == 0 else (("auto", auto), ("fixed", fixed))):
                window[tag].append(back_to_back(fn) * 1e3)
        rgb = window["fixed"]
        rate = nbytes / (statistics.median(rgb) * 1e-6) / 1e9
        thumb = host_thumb if name == "thumbnails" else None
        numpy_path(c, thumb)
        one = [T.timed(lambda: numpy_path(c, thumb)) for _ in range(args.numpy_rounds)]
        med = statistics.median(ms[name])
        res = {"workload": f"{B} slides, K = {K} x {L} levels, folded importance, level-0 grids {sorted(set(grids))}, cell_px = {c}: "
                           f"{grids[0][0] * f * c} x {grids[0][1] * f * c} pixels per slide" + (", over thumbnails" if thumb is not None else ""),
               "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "cell_px": c, "thumbnails": thumb is not None,
               "render_ms": T.summ(ms[name]), "rgb_window_us": T.summ(rgb), "with_range_window_us": T.summ(window["auto"]),
               "range_us_by_difference": round(statistics.median(window["auto"]) - statistics.median(rgb), 1),
               "rgb_stored_MB": round(nbytes / 1e6, 1), "rgb_GB_per_s": round(rate, 1), "rgb_of_hbm_rate": round(rate / HBM_GBS, 3),
               "hbm_rate_GB_per_s": HBM_GBS, "numpy_rounds": args.numpy_rounds, "numpy_one_slide_ms": T.summ(one),
               "numpy_batch_ms": round(B * statistics.median(one), 1), "numpy_over_render": round(B * statistics.median(one) / med, 1)}
        print(json.dumps(res), flush=True)
        results.append(res)
    del thumbs

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(results, fh, indent=1)
    fh.write("\n")
