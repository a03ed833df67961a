#!/usr/bin/env python3
"""Cost of annotation coverage per batch: annotations.coverage (csrc/polygons.hip: paths_polygon_cover) for EIGHT slides of the
K = 2048 x 5 levels workload - a 512 x 1024 finest raster each -, s = 4 samples per axis, five polygons of about 1,000 jittered vertices
per slide, against what a caller can do without it: Pillow's ``ImageDraw.polygon`` fill of an 8-bit image at sample resolution on the
host, block sums, and the upload.  Pillow fills by another rule (pixel centres, its own edge handling), so it is a yardstick for TIME
only, never for bits.  One JSON object, written to --out (default profiles/annotation_time.json) and printed:

    coverage_ms            annotations.coverage for the whole batch, its table already on the device, to a device synchronise
    pillow_ms              the host route for the whole batch (fill, block sums, one upload per slide)
    pillow_over_coverage   ratio of the medians
    coverage_window_us     device time per call of ten coverage calls queued behind one another, between two events
    stream_only_window_us  the same for the same polygons moved to the near side of every grid, where the tile test drops every edge:
                           what streaming the edges through LDS and writing the raster cost by themselves
    naive_tests            samples x edges, summed over the slides
    tile_tests             (tile, edge) tests of the loader: one per edge and 16 x 16-cell workgroup
    cell_tests             (cell, kept edge) classifications
    row_only               of those, edges wholly beyond the cell's samples: a row test per sample row, no product
    sample_tests           (sample, edge) evaluations of t that remain
    naive_over_sample_tests
    bound                  which part bounds the kernel, from the two windows
    draw_ms / draw_window_us   annotations.draw of the same polygons on images of cell_px 4 and 16, width 1

Both sides are measured in one process, alternating rounds (A/B, then reversed) after warm-up, a host clock around calls that end in a
device synchronise.

    python tools/annotation_time.py [--limit 420] [--rounds 6] [--out profiles/annotation_time.json]

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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotation_time.json"))
args = ap.parse_args()
assert args.rounds >= 5, "the medians are taken over at least 5 rounds"

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--warmup", args.warmup, "--out", args.out])

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image, ImageDraw  # noqa: E402

import bench  # noqa: E402
from paths_amd import annotations as A  # noqa: E402

K, B, L, S, PATCH = 2048, 8, 5, 4, 256
TILE = 16
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
grids = [bench.BASE_SHAPES[K]] * B
f = 1 << (L - 1)
X, Y = grids[0][0] * f, grids[0][1] * f
cell = PATCH / f                                           # level-0 pixels per finest cell


def blobs(seed):
    """Five closed curves of about 1,000 jittered vertices each, in level-0 pixels, one of them partly outside the slide."""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate((1400, 1100, 1000, 900, 600)):
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        radius = rng.uniform(40, 140) * cell * (1 + 0.25 * np.sin(3 * a + k)) + rng.uniform(-0.4, 0.4, n) * cell
        centre = (rng.uniform(0.15, 0.85) * X * cell, rng.uniform(0.15, 0.85) * Y * cell) if k else (0.95 * X * cell, 0.5 * Y * cell)
        out.append(np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1))
    return out


per_slide = [blobs(b) for b in range(B)]
polygons = A.Polygons(per_slide, grids, L)
near_side = A.Polygons([[p - np.array([0.0, 2.0 * Y * cell]) for p in polys] for polys in per_slide], grids, L)


def pillow_route():
    out = []
    for polys in per_slide:
        image = Image.new("L", (Y * S, X * S), 0)              # (width, height): columns are the grid's Y
        pen = ImageDraw.Draw(image)
        for p in polys:
            pen.polygon([(float(c) / cell * S, float(r) / cell * S) for r, c in p], fill=1)
        counts = np.asarray(image, dtype=np.uint8).reshape(X, S, Y, S).sum(axis=(1, 3), dtype=np.int32)
        out.append(torch.from_numpy(counts).to(dev))
    return out


def back_to_back(fn, n=10):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def culling_counts(p):
    """The tests paths_polygon_cover executes for ``p``, by the kernel's own rules (csrc/polygons.hip), against samples x edges."""
    step, first = 65536 // S, 65536 // S // 2
    naive = tile_tests = cell_tests = row_only = sample_tests = 0
    cx = np.arange(TILE, dtype=np.int64)
    for b in range(p.B):
        ex, ey = p.finest(b)
        v0, v1 = int(p.poly_off[p.slide_poly[b]]), int(p.poly_off[p.slide_poly[b + 1]])
        a = p.verts[v0:v1].astype(np.int64)
        c = p.verts[p.next_vertex[v0:v1]].astype(np.int64)
        rmin, rmax, cmin, cmax = np.minimum(a[:, 0], c[:, 0]), np.maximum(a[:, 0], c[:, 0]), np.minimum(a[:, 1], c[:, 1]), np.maximum(a[:, 1], c[:, 1])
        naive += ex * ey * S * S * len(a)
        for tx in range(0, ex, TILE):
            tr_lo, tr_hi = (tx << 16) + first, ((min(tx + TILE, ex) - 1) << 16) + first + (S - 1) * step
            rows_meet = (rmin != rmax) & (rmin <= tr_hi) & (rmax > tr_lo)
            for ty in range(0, ey, TILE):
                tile_tests += len(a)
                kept = np.nonzero(rows_meet & (cmax > (ty << 16) + first))[0]
                if kept.size == 0:
                    continue
                nx, ny = min(TILE, ex - tx), min(TILE, ey - ty)
                cell_tests += nx * ny * kept.size
                pr0 = ((tx + cx[:nx]) << 16)[:, None] + first                               # [nx, 1] against [1, kept]
                pc0 = ((ty + cx[:ny]) << 16)[:, None] + first
                below = lambda m: np.clip(-((pr0 - m[None, :]) // step), 0, S)              # sample rows of the cell below m
                rows = below(rmax[kept]) - below(rmin[kept])                                # [nx, kept]: sample rows the edge crosses
                beyond = cmin[kept][None, :] > pc0 + (S - 1) * step                         # [ny, kept]
                near = cmax[kept][None, :] <= pc0
                crossed = (rows > 0).astype(np.int64)
                row_only += int(crossed.sum(axis=0) @ beyond.sum(axis=0))
                sample_tests += int(rows.sum(axis=0) @ (~beyond & ~near).sum(axis=0)) * S
    return {"naive_tests": int(naive), "tile_tests": int(tile_tests), "cell_tests": int(cell_tests), "row_only": row_only, "sample_tests": sample_tests,
            "naive_over_sample_tests": round(naive / max(sample_tests, 1), 1)}


runs = {"coverage": lambda: A.coverage(polygons, S), "pillow": pillow_route}
for name in runs:
    for _ in range(args.warmup):
        runs[name]()
ms = T.alternating(runs, args.rounds)
A.coverage(near_side, S)
window = {"coverage": [], "stream_only": []}
for r in range(args.rounds):
    order = (("coverage", polygons), ("stream_only", near_side))
    for tag, p in (order if r % 2 == 0 else order[::-1]):
        window[tag].append(back_to_back(lambda: A.coverage(p, S)) * 1e3)
full, stream = statistics.median(window["coverage"]), statistics.median(window["stream_only"])
got, ref = A.coverage(polygons, S), pillow_route()
agree = [float(((g - r).abs() <= S).float().mean()) for g, r in zip(got, ref)]
res = {"workload": f"{B} slides, K = {K} x {L} levels: a {X} x {Y} finest raster each, s = {S}, {polygons.P // B} polygons and "
                   f"{polygons.V // B} vertices per slide", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
       "coverage_ms": T.summ(ms["coverage"]), "pillow_ms": T.summ(ms["pillow"]),
       "pillow_over_coverage": round(statistics.median(ms["pillow"]) / statistics.median(ms["coverage"]), 1),
       "coverage_window_us": T.summ(window["coverage"]), "stream_only_window_us": T.summ(window["stream_only"]),
       "cells_within_s_of_pillow": round(min(agree), 4)}
res.update(culling_counts(polygons))
res["bound"] = ("edge streaming and the store: the window without any kept edge is %.0f%% of the full one" % (100 * stream / full) if stream > 0.5 * full
                else "the edge evaluation: the window without any kept edge is %.0f%% of the full one" % (100 * stream / full))
res["draw"] = []
for c in (4, 16):
    images = [torch.zeros((g[0] * f * c, g[1] * f * c, 3), dtype=torch.uint8, device=dev) for g in grids]
    A.draw(images, polygons, c)
    host = [T.timed(lambda: A.draw(images, polygons, c)) for _ in range(args.rounds)]
    dev_us = [back_to_back(lambda: A.draw(images, polygons, c)) * 1e3 for _ in range(args.rounds)]
    res["draw"].append({"cell_px": c, "steps": int(A.step_table(polygons, c)[-1]), "draw_ms": T.summ(host), "draw_window_us": T.summ(dev_us)})
    del images
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
