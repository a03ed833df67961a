#!/usr/bin/env python3
"""Cost of the pixel side per level of a batch (paths_amd.pixels; csrc/tiles.hip): 8,192 tiles of 256 x 256 pixels (1.6 GB
of bytes in, 3.2 GB of fp16 encoder input out when all are tissue), about a third of them blank, in three phases, each against the
torch chain a caller writes today for the same bytes:

    tissue     pixels.tile_tissue (paths_tile_tissue + paths_tile_compact + its one host read of m)
               torch: lattice-sample, grey in integers, compare, mean, nonzero, the host read of m
    input      pixels.encoder_input for the m tissue tiles in chunks of --batch tiles, ImageNet normalisation, fp16
               torch: index, permute / float / div / normalise / half, per chunk
    rows       pixels.scatter_rows of [m, 1024] fp16 encoder rows into [n, 1024] fp32
               torch: zeros + index_copy of the cast rows

One JSON object, written to --out (default profiles/tiles_time.json) and printed: per phase the median / min / max milliseconds of
both sides over --rounds alternating rounds in one process (A/B, then B/A; a host clock around calls that end in a device
synchronise), ``torch_over_ours``, and for ``input`` the bytes moved over the 6.3 TB/s HBM rate the project measures against.  The
results of both sides are compared once before timing: flags, order and rows must be equal; the inputs may differ in the last bit
(torch divides by 255 on the device as a multiplication by the reciprocal; the table holds the host's true division) and the largest
difference is reported.

    python tools/tiles_time.py [--limit 420] [--rounds 6] [--tiles 8192] [--batch 256] [--out profiles/tiles_time.json]

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
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--tiles", type=int, default=8192)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles_time.json"))
args = ap.parse_args()
assert args.rounds >= 6, "the medians are taken over at least 6 rounds"

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--warmup", args.warmup, "--tiles", args.tiles, "--batch", args.batch, "--out", args.out])

import torch  # noqa: E402

from paths_amd import pixels  # noqa: E402

P, DIM, STRIDE, THR = 256, 1024, 4, 0.1
HBM_GBS = 6300.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
dev = torch.device("cuda:0")
n = args.tiles
gen = torch.Generator(device=dev).manual_seed(0)
tiles = torch.randint(0, 200, (n, P, P, 3), dtype=torch.uint8, device=dev, generator=gen)
tiles[::3] = 255                                                      # a third of the tiles are blank
t = pixels.otsu_threshold([tiles[k] for k in range(0, n, max(1, n // 16))])
table = pixels.normalize_table(MEAN, STD, torch.float16).to(dev)
mean, std = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)
at = torch.arange(P // STRIDE, device=dev) * STRIDE + STRIDE // 2


def ours_tissue():
    return pixels.tile_tissue(tiles, t, THR, STRIDE)


def torch_tissue():
    s = tiles[:, at][:, :, at].to(torch.int32)
    g = (4899 * s[..., 0] + 9617 * s[..., 1] + 1868 * s[..., 2] + 8192) >> 14
    flags = (g < t).double().mean(dim=(1, 2)) > THR
    order = torch.nonzero(flags).flatten()
    return flags, order, int(order.numel())


ts = ours_tissue()
flags_t, order_t, m_t = torch_tissue()
assert ts.m == m_t and torch.equal(ts.flags.bool(), flags_t) and torch.equal(ts.order[:ts.m].long(), order_t)
m = ts.m
chunks = [(first, min(args.batch, m - first)) for first in range(0, m, args.batch)]


def ours_input():
    for first, count in chunks:
        pixels.encoder_input(ts.tiles, ts.order, first, count, table)       # (the tile table of tile_tissue, as TileEncoder does)


def torch_input_chunk(first, count):
    return tiles[order_t[first:first + count]].permute(0, 3, 1, 2).float().div(255).sub(mean).div(std).half()


def torch_input():
    for first, count in chunks:
        torch_input_chunk(first, count)


first, count = chunks[len(chunks) // 2]
input_diff = float((pixels.encoder_input(tiles, ts.order, first, count, table).float() - torch_input_chunk(first, count).float()).abs().max())
encoded = torch.randn((m, DIM), device=dev, generator=gen).half()


def ours_rows():
    return pixels.scatter_rows(encoded, ts.slots, n, DIM, torch.float32)


def torch_rows():
    return torch.zeros((n, DIM), dtype=torch.float32, device=dev).index_copy_(0, order_t, encoded.float())


assert torch.equal(ours_rows(), torch_rows())

res = {"workload": f"{n} tiles of {P} x {P} pixels ({n * P * P * 3 / 1e9:.2f} GB), {m} with tissue, stride {STRIDE}, encoder input in fp16 in chunks of "
                   f"{args.batch} tiles ({m * 3 * P * P * 2 / 1e9:.2f} GB), rows [{m}, {DIM}] fp16 -> [{n}, {DIM}] fp32",
       "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "threshold": t, "tissue_tiles": m,
       "input_max_abs_difference_to_torch_on_device": input_diff, "hbm_rate_GB_per_s": HBM_GBS}
for phase, ours, theirs in (("tissue", ours_tissue, torch_tissue), ("input", ours_input, torch_input), ("rows", ours_rows, torch_rows)):
    runs = {"ours": ours, "torch": theirs}
    for fn in runs.values():
        for _ in range(args.warmup):
            fn()
    ms = T.alternating(runs, args.rounds)
    res[phase] = {"ours_ms": T.summ(ms["ours"]), "torch_ms": T.summ(ms["torch"]),
                  "torch_over_ours": round(statistics.median(ms["torch"]) / statistics.median(ms["ours"]), 2)}
moved = m * P * P * 3 + m * 3 * P * P * 2
rate = moved / (res["input"]["ours_ms"]["median"] * 1e-3) / 1e9
res["input"].update({"bytes_moved_GB": round(moved / 1e9, 2), "GB_per_s": round(rate, 1), "of_hbm_rate": round(rate / HBM_GBS, 3)})
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
