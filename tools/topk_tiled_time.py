#!/usr/bin/env python3
"""Cost of the tiled top-K (csrc/topk_tiled.hip) beside the LDS-resident one (csrc/select.hip): B = 8 slides, keep = 2048, the
synthetic score rows of tests/test_gpu_select.py (normal values, a run of exact ties at the boundary, signed zeros, special values),
every slide full.  One JSON object, written to --out (default profiles/topk_tiled_time.json) and printed:

    at_8192     paths_topk_rows and paths_topk_rows_tiled on the same buffers, alternating rounds in one process (A/B, then B/A):
                microseconds per launch (median, min, max over the rounds) and the ratio of the medians - what streaming the keys
                through a 16-KiB tile costs where both forms apply.  It decides nothing: the dispatch stays at the LDS limit.
    tiled       paths_topk_rows_tiled alone at n = 16,384, 32,768 and 65,535: microseconds per launch, and the rate of 64-bit
                compares (B n^2 per launch) it amounts to

Every figure is event-timed: ``--reps`` launches back to back between two events on an otherwise idle device, divided by their
number; outputs of the two forms are compared once before anything is timed.

    python tools/topk_tiled_time.py [--limit 300] [--rounds 7] [--reps 20] [--out profiles/topk_tiled_time.json]

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
ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (at least 5)")
ap.add_argument("--reps", type=int, default=20, help="launches per timed round")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_tiled_time.json"))
args = ap.parse_args()
assert args.rounds >= 5, "the medians are taken over at least 5 rounds"

if not args.child:
    T.run_in_child(__file__, args.limit, ["--rounds", args.rounds, "--reps", args.reps, "--warmup", args.warmup, "--out", args.out])

import numpy as np  # noqa: E402
import torch  # noqa: E402

from paths_amd import _lib  # noqa: E402
from tests.test_gpu_select import _topk_scores  # noqa: E402

B, KEEP = 8, 2048
dev = torch.device("cuda:0")


def case(n):
    rng = np.random.default_rng(n)
    sc = torch.from_numpy(_topk_scores(rng, n, [n] * B, KEEP, 0)).to(dev)
    num = torch.full((B,), n, dtype=torch.int64, device=dev)
    table, zero_row = torch.zeros((B, n, 4), device=dev), torch.zeros((4,), device=dev)
    out = lambda: (torch.zeros((B, KEEP), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev),
                   torch.zeros((B, KEEP), dtype=torch.int64, device=dev))

    def launcher(name, bufs):
        ki, kc, kr = bufs
        a = (sc.data_ptr(), n, num.data_ptr(), B, n, KEEP, ki.data_ptr(), KEEP, kc.data_ptr(), table.data_ptr(), 4, n, kr.data_ptr(),
             zero_row.data_ptr())
        return lambda: _lib.call(name, *a, _lib.stream())

    return out, launcher, (sc, num, table, zero_row)


def timed_us(fn) -> float:
    """Microseconds per launch: args.reps launches between two events."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.reps


# --- both forms at n = 8192, the largest size the LDS-resident kernel takes
out, launcher, hold = case(8192)
old_bufs, new_bufs = out(), out()
runs = {"paths_topk_rows": launcher("paths_topk_rows", old_bufs), "paths_topk_rows_tiled": launcher("paths_topk_rows_tiled", new_bufs)}
for fn in runs.values():
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
assert all(torch.equal(a, b) for a, b in zip(old_bufs, new_bufs)), "the two forms disagree"
us = T.alternating(runs, args.rounds, measure=timed_us)
med = {k: statistics.median(v) for k, v in us.items()}
res = {"workload": f"{B} slides, keep = {KEEP}, every slide full, score rows of tests/test_gpu_select.py::_topk_scores",
       "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "launches_per_round": args.reps,
       "at_8192": {"paths_topk_rows_us": T.summ(us["paths_topk_rows"]), "paths_topk_rows_tiled_us": T.summ(us["paths_topk_rows_tiled"]),
                   "tiled_over_resident": round(med["paths_topk_rows_tiled"] / med["paths_topk_rows"], 2)},
       "tiled": []}
del hold, old_bufs, new_bufs, runs

# --- the tiled form alone past the LDS limit
for n in (16384, 32768, 65535):
    out, launcher, hold = case(n)
    fn = launcher("paths_topk_rows_tiled", out())
    for _ in range(args.warmup):
        fn()
    v = [timed_us(fn) for _ in range(args.rounds)]
    m = statistics.median(v)
    res["tiled"].append({"n": n, "us": T.summ(v), "compares": B * n * n, "compares_per_s": float(f"{B * n * n / (m * 1e-6):.3g}")})
    del hold, fn

print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
