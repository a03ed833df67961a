#!/usr/bin/env python3
"""Host-resident slides (paths_amd.data_utils.slide.HostSlide) at the headline shape: 8 slides at K = 2048 x 5 levels whose grids stay
in pinned host memory (22.9 GB as fp32, 11.4 GB as fp16), against the same slides resident in HBM and against uploading a slide that
is not resident (DeviceSlide.from_host + recurse, what a cohort beyond HBM had to do before).  One JSON line per dtype:

    stage_us_per_level      the staging launch of every level alone, event-timed on an otherwise idle device, with the bytes it
                            staged and the host-link rate (bytes / time) beside the 63 GB/s PCIe Gen5 x16 spec figure
    host_slides_per_s       TapedRecursion replay on the host batch
    resident_slides_per_s   the same tape on the resident twins, same process
    upload_slides_per_s     DeviceSlide.from_host of the same pinned grids + recurse, per slide

    python tools/host_slides_time.py [--dtypes fp32,fp16] [--limit 420]

Each dtype runs in a fresh child process under ``timeout -k 10 <limit>``; the first failure ends the run."""
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
ap.add_argument("--dtypes", default="fp32,fp16")
ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
ap.add_argument("--child", default=None, help="(internal) run one dtype in this process")
ap.add_argument("--steps", type=int, default=20, help="replays per timed run")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()

if args.child is None:
    for name in args.dtypes.split(","):
        rc = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", name,
                             "--steps", str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]).returncode
        if rc != 0:
            print(f"host_slides_time: {name} ended with status {rc}; stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402

import bench  # noqa: E402
from paths_amd import _lib  # noqa: E402
from paths_amd import utils as putils  # noqa: E402
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch, HostSlide  # noqa: E402

K, SPG, SPEC_GBS = 2048, 8, 63.0
dtype = {"fp32": torch.float32, "fp16": torch.float16}[args.child]
dev = torch.device("cuda:0")
cfg, model, _ = bench.build_model(K, dev, None)
keep, L = cfg.top_k_patches, cfg.num_levels

# the pyramids are generated on the device (the resident twins) and copied into pinned memory; HostSlide's own constructor then runs
# the chunked mask pass over the pinned grids
twins = [DeviceSlide.synthetic(1234, i, bench.BASE_SHAPES[K], device=dev, dtype=dtype) for i in range(SPG)]
host, mask_ms = [], []
for s in twins:
    grids = []
    for g in s.grids:
        h = torch.empty(g.shape, dtype=g.dtype, pin_memory=True)
        h.copy_(g)
        grids.append(h)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hs = HostSlide(grids, device=dev, slide_id=s.slide_id)
    mask_ms.append((time.perf_counter() - t0) * 1e3)
    assert all(torch.equal(a, b) for a, b in zip(hs.masks, s.masks)) and hs.feature_absmax() == s.feature_absmax()
    host.append(hs)
hb, rb = DeviceSlideBatch(host), DeviceSlideBatch(twins)
pinned_gb = sum(s.host_bytes() for s in host) / 1e9
row_bytes = hb.dim * host[0].grids[0].element_size()

# --- the staging launch of every level alone: an eager pass whose staging calls are bracketed by events on an idle device
real_call, stage_us = _lib.call, []


def timed_call(name, *a):
    if name != "paths_stage_rows":
        return real_call(name, *a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.ExternalStream(a[-1], device=dev)
    e0.record(stream)
    real_call(name, *a)
    e1.record(stream)
    torch.cuda.synchronize()
    stage_us.append(e0.elapsed_time(e1) * 1e3)


per_level = []
with torch.no_grad():
    putils.recurse(model, hb, keep, L)                       # warm-up: packs, images
    for rep in range(5):
        stage_us.clear()
        trace = []
        _lib.call = timed_call
        try:
            out_h = putils.recurse(model, hb, keep, L, trace=trace)
        finally:
            _lib.call = real_call
        assert len(stage_us) == L and int(out_h["status"].item()) == 0
        per_level.append(list(stage_us))
    staged_rows = [int(t["num_ims"].sum()) for t in trace]
    out_r = putils.recurse(model, rb, keep, L)
    assert torch.equal(out_h["logits"], out_r["logits"]) and torch.equal(out_h["ctx_slide"], out_r["ctx_slide"]), "host / resident outputs differ"
med_us = [statistics.median(r[l] for r in per_level) for l in range(L)]
stage = [{"level": l, "rows": staged_rows[l], "MB": round(staged_rows[l] * row_bytes / 1e6, 1), "us": round(med_us[l], 1),
          "GB_per_s": round(staged_rows[l] * row_bytes / (med_us[l] * 1e-6) / 1e9, 2)} for l in range(L)]
total_bytes = sum(staged_rows) * row_bytes

# --- taped replay: host batch against its resident twins, alternating rounds
tapes = {"host": putils.TapedRecursion(model, hb, keep, L).record(), "resident": putils.TapedRecursion(model, rb, keep, L).record()}


def run(name, steps):
    t = tapes[name]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for _ in range(steps):
            t.replay()
    torch.cuda.synchronize()
    return SPG * steps / (time.perf_counter() - t0)


for name in tapes:
    run(name, args.warmup)
rates = {"host": [], "resident": []}
for r in range(args.rounds):
    for name in (("host", "resident") if r % 2 == 0 else ("resident", "host")):
        rates[name].append(run(name, args.steps))
with torch.no_grad():
    assert torch.equal(tapes["host"].replay()["logits"], tapes["resident"].replay()["logits"])
for t in tapes.values():
    t.close()

# --- what a slide that is not resident cost before: upload every grid, then recurse (per slide, batch of one)
del rb, twins, tapes
torch.cuda.empty_cache()
up = []
with torch.no_grad():
    for rnd in range(2):                                     # (the first round warms the allocator and the batch-of-one shapes)
        for s in host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = DeviceSlide([g.to(dev, non_blocking=True) for g in s.grids])       # (DeviceSlide.from_host of grids that already have the dtype)
            o = putils.recurse(model, [d], keep, L)
            torch.cuda.synchronize()
            if rnd == 1:
                up.append(time.perf_counter() - t0)
            del d, o
summ = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
host_rate, res_rate, up_rate = statistics.median(rates["host"]), statistics.median(rates["resident"]), 1.0 / statistics.median(up)
print(json.dumps({
    "workload": f"K = {K} x {L} levels, {SPG} slides per batch, grids {args.child}", "device": torch.cuda.get_device_name(dev),
    "pinned_GB": round(pinned_gb, 2), "mask_pass_ms_per_slide": round(statistics.median(mask_ms), 1),
    "stage_us_per_level": stage, "staged_MB_per_step": round(total_bytes / 1e6, 1),
    "stage_GB_per_s": round(total_bytes / (sum(med_us) * 1e-6) / 1e9, 2), "link_spec_GB_per_s": SPEC_GBS,
    "host_slides_per_s": summ(rates["host"]), "resident_slides_per_s": summ(rates["resident"]),
    "upload_slides_per_s": round(up_rate, 2), "upload_ms_per_slide": summ([x * 1e3 for x in up]),
    "host_over_upload": round(host_rate / up_rate, 1), "host_over_resident": round(host_rate / res_rate, 4),
    "steps_per_run": args.steps, "rounds": args.rounds}), flush=True)
