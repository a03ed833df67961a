#!/usr/bin/env python3
"""Cost of the special token's attention export (utils.recurse(..., attention=True), csrc/attn_token0.hip: paths_token0_attention) at the
headline shape (K = 2,048 patches per level, 8 slides, 5 levels, bench weights and slides): eager steps with and without the export,
interleaved in rounds so that clock drift hits both alike; plus the export's own launches on one level's layer inputs."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from paths_amd import _lib, ops
from paths_amd import utils as putils
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch

dev = torch.device("cuda:0")
cfg, model, sd = bench.build_model(2048, dev, None)
slides = DeviceSlideBatch([DeviceSlide.synthetic(1234, i, bench.BASE_SHAPES[2048], device=dev) for i in range(8)])


def step(att: bool):
    tr = []
    with torch.no_grad():
        putils.recurse(model, slides, cfg.top_k_patches, cfg.num_levels, trace=tr, check_status=False, attention=att)
    return tr


for att in (False, True, False, True):           # warm-up: packs, images, allocator
    step(att)
torch.cuda.synchronize()
STEPS, ROUNDS = 20, 5
t = {False: [], True: []}
for r in range(ROUNDS):
    for att in ((False, True) if r % 2 == 0 else (True, False)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step(att)
        torch.cuda.synchronize()
        t[att].append((time.perf_counter() - t0) / STEPS * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
print(f"eager recurse, K = 2048 x 8 slides x 5 levels: without export {med[False]:.3f} ms/step, with {med[True]:.3f} ms/step "
      f"(+{(med[True] / med[False] - 1) * 100:.1f} %); rounds: {[round(x, 3) for x in t[False]]} / {[round(x, 3) for x in t[True]]}", flush=True)

# the export alone: one layer of the deepest level's tokens (T = 2,049), timed with events over back-to-back launches
mc = cfg.model_config
B, T, d, H = 8, 2049, mc.trans_dim, mc.trans_heads
x = torch.randn((B, T, d), device=dev)
num_ims = torch.full((B,), T - 1, device=dev, dtype=torch.int64)
lvl = ops.pack_level(model.procs[0])
att = (torch.empty((B, mc.trans_layers, H, T - 1), device=dev), torch.empty((B, mc.trans_layers, H), device=dev))
for _ in range(10):
    ops._export_attention(att, lvl, 0, x, num_ims, H, 0)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(100):
    ops._export_attention(att, lvl, 0, x, num_ims, H, 0)
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 10
print(f"one layer's export, B = {B}, T = {T}, d = {d}, H = {H}: {us:.1f} us ({B * T * d * 4 * H / us / 1e3:.0f} GB/s of layer rows read per head)", flush=True)
