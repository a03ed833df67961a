#!/usr/bin/env python3
"""Cost of the special token's attention rollout (utils.recurse(..., rollout=True), csrc/attn_rollout.hip) at the headline shape
(K = 2,048 patches per level, 8 slides, 5 levels, bench weights and slides): eager steps with and without the rollout, interleaved in
rounds so that clock drift hits both alike; plus the rollout's own launches (prepare, seed, step) on one level's layer inputs."""
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


def step(ro: bool):
    tr = []
    with torch.no_grad():
        putils.recurse(model, slides, cfg.top_k_patches, cfg.num_levels, trace=tr, check_status=False, rollout=ro)
    return tr


for ro in (False, True, False, True):            # warm-up: packs, images, allocator
    step(ro)
torch.cuda.synchronize()
STEPS, ROUNDS = 20, 5
t = {False: [], True: []}
for r in range(ROUNDS):
    for ro in ((False, True) if r % 2 == 0 else (True, False)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step(ro)
        torch.cuda.synchronize()
        t[ro].append((time.perf_counter() - t0) / STEPS * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
print(f"eager recurse, K = 2048 x 8 slides x 5 levels: without rollout {med[False]:.3f} ms/step, with {med[True]:.3f} ms/step "
      f"(+{(med[True] / med[False] - 1) * 100:.1f} %); rounds: {[round(x, 3) for x in t[False]]} / {[round(x, 3) for x in t[True]]}", flush=True)

# the rollout's launches alone on one level's tokens (T = 2,049), timed with events over back-to-back launches
mc = cfg.model_config
B, T, d, H = 8, 2049, mc.trans_dim, mc.trans_heads
x = torch.randn((B, T, d), device=dev)
num_ims = torch.full((B,), T - 1, device=dev, dtype=torch.int64)
lay = ops.pack_level(model.procs[0])["layers"][0]
ws = torch.empty((int(_lib.load().paths_attention_rollout_workspace(B, T, d, H)),), device=dev)
att = (torch.rand((B, 1, H, T - 1), device=dev) / T, torch.rand((B, 1, H), device=dev) / T)
r = torch.empty((B, T), device=dev)
out = (torch.empty((B, T - 1), device=dev), torch.empty((B,), device=dev))
p, st = _lib.ptr, _lib.stream()
launches = {
    "prepare": lambda: _lib.call("paths_attention_rollout_prepare", p(x), p(num_ims), p(lay["w_in"]), p(lay["b_in"]), p(ws), B, T, d, H, 0, st),
    "seed": lambda: _lib.call("paths_attention_rollout_seed", p(att[0]), H * (T - 1), p(att[1]), H, p(num_ims), p(r), None, 0, None, B, T, H, st),
    "step": lambda: _lib.call("paths_attention_rollout_step", p(ws), p(num_ims), p(r), None, p(out[0]), T - 1, p(out[1]), B, T, d, H, st),
}
for fn in launches.values():
    for _ in range(5):
        fn()
for name, fn in launches.items():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 50
    flop = 2.0 * B * H * T * T * (d // H) if name != "seed" else 0.0
    print(f"{name}, B = {B}, T = {T}, d = {d}, H = {H}: {us:.1f} us" + (f" ({flop / us / 1e6:.1f} TFLOP/s of score products)" if flop else ""),
          flush=True)
