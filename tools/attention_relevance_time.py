#!/usr/bin/env python3
"""Cost of the gradient-weighted attention relevance (paths_amd.saliency.attention_relevance, csrc/attn_relevance.hip) at the headline
shape (K = 2,048 patches per level, 8 slides, 5 levels, bench weights and slides): attention_relevance against input_gradients on the
same batch, A/B/A/B in one process so that clock drift hits both alike; then the seed and the step alone at every level's own
(T, num_ims), timed with device events over back-to-back launches, with the achieved TFLOP/s of the step's two score products
(S^T = K Q^T and G^T = V dO^T: 2 * 2 * H * hd * sum_b T_b^2 floating-point operations over the valid tokens)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from paths_amd import saliency
from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch

dev = torch.device("cuda:0")
cfg, model, sd = bench.build_model(2048, dev, None)
slides = DeviceSlideBatch([DeviceSlide.synthetic(1234, i, bench.BASE_SHAPES[2048], device=dev) for i in range(8)])
L = cfg.num_levels
FNS = {"input_gradients": saliency.input_gradients, "attention_relevance": saliency.attention_relevance}


def call(name):
    return FNS[name](model, slides, cfg.top_k_patches, L)


for name in ("input_gradients", "attention_relevance") * 2:          # warm-up: packs, images, allocator
    out, trace = call(name)
torch.cuda.synchronize()
STEPS, ROUNDS = 10, 6
t = {name: [] for name in FNS}
for r in range(ROUNDS):
    for name in (tuple(FNS) if r % 2 == 0 else tuple(FNS)[::-1]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            call(name)
        torch.cuda.synchronize()
        t[name].append((time.perf_counter() - t0) / STEPS * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
a, b = med["input_gradients"], med["attention_relevance"]
print(f"K = 2048 x 8 slides x {L} levels: input_gradients {a:.3f} ms/call, attention_relevance {b:.3f} ms/call "
      f"(+{b - a:.3f} ms, +{(b / a - 1) * 100:.1f} %); rounds: {[round(x, 3) for x in t['input_gradients']]} / "
      f"{[round(x, 3) for x in t['attention_relevance']]}", flush=True)

# the two kernels alone at every level's own shape: operands of the shipped geometry's form (head-major, pre-scaled q), random values
# with a statistic that keeps every probability finite - the kernels' time does not depend on the values
mc = cfg.model_config
H, hd = mc.trans_heads, mc.trans_dim // mc.trans_heads
gen = torch.Generator(device=dev).manual_seed(0)
tot = {"seed": 0.0, "step": 0.0}
for l, rec in enumerate(trace):
    num_ims = rec["num_ims"].contiguous()
    B, T = num_ims.shape[0], rec["importance"].shape[1] + 1
    q, k, v = (torch.randn((B, H, T, hd), device=dev, generator=gen) for _ in range(3))
    d_o = torch.randn((B, T, H * hd), device=dev, generator=gen)
    lse = torch.full((B, H, T), 30.0, device=dev)
    r_in = torch.ones((B, T), device=dev)
    launches = {"seed": lambda: saliency.relevance_seed(q, k, v, 1.0, d_o[:, 0], lse[:, :, 0], num_ims),
                "step": lambda: saliency.relevance_step(q, k, v, 1.0, d_o, lse, num_ims, r_in, outputs=True)}
    flop = 2.0 * 2.0 * H * hd * float(((num_ims.clamp(0, T - 1) + 1).double() ** 2).sum())
    for name, fn in launches.items():
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 50
        tot[name] += us * (1 if name == "seed" else mc.trans_layers - 1)
        print(f"level {l}: {name}, B = {B}, T = {T}, valid tokens {int(num_ims.min()) + 1} .. {int(num_ims.max()) + 1}, H = {H}, hd = {hd}: "
              f"{us:.1f} us" + (f" ({flop / us / 1e6:.1f} TFLOP/s of the two score products)" if name == "step" else ""), flush=True)
print(f"all levels: seeds {tot['seed']:.1f} us, steps {tot['step']:.1f} us ({mc.trans_layers - 1} per level)", flush=True)
