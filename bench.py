#!/usr/bin/env python3
"""Headline benchmark: slides/sec of the 5-level PATHS recursion at K=2048 patches/level x 1024-dim features
(BASELINE.json metric), on N GPUs of one node.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path (reference utils.py:228-279: 5 x [level forward, top-K, child expansion,
gather]) over one batch of synthetic slides that are ALREADY RESIDENT in HBM.  Slides are independent, so ranks
shard the batch with no data-path collective (weak scaling: --slides-per-gpu slides per rank); the only
collectives are the barriers around the timed region and a MAX-reduce of the elapsed time.

Rank 0 prints ONE JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step, the run's shape and config).  A plain
run does only what that line needs: set up, warm up, time the steps, write --dump-outputs, print.  Everything else the benchmark
measures runs with --full, after the timed steps, and adds its objects to the line (infer mode: single_batch, sustained,
launch_modes, serialized_breakdown, train, k1024, trans_dim_192, stress, parity_checked, and the two below):
  roofline     dominant kernel (output-gate GEMM of the LSTM cell) timed with events on its launch stream over the same K
               steps (an eager instrumented pass; --eager: the timed steps themselves); achieved = algorithmic FLOP (2 M N K) /
               measured duration.  Default build
               (PATHS_GEMM_MODE=h3): the GEMM multiplies fp32 operands as 2 fp16 planes with 3 MFMAs per product block
               (csrc/gemm_x6.hip), so its ceiling is the dense 16-bit MFMA peak / 3; "x6": 3 bf16 planes, 6 MFMAs, peak / 6;
               "f32": the f32-input MFMA kernel (peak 157.3 TFLOP/s).
  cpu_baseline the oracle (oracle/paths_oracle.py, plain torch CPU ops) timed on this box's host cores on a bounded
               sample of the same workload (rank 0, N=1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md "Peak FP32 (matrix)" (measured 155)
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense"
MFMA_PER_PRODUCT = {3: 6, 2: 3}   # 16-bit MFMAs issued per fp32 product block: 3 bf16 planes ("x6") / 2 fp16 planes ("h3")
BASE_SHAPES = {2048: (32, 64), 1024: (32, 32), 256: (16, 16)}
PMC_PROFILE_H3 = "r05fin_pmc_traffic.json"     # separate --pmc passes of the default build in round 5 (tools/refresh_profiles.sh)
ROOFLINE_FILE = "roofline.json"               # measured MFMA issue peak / stream bandwidth of the pool's boxes (tools/peaks.hip)
CPU_DSEED = 1234
# slide ids of the cpu_baseline / parity sample: screened here with the oracle so that every level's top-K boundary gap
# (score[k-1] - score[k]) is >= 1e-5 with the bench weights (seed 0) - the reference's own selection is thread-count
# dependent below ~1e-6 (hard part 1); id 10001 at K=2048 has a 2.4e-7 gap at level 0 and is left out
# (round 4: 10006-10008, 10011, 10014 added so that the parity sample is a FULL 8-slide batch; 10002 (2.1e-6 at level 2), 10009,
# 10010 and 10012 have gaps < 1e-5)
CPU_SLIDE_IDS = {2048: [10003, 10004, 10005, 10006, 10007, 10008, 10011, 10014], 1024: [10000, 10001, 10003, 10002], 256: [10000, 10001, 10002, 10003]}
DUMP_BYTES = 64 << 20             # --dump-outputs: at most this much in all
DUMP_SEED = 0                     # --dump-outputs: the fixed sample of rows / elements of outputs too large to write whole
DUMP_ROWS = 512                   # --dump-outputs: ctx_patch rows sampled per slide (fewer if the budget needs it)


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def measured_peaks():
    """profiles/roofline.json: the denominators measured on the box next to the spec values."""
    try:
        with open(os.path.join(ROOT, "profiles", ROOFLINE_FILE)) as fh:
            return json.load(fh)
    except (OSError, ValueError):
        return None


def host_cpu_share() -> int:
    """Cores this process may really use: min(affinity, cgroup cpu quota, PATHS_CPU_THREADS or 16).  A GPU box shows
    every core of the host (256) but gives one GPU job a 16-core share; oversubscribing makes torch CPU ops crawl."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, int(os.environ.get("PATHS_CPU_THREADS", "16"))))


def host_cpu_share_all() -> int:
    """:func:`host_cpu_share` without the 16-thread cap: every core the job may use (self-launch splits them among its ranks)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def recursion_outputs(out, budget: int = DUMP_BYTES) -> dict:
    """--dump-outputs of a recursion step: what recurse() / a tape replay hands its caller (the last level's outputs), copied to
    the host.  logits, ctx_slide and importance whole; ctx_patch ([B, N, D + Hc], 84 MB at K = 2048 x 8 slides) as the same
    seeded sample of row positions in every slide, with its padding rows (zero importance: the kernels never write them) zeroed."""
    res = {k: out[k].detach().float().cpu().numpy() for k in ("logits", "ctx_slide", "importance")}
    cp, imp = out["ctx_patch"], out["importance"]
    B, N, Dp = cp.shape
    rows = max(1, min(N, DUMP_ROWS, (budget - sum(a.nbytes for a in res.values())) // (4 * B * Dp + 8)))
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(DUMP_SEED))[:rows].sort().values.to(cp.device)
    sample = cp.index_select(1, idx) * (imp.index_select(1, idx) != 0).unsqueeze(-1)
    res["ctx_patch_sample"] = sample.float().cpu().numpy()
    res["ctx_patch_sample_rows"] = idx.double().cpu().numpy()
    return res


def write_outputs(path: str, arrays: dict) -> None:
    """--dump-outputs: every array as ``path/<name>.npy`` (float32 / float64); arrays too large for what is left of the budget are
    written as a fixed seeded sample of their elements (flattened)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    left, written = DUMP_BYTES - 128 * len(arrays), 0          # (each .npy header: 128 bytes)
    for name, a in sorted(arrays.items(), key=lambda kv: kv[1].nbytes):
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        if a.nbytes > left:
            keep = left // a.itemsize
            a = a.reshape(-1)[np.sort(np.random.RandomState(DUMP_SEED).choice(a.size, keep, replace=False))]
            name += "_sample"
        np.save(os.path.join(path, name + ".npy"), a)
        left -= a.nbytes
        written += a.nbytes
    log(f"outputs of the last timed step written to {path}: {', '.join(sorted(arrays))} ({written / 2**20:.1f} MB)")


def build_model(K: int, dev, dropout=None, trans_dim=None):
    from paths_amd import synthetic as syn
    from paths_amd.config import Config
    cfg = Config.load(os.path.join(ROOT, "tests", "golden", "sample"), test_mode=True)
    if dropout is not None:               # (None: the shipped value, models/sample/config.json: 0.05; only train mode reads it)
        cfg.model_config.dropout = float(dropout)
    if trans_dim is not None:             # (td192 probe: the reference's dataclass default width, config.py:30)
        cfg.model_config.trans_dim = int(trans_dim)
    cfg.top_k_patches = [K // 4] * (cfg.num_levels - 1)
    model = cfg.get_model()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = syn.make_state_dict(0, shapes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return cfg, model.to(dev).eval(), sd


def gemm_split(cfg, batch):
    """(x6, planes) of the recursion's LSTM output-gate GEMM on ``batch``, as its launch reports them to the kernel timer
    (paths_amd/ops.py level_forward), known without running a step: split-operand kernels or not, and 2 (fp16) / 3 (bf16) planes."""
    from paths_amd import ops
    mc = cfg.model_config
    if not mc.lstm:                      # (no LSTM cell: no output-gate launch, the line says "f32")
        return False, 0
    with ops.range_guard(batch.feat_absmax):
        x6 = ops.use_x6(batch.dim, mc.hierarchical_ctx_mlp_hidden_dim)
        return x6, (ops.split_planes() if x6 else 0)


def infer_dtype(x6: bool, planes: int) -> str:
    return ("f32 (products as 2 fp16 planes per operand = 22 bits, 3 fp16 MFMAs per block, fp32 accumulate)" if planes == 2 else
            "f32 (products as 3 exact bf16 planes per operand, 6 bf16 MFMAs per block, fp32 accumulate)" if x6 else "f32")


def infer_gemm_mode(x6: bool, planes: int) -> str:
    return (("h3: GEMM, attention and token-layer operands split into 2 fp16 planes (22 bits), 3 fp16 MFMAs per "
             "product block, fp32 accumulate, power-of-two scaling of weights / GEMM activations (error of the "
             "order of an fp32 FMA chain's); everything else fp32") if planes == 2 else
            ("x6: operands split exactly into 3 bf16 planes, 6 bf16 MFMAs per product block, fp32 "
             "accumulate (error <= an fp32 FMA chain's); everything else fp32") if x6 else "f32 MFMA")


def cpu_baseline(cfg, sd, K: int, n_slides: int, reps: int):
    """Oracle on the host cores: B = n_slides batch, full 5-level recursion, grids evaluated lazily and cached so
    the timed repetitions do not pay for input generation (the GPU side has its inputs resident too)."""
    from oracle import paths_oracle as orc
    from paths_amd import synthetic as syn

    class CachedGrids(orc.LazyGrids):
        def __init__(self, slide):
            super().__init__(slide)
            self.cache = {}

        def rows(self, level, x, y):
            key = (level, x.numpy().tobytes(), y.numpy().tobytes())
            if key not in self.cache:
                self.cache[key] = super().rows(level, x, y)
            return self.cache[key]

    threads = host_cpu_share()
    torch.set_num_threads(threads)
    log(f"cpu_baseline: {threads} threads (os.cpu_count()={os.cpu_count()}), {n_slides} slides x {reps} reps")
    ocfg = orc.OracleConfig(top_k_patches=list(cfg.top_k_patches))
    params = {k: torch.from_numpy(v) for k, v in sd.items()}
    n_slides = min(n_slides, len(CPU_SLIDE_IDS[K]))
    ids = CPU_SLIDE_IDS[K][:n_slides]
    grids = [CachedGrids(syn.SyntheticSlide(CPU_DSEED, i, BASE_SHAPES[K])) for i in ids]
    otrace = []
    with torch.no_grad():
        t0 = time.perf_counter()
        ohz, _ = orc.inference_end2end(params, ocfg, grids, None, otrace)     # warm-up + fills the row cache; kept for the parity check
        log(f"cpu_baseline: warm-up pass {time.perf_counter() - t0:.1f} s")
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            orc.inference_end2end(params, ocfg, grids)
            times.append(time.perf_counter() - t0)
            log(f"cpu_baseline: rep {times[-1]:.2f} s")
    times.sort()
    med = times[len(times) // 2]
    return {"value": n_slides / med, "unit": "slides/s", "cores": threads, "kind": "port",
            "sample": f"{n_slides} slides x {reps} timed repetitions (median) of the same 5-level K={K} recursion, "
                      f"fp32 torch CPU ops, {threads} threads, inputs cached"}, ids, otrace, ohz


def parity_check(cfg, model, K, ids, otrace, ohz, dev):
    """The cpu_baseline leg's oracle outputs against the HIP recursion on the SAME slides (outside the timed region): per
    level num_ims, location sets, kept (top-K) sets, (child -> parent) pairs bit-exact, importance and final hazards within
    tolerance (oracle/compare.py)."""
    from oracle.compare import compare_recursion
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    sl = DeviceSlideBatch([DeviceSlide.synthetic(CPU_DSEED, i, BASE_SHAPES[K], device=dev) for i in ids])
    trace = []
    with torch.no_grad():
        out = putils.recurse(model, sl, cfg.top_k_patches, cfg.num_levels, trace=trace)
    torch.cuda.synchronize()
    res = compare_recursion(trace, otrace, torch.sigmoid(out["logits"]), ohz, raise_on_mismatch=False)
    res["slide_ids"] = list(ids)
    if res["problems"]:
        log("PARITY MISMATCH vs oracle: " + "; ".join(res["problems"][:6]))
    return res


def stress_measure(trans_dim, trans_heads, fp8, steps, warmup, spg, rank, world, dev, dev_reduce, pdist, putils, outputs=None):
    """BASELINE.json configs[4] geometry: ONE level over K = 8192 patches of d = 1536 features per slide = full quadratic attention
    over 8193 tokens.  Measures the fp32-accurate (parity) path and, with ``fp8``, the opt-in e4m3 variants (whole aggregator; at
    trans_dim 128 / 4 heads also attention only) with their logit distance from the accurate path.  Returns a dict; ``outputs`` (a
    dict) receives the accurate path's last timed step (:func:`recursion_outputs`)."""
    from paths_amd import ops
    from paths_amd import synthetic as syn
    from paths_amd.config import Config
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    cfg = Config.load(os.path.join(ROOT, "tests", "golden", "sample"), test_mode=True)
    cfg.model_config.patch_embed_dim, cfg.num_levels, cfg.top_k_patches = 1536, 1, []
    cfg.model_config.trans_dim, cfg.model_config.trans_heads = trans_dim, trans_heads
    model = cfg.get_model()
    sd = syn.make_state_dict(0, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval()
    slides = DeviceSlideBatch([DeviceSlide.synthetic(1234, rank * spg + i, (64, 128), dim=1536, num_levels=1, device=dev)
                               for i in range(spg)])

    def step():
        with torch.no_grad():
            return putils.recurse(model, slides, [], 1, check_status=False)

    def barrier():
        torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()

    def timed_run(capture=False):
        for _ in range(warmup):
            step()
        barrier()
        ev = []

        def timer(name, launch, meta):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = launch()
            e1.record()
            ev.append((name, e0, e1))
            return r

        ops.KERNEL_TIMER, ops.TIMER_ALL = timer, True
        t0 = time.perf_counter()
        try:
            for _ in range(steps):
                out_ = step()
            barrier()
        finally:
            ops.KERNEL_TIMER, ops.TIMER_ALL = None, False
        el = pdist.max_over_ranks(time.perf_counter() - t0, dev_reduce)
        assert int(out_["status"].item()) == 0
        if capture:
            outputs.update(recursion_outputs(out_))
        att = [e0.elapsed_time(e1) * 1e3 for n, e0, e1 in ev if n == "agg_attention"]
        agg = [e0.elapsed_time(e1) * 1e3 for n, e0, e1 in ev if n == "aggregator"]
        timed_run.agg_us = sum(agg) / len(agg) if agg else None
        return el, out_["logits"].clone(), (sum(att) / len(att) if att else None)

    elapsed, logits, attn_us = timed_run(capture=outputs is not None)
    agg_us = timed_run.agg_us
    T_, d_, L_ = 8193, trans_dim, cfg.model_config.trans_layers
    # algorithmic FLOPs of the aggregator per step and GPU (24 T d^2 + 4 T^2 d per layer, degenerate cross-attention 0)
    agg_flops = spg * L_ * (24 * T_ * d_ * d_ + 4 * T_ * T_ * d_)
    fp8_agg = None
    if fp8 and ops.fp8_supported(cfg.model_config):
        # the whole aggregator's big products in e4m3 (csrc/gemm_fp8.hip + csrc/attn_fp8.hip): in_proj, the full layers' attention,
        # out_proj and the feed-forward pair; the first (warm-up) step calibrates the hidden layer's scale
        ops.AGG_FP8 = True
        try:
            el8, logits8, _ = timed_run()
        finally:
            ops.AGG_FP8 = False
        agg8_us = timed_run.agg_us
        diff = float((logits8 - logits).abs().max())
        fp8_agg = {"slides_per_s": round(spg * world * steps / el8, 2), "ms_per_step": round(el8 / steps * 1e3, 3),
                   "aggregator_us": round(agg8_us, 1) if agg8_us else None, "aggregator_us_accurate_path": round(agg_us, 1) if agg_us else None,
                   "max_logit_diff_vs_accurate_path": diff, "meets_1e-4_logit_bar": bool(diff <= 1e-4),
                   "what": "in_proj, full-layer attention, out_proj, linear1 / linear2 with e4m3 operands and per-tensor scales "
                           "(v_mfma_scale_f32_32x32x64_f8f6f4 GEMMs, fp8 attention); LayerNorm, residuals, the last layer's "
                           "token-0 row chain, the classifier and the whole selection chain (LSTM, importance, top-K) in fp32",
                   "roofline": None if not agg8_us else {
                       "bound": "mfma", "achieved": round(agg_flops / (agg8_us * 1e-6) / 1e12, 1), "peak": 5000.0, "unit": "TFLOP/s",
                       "frac": round(agg_flops / (agg8_us * 1e-6) / 1e12 / 5000.0, 4),
                       "note": "algorithmic aggregator FLOPs (L (24 T d^2 + 4 T^2 d) per slide) / event-timed aggregator span, against "
                               "the dense fp8 MFMA peak; the last layer runs at token 0 only, so the executed share is smaller"}}
    fp8_att = None
    if fp8 and trans_dim == 128 and trans_heads == 4:
        # the e4m3 attention variant (csrc/attn_fp8.hip) on the same batch: its speed AND its distance from the fp32-accurate logits
        ops.ATTN_FP8 = True
        try:
            el8, logits8, attn8_us = timed_run()
        finally:
            ops.ATTN_FP8 = False
        afl = spg * 4 * 8193 * 8193 * 128                                      # the full attention of layer 0, per launch
        fp8_att = {"slides_per_s": round(spg * world * steps / el8, 2), "ms_per_step": round(el8 / steps * 1e3, 3),
                   "attention_us": round(attn8_us, 1), "attention_us_split_path": round(attn_us, 1),
                   "max_logit_diff_vs_split_path": float((logits8 - logits).abs().max()),
                   "meets_1e-4_logit_bar": bool(float((logits8 - logits).abs().max()) <= 1e-4),
                   "roofline": {"bound": "mfma", "achieved": round(afl / (attn8_us * 1e-6) / 1e12, 1), "peak": 5000.0, "unit": "TFLOP/s",
                                "frac": round(afl / (attn8_us * 1e-6) / 1e12 / 5000.0, 4),
                                "note": "algorithmic 4 T^2 d FLOPs of the one full attention launch / its event-timed duration, against the "
                                        "dense fp8 MFMA peak; head_dim 32 gives one 16x16x32 k-step per score tile, the loop is exp2 / "
                                        "conversion (VALU) bound"}}
    del model, slides
    torch.cuda.empty_cache()
    return {"slides_per_s": round(spg * world * steps / elapsed, 2), "ms_per_step": round(elapsed / steps * 1e3, 3), "steps": steps, "warmup": warmup,
            "trans_dim": trans_dim, "trans_heads": trans_heads, "slides_per_gpu": spg,
            "attn_ffn_flops_per_step": agg_flops * world, "attention_us": round(attn_us, 1) if attn_us else None,
            "aggregator_us": round(agg_us, 1) if agg_us else None,
            "aggregator_frac_of_fp32_product_peak": round(agg_flops / (agg_us * 1e-6) / 1e12 / (PEAK_BF16_MFMA_TFLOPS / 3), 4) if agg_us else None,
            "fp8_attention": fp8_att, "fp8_aggregator": fp8_agg}


def stress_bench(args, rank, world, dev, dev_reduce, pdist, putils):
    """Extra line (BASELINE.json configs[4] geometry): ONE level over K = 8192 patches of d = 1536 features per slide = full
    quadratic attention over 8193 tokens, on the split-operand fp32-accurate kernels; --fp8 adds the opt-in e4m3 variants
    (tests/test_gpu_parity.py::test_stress_shape_k8192_d1536_single_level_vs_oracle checks this shape on the accurate path)."""
    spg = args.slides_per_gpu
    outputs = {} if args.dump_outputs and rank == 0 else None
    m = stress_measure(args.trans_dim, args.trans_heads, args.fp8, args.steps, args.warmup, spg, rank, world, dev, dev_reduce, pdist, putils,
                       outputs)
    if outputs is not None:
        write_outputs(args.dump_outputs, outputs)
    if rank == 0:
        print(json.dumps({
            "metric": "stress_slides_per_sec_1level_K8192_D1536", "value": m["slides_per_s"],
            "unit": "slides/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": m["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (two fp16 planes per operand, fp32 accumulate) - the parity path; 'fp8_attention' (--fp8) is the opt-in "
                     "e4m3 attention variant of BASELINE configs[4], outside the 1e-4 logit bar",
            "data": "synthetic",
            "config": {"workload": f"single level, 8192 patches x 1536 features per slide, {spg} slides per GPU, full quadratic "
                                   f"attention over 8193 tokens (BASELINE.json configs[4] geometry), trans_dim {args.trans_dim} / "
                                   f"{args.trans_heads} heads", "global_batch": spg * world},
            "attn_ffn_flops_per_step": m["attn_ffn_flops_per_step"], "attention_us": m["attention_us"],
            "aggregator_us": m["aggregator_us"], "fp8_attention": m["fp8_attention"], "fp8_aggregator": m["fp8_aggregator"]}), flush=True)
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def train_dtype(planes: int) -> str:
    """What the training step multiplies in (paths_amd.ops.TRAIN_PLANES)."""
    fwd = "forward: f32 operands as 2 fp16 planes (22 bits), 3 MFMAs per product block, fp32 accumulate"
    if planes == 4:
        return ("mixed: " + fwd + "; gradient GEMMs (dX, dW): operands as 2 bf16 planes = 16 significant bits at fp32 range, 3 MFMAs per "
                "block, fp32 accumulate (PATHS_TRAIN_PLANES=4, the default); attention backward (the five products of dQ / dK / dV): "
                "the same two bf16 planes (paths_attention_bwd_x6_planes); master weights, gradients and AdamW state fp32")
    return ("f32: " + fwd + "; gradient GEMMs and attention backward: operands as 3 exact bf16 planes (hi + mid + lo = the fp32 value), 6 "
            "MFMAs per block, fp32 accumulate (PATHS_TRAIN_PLANES=3); master weights, gradients and AdamW state fp32")


def train_bench(args, cfg, model, slides, rank, world, dev, pdist, putils, _unused):
    """Secondary metric (BASELINE.json configs[3]): training slides/s = recursion forward + hand-written HIP backward +
    AdamW, one flat 39.5 MB gradient all-reduce per step over RCCL when world > 1."""
    import numpy as np
    model.train()
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides.slides], np.int64)
    batch = {"slide": slides, "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    from paths_amd.optim import HipAdamW
    opt = (torch.optim.AdamW if os.environ.get("PATHS_TORCH_ADAMW", "0") != "0" else HipAdamW)(model.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    gb = len(slides) * world
    ar = pdist.allreduce_gradients if world > 1 else None

    def sync():
        torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()

    import torch.distributed as tdist
    if ar is None and tdist.is_initialized():          # PATHS_FORCE_DIST=1: a one-rank group, so that the RCCL path runs and is timed
        ar = pdist.allreduce_gradients
    pdist.TIME_ALLREDUCE = ar is not None
    loss = None
    for i in range(args.warmup):
        loss = putils.train_step(model, opt, batch, cfg.num_levels, cfg.top_k_patches, global_batch=gb, allreduce=ar)
        torch.cuda.synchronize()
        log(f"train warm-up step {i}: local loss share {float(loss):.4f}")
    sync()
    t0 = time.perf_counter()
    ar_ev = []
    for _ in range(args.steps):
        loss = putils.train_step(model, opt, batch, cfg.num_levels, cfg.top_k_patches, global_batch=gb, allreduce=ar)
        if ar is not None and pdist.LAST_ALLREDUCE_EVENTS is not None:
            ar_ev.append(pdist.LAST_ALLREDUCE_EVENTS)
    torch.cuda.synchronize()
    own = time.perf_counter() - t0                 # this rank's own K steps (with a process group every step already ends in the all-reduce)
    sync()
    elapsed = pdist.max_over_ranks(time.perf_counter() - t0, dev)
    per_rank = pdist.gather_floats(own / args.steps * 1e3)
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, {"loss": loss.detach().float().reshape(1).cpu().numpy(),
                                          "parameters": torch.cat([p.detach().float().reshape(-1) for p in model.parameters()]).cpu().numpy()})
    if rank == 0:
        K = args.k
        print(json.dumps({
            "metric": "train_slides_per_sec_5level_K%d_D1024" % K, "value": round(gb * args.steps / elapsed, 2), "unit": "slides/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "per_rank_ms_per_step": [round(v, 3) for v in per_rank], "rank_imbalance_max_over_min": round(max(per_rank) / max(min(per_rank), 1e-9), 4),
            "cores_per_rank": args.cores_per_rank or None,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": train_dtype(__import__("paths_amd.ops", fromlist=["ops"]).TRAIN_PLANES),
            "data": "synthetic", "train_planes": __import__("paths_amd.ops", fromlist=["ops"]).TRAIN_PLANES,
            "config": {"workload": f"train step (reference train.py:59-68 semantics): 5-level recursion K={K}, forward + HIP backward + "
                                   f"AdamW, {len(slides)} slides per GPU, dropout {cfg.model_config.dropout}", "global_batch": gb,
                       "parallelism": f"dp{world}: one flat fp32 gradient all-reduce per step" if world > 1 else "single GPU"},
            "final_loss_share": float(loss), "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2**30, 2),
            "allreduce_ms": round(sum(a.elapsed_time(b) for a, b in ar_ev) / len(ar_ev), 3) if ar_ev else None}), flush=True)
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def td192_probe(slides, K, spg, rank, world, dev, dev_reduce, pdist, putils, steps: int):
    """The headline workload (same resident slides, 5 levels, K = 2048) with the aggregator at the reference's dataclass-default width
    (trans_dim 192 = 4 heads of 48, reference config.py:30; the shipped models/sample/config.json says 128): weight-stationary chain and
    token-0 tail instantiated at 192, attention on the head_dim-48 split-operand kernel; launch tape replay; whole-job slides/s."""
    cfg, model, _ = build_model(K, dev, None, trans_dim=192)
    tape = putils.TapedRecursion(model, slides, cfg.top_k_patches, cfg.num_levels).record()
    for _ in range(3):
        tape.replay()
    torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tape.replay()
    torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()
    el = pdist.max_over_ranks(time.perf_counter() - t0, dev_reduce)
    assert int(out["status"].item()) == 0
    tape.close()
    del tape, model
    torch.cuda.empty_cache()
    return {"slides_per_s": round(spg * world * steps / el, 2), "ms_per_step": round(el / steps * 1e3, 3), "steps": steps, "slides_per_gpu": spg,
            "trans_dim": 192, "trans_heads": 4,
            "workload": "the headline recursion (5 levels, K = 2048, same resident slides) at the reference's dataclass-default aggregator width "
                        "(config.py:30); parity at this width: tests/test_gpu_parity.py::test_recursion_trans_dim_192_at_k1024_vs_oracle, G12 / G13 fixtures"}


def k1024_probe(model, cfg, spg, rank, world, dev, dev_reduce, pdist, putils, steps: int):
    """BASELINE.json configs[1] ("5-level PATHS, K=1024 patches/level, d=1024, 1 x MI355X"): the headline's launch mode (recorded
    tape) on this rank's own resident K = 1024 slides; whole-job slides/s.  Measured at the headline's batch (``spg`` slides per step
    and GPU) AND at twice that: at K = 1024 eight slides put 128 workgroups on a 256-CU chip in the gate GEMMs (half a round) -
    sixteen fill it (the config names no batch size)."""
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    K1 = 1024
    keep = [K1 // 4] * (cfg.num_levels - 1)

    def run(nsl):
        batch = DeviceSlideBatch([DeviceSlide.synthetic(1234, 200000 + rank * nsl + i, BASE_SHAPES[K1], device=dev) for i in range(nsl)])
        tape = putils.TapedRecursion(model, batch, keep, cfg.num_levels).record()
        for _ in range(3):
            tape.replay()
        torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = tape.replay()
        torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()
        el = pdist.max_over_ranks(time.perf_counter() - t0, dev_reduce)
        assert int(out["status"].item()) == 0
        tape.close()
        del tape, batch
        torch.cuda.empty_cache()
        return {"slides_per_s": round(nsl * world * steps / el, 2), "ms_per_step": round(el / steps * 1e3, 3), "slides_per_gpu": nsl}

    small, big = run(spg), run(2 * spg)
    return dict(big, steps=steps, at_headline_batch=small,
                workload=f"5-level recursion, K=1024 patches/level (level-0 grid 32x32, top_k 256), D=1024, {2 * spg} resident slides per GPU "
                         f"per step (at_headline_batch: {spg}), launch tape replay (BASELINE.json configs[1]); parity at this size: "
                         "tests/test_gpu_parity.py::test_headline_recursion_vs_oracle[1024]")


def self_launch(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher (no RANK / WORLD_SIZE in the environment): the parent - BEFORE any
    torch.cuda call, it never touches the GPU - starts N fresh child processes of this script, one per device, with the
    torch.distributed.run environment contract (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT), lets rank 0
    write the ONE JSON line to the inherited stdout and returns non-zero if any child does.  Nothing is re-exec'ed."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if torch.cuda.device_count() < n and "PATHS_DIST_BACKEND" not in env:      # (device_count() does not initialise the GPU)
        # fewer devices than ranks: a rehearsal (ranks share devices), RCCL refuses two ranks of one communicator on one device
        env["PATHS_DIST_BACKEND"] = "gloo"
        log(f"self-launch: {torch.cuda.device_count()} device(s) for {n} ranks - rehearsal over gloo")
    argv = list(sys.argv[1:])
    if not any(a == "--cores-per-rank" or a.startswith("--cores-per-rank=") for a in argv) and hasattr(os, "sched_getaffinity"):
        # default: every child pinned to its own 1/N of this process's host cores (N ranks x unpinned torch / HIP runtime threads on
        # one host share is the remaining risk for a host-paced training step); --cores-per-rank overrides
        argv += ["--cores-per-rank", str(max(1, host_cpu_share_all() // n))]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)))
             for r in range(n)]
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is not None:
                    pending.discard(r)
                    if code != 0 and rc == 0:
                        rc = code if code > 0 else 1
                        log(f"self-launch: rank {r} exited with {code}; stopping the other ranks")
                        for q in pending:
                            procs[q].terminate()
            time.sleep(0.05)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
            pr.wait()
    return rc


def train_probe(cfg, model, slides, world, dev_reduce, pdist, putils, steps: int, warmup: int, planes=None):
    """Short training measurement for the DEFAULT bench line (BASELINE.json configs[3] shape on this rank's resident slides):
    forward + hand-written HIP backward + AdamW (+ the flat gradient all-reduce when a process group exists) on a COPY of the
    model; returns ms_per_step (max over ranks), slides/s of the whole job, peak memory and the all-reduce time per step."""
    import copy
    import numpy as np
    from paths_amd import ops as pops
    saved_planes = pops.TRAIN_PLANES
    if planes is not None:
        pops.TRAIN_PLANES = int(planes)
    m = copy.deepcopy(model).train()
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides.slides], np.int64)
    batch = {"slide": slides, "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    from paths_amd.optim import HipAdamW
    opt = (torch.optim.AdamW if os.environ.get("PATHS_TORCH_ADAMW", "0") != "0" else HipAdamW)(m.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    gb = len(slides) * world
    grouped = torch.distributed.is_available() and torch.distributed.is_initialized()
    ar = pdist.allreduce_gradients if grouped else None
    pdist.TIME_ALLREDUCE = grouped
    torch.cuda.reset_peak_memory_stats()
    for _ in range(warmup):
        putils.train_step(m, opt, batch, cfg.num_levels, cfg.top_k_patches, global_batch=gb, allreduce=ar)
    torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ar_ms = []
    for _ in range(steps):
        putils.train_step(m, opt, batch, cfg.num_levels, cfg.top_k_patches, global_batch=gb, allreduce=ar)
        if grouped and pdist.LAST_ALLREDUCE_EVENTS is not None:
            ar_ms.append(pdist.LAST_ALLREDUCE_EVENTS)
    torch.cuda.synchronize(); pdist.barrier(); torch.cuda.synchronize()
    el = pdist.max_over_ranks(time.perf_counter() - t0, dev_reduce)
    pdist.TIME_ALLREDUCE = False
    out = {"steps": steps, "warmup": warmup, "ms_per_step": round(el / steps * 1e3, 3), "slides_per_s": round(gb * steps / el, 2),
           "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2**30, 2), "dropout": cfg.model_config.dropout,
           "allreduce_ms": round(sum(a.elapsed_time(b) for a, b in ar_ms) / len(ar_ms), 3) if ar_ms else None,
           "allreduce": (f"one flat fp32 bucket per step over {torch.distributed.get_backend()} (world {world})" if grouped else
                         "none (single rank without a process group)"),
           "train_planes": pops.TRAIN_PLANES, "dtype": train_dtype(pops.TRAIN_PLANES), "optimizer": type(opt).__name__ + (
               " (torch.optim.AdamW's foreach update in one HIP launch, bit-identical: paths_amd/optim.py)" if type(opt).__name__ == "HipAdamW" else ""),
           "workload": "train step (reference train.py:59-68): 5-level recursion forward + HIP backward + AdamW on the same resident slides"}
    pops.TRAIN_PLANES = saved_planes
    del m, opt
    torch.cuda.empty_cache()
    return out


def close_process_group():
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slides-per-gpu", type=int, default=8)
    ap.add_argument("--k", type=int, default=2048, choices=sorted(BASE_SHAPES))
    ap.add_argument("--full", action="store_true", help="infer mode: after the timed steps, also measure and check everything "
                    "beyond the headline (the options below marked --full) and add it to the line; off: the line carries the timed steps only")
    ap.add_argument("--cpu-slides", type=int, default=8, help="--full: slides of the cpu_baseline / parity_checked sample (a full batch at "
                    "K=2048; capped at the number of screened ids of the K)")
    ap.add_argument("--cpu-reps", type=int, default=2, help="--full: timed repetitions of the cpu_baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip cpu_baseline / parity_checked")
    ap.add_argument("--eager", action="store_true", help="timed region issues every launch through the Python launch path instead of "
                    "replaying the recorded launch tape (paths_amd.utils.TapedRecursion)")
    ap.add_argument("--graph", action="store_true", help="timed region replays the captured HIP graph of the recursion "
                    "(paths_amd.utils.GraphedRecursion) instead of issuing every launch from Python.  Measured on ROCm 7.2: the host "
                    "share drops from 0.65 to 0.13 of the step but the replay executes the three captured streams with far less "
                    "overlap (3.92 ms per step against 2.43 ms eager), so eager launches stay the default")
    ap.add_argument("--sustain", type=float, default=6.0, help="--full: seconds of the extra DVFS-steady loop (0 = skip); >= 6 s so that a 5-s "
                    "utilisation sampler beside the run lands inside GPU work")
    ap.add_argument("--breakdown-steps", type=int, default=3, help="--full: steps of the serialised per-kernel breakdown pass (0 = skip)")
    ap.add_argument("--dropout", type=float, default=None, help="train mode: dropout probability (default: the shipped config's 0.05)")
    ap.add_argument("--trans-dim", type=int, default=128, help="stress mode: aggregator width (BASELINE configs[4] reports 128 and 1536; "
                    "1536 with --trans-heads 24 = head_dim 64 runs on the flash-style kernels, with the reference's own 4 heads = head_dim "
                    "384 on the three-step wide-head form of csrc/attn_wide.hip: correct, untuned)")
    ap.add_argument("--trans-heads", type=int, default=4)
    ap.add_argument("--fp8", action="store_true", help="stress mode: also run the opt-in e4m3 variants (attention only; the whole aggregator) and report speed and "
                    "its logit distance from the fp32-accurate path")
    ap.add_argument("--rotate", type=int, default=3, help="infer mode: distinct resident slide batches (21 GiB each at K=2048) cycled "
                    "through the timed region, one recorded launch tape each; the headline is measured on the rotation (every step works "
                    "on different rows than the step before); --full reports the single-batch replay figure beside it")
    ap.add_argument("--train-steps", type=int, default=10, help="--full: timed steps of the short training measurement added to the "
                    "line as 'train' (0 = skip); 3 warm-up steps")
    ap.add_argument("--stress-steps", type=int, default=4, help="--full, N=1: timed steps of the 'stress' object (BASELINE configs[4]: one level, "
                    "K = 8192 x d = 1536, fp32-accurate path and the opt-in e4m3 variants at trans_dim 128 / 4 heads, 1536 / 24 heads and 1536 / 4 heads); 0 = skip")
    ap.add_argument("--k1024-steps", type=int, default=20, help="--full: timed steps of the 'k1024' object (BASELINE configs[1]: the same "
                    "5-level recursion at K = 1024 patches per level on one GPU's 8 resident slides); 0 = skip")
    ap.add_argument("--td192-steps", type=int, default=20, help="--full: timed steps of the 'trans_dim_192' object (the headline workload at the "
                    "reference's dataclass-default aggregator width, config.py:30); 0 = skip")
    ap.add_argument("--cores-per-rank", type=int, default=0, help="pin this rank to N host cores (cores [rank N, rank N + N) of the "
                    "process's allowed set) BEFORE anything touches the GPU: what a rank gets when 8 ranks share one host's CPU share "
                    "(0 = leave the affinity alone)")
    ap.add_argument("--mode", default="infer", choices=["infer", "train", "stress"],
                    help="infer (default, the BASELINE metric); train: forward + HIP backward + AdamW + gradient all-reduce; "
                         "stress: one level over 8192 patches x 1536 features (BASELINE configs[4] geometry, fp32-accurate path)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0's) as DIR/<name>.npy, float32 / "
                         "float64, at most 64 MB in all: infer / stress the recursion's outputs (ctx_patch as a seeded row sample), train "
                         "the loss and every parameter after the step.  Inputs and weights are seeded: the same arguments give the same "
                         "inputs in every run")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    from paths_amd import distributed as pdist
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))           # parent of a self-launched job: never touches the GPU
    rank, world, local_rank = pdist.env_rank_world()
    if args.cores_per_rank > 0 and hasattr(os, "sched_setaffinity"):
        allowed = sorted(os.sched_getaffinity(0))
        n = args.cores_per_rank
        mine = allowed[(local_rank * n) % len(allowed):][:n] or allowed[:n]
        os.sched_setaffinity(0, mine)              # (threads created later - HIP runtime, torch - inherit it)
        torch.set_num_threads(max(1, len(mine)))
        print(f"[bench rank {rank}/{world}] pinned to host cores {mine}", file=sys.stderr, flush=True)
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch N ranks with torch.distributed.run (or run "
                 f"'python bench.py --gpus N' without RANK / WORLD_SIZE in the environment and it starts them itself)")
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    ndev = torch.cuda.device_count()
    local_dev = local_rank % max(1, ndev)        # (rehearsals on a 1-GPU box put every rank on device 0)
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    backend = os.environ.get("PATHS_DIST_BACKEND", "nccl")     # "nccl" = RCCL; "gloo" only for 1-GPU rehearsals
    pdist.init(backend, dev)                     # no-op for a single rank
    if backend != "nccl":
        dev_reduce = torch.device("cpu")
    else:
        dev_reduce = dev

    from paths_amd import _lib, ops
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    _lib.load()
    if args.mode == "stress":
        stress_bench(args, rank, world, dev, dev_reduce, pdist, putils)
        return
    K, spg = args.k, args.slides_per_gpu
    cfg, model, sd = build_model(K, dev, args.dropout)
    slides = DeviceSlideBatch([DeviceSlide.synthetic(1234, rank * spg + i, BASE_SHAPES[K], device=dev) for i in range(spg)])
    torch.cuda.synchronize()
    log(f"model + {spg} slides resident ({torch.cuda.memory_allocated() / 2**30:.1f} GiB)")
    print(f"[bench rank {rank}/{world}] slide ids {[rank * spg + i for i in range(spg)]}", file=sys.stderr, flush=True)

    def barrier():
        torch.cuda.synchronize()
        pdist.barrier()
        torch.cuda.synchronize()

    if args.mode == "train":
        train_bench(args, cfg, model, slides, rank, world, dev_reduce, pdist, putils, None)
        return

    # --rotate distinct resident batches (slide ids disjoint across batches and ranks)
    nrot = max(1, args.rotate)
    batches = [slides]
    for r in range(1, nrot):
        batches.append(DeviceSlideBatch([DeviceSlide.synthetic(1234, 100000 * r + rank * spg + i, BASE_SHAPES[K], device=dev) for i in range(spg)]))
    if nrot > 1:
        torch.cuda.synchronize()
        log(f"{nrot} distinct batches resident ({torch.cuda.memory_allocated() / 2**30:.1f} GiB)")

    def step(trace=None, batch=None):
        with torch.no_grad():
            return putils.recurse(model, slides if batch is None else batch, cfg.top_k_patches, cfg.num_levels, trace=trace, check_status=False)

    # --graph: the whole recursion (5 levels, 3 streams, ~70 launches) captured once into a HIP graph and replayed per step
    # (paths_amd.utils.GraphedRecursion); default: the eager launch sequence (faster on this stack, see --graph's help)
    # default: the recursion recorded once as a flat launch tape and replayed (same three streams and joins as the eager pass,
    # Python's per-launch work gone: paths_amd.utils.TapedRecursion); --eager: every launch through the Python launch path
    graphed, launch_mode, replays = None, "eager", None
    if args.graph:
        replays = [putils.GraphedRecursion(model, b, cfg.top_k_patches, cfg.num_levels).capture() for b in batches]
        graphed, launch_mode = replays[0], "hip_graph_replay"
        log("recursion captured into a HIP graph")
    elif not args.eager:
        replays = [putils.TapedRecursion(model, b, cfg.top_k_patches, cfg.num_levels).record() for b in batches]
        graphed, launch_mode = replays[0], "launch_tape_replay"
        log(f"recursion recorded as a launch tape ({len(graphed.tape)} C calls per step, one tape per resident batch)")

    def timed_step(i=0):
        return replays[i % nrot].replay() if replays is not None else step(batch=batches[i % nrot])

    for i in range(max(args.warmup, nrot)):
        timed_step(i)
        torch.cuda.synchronize()
        log(f"warm-up step {i} done")
    # ---- timed region; the dominant kernel and the aggregator span are bracketed by events on their launch streams
    events = []

    def timer(name, launch, meta):
        # An event recorded right behind a kernel launch is attached to THAT kernel and reads its start time (measured: a start
        # event behind the memory-cell GEMM made the output-gate figure the sum of both, 187 us).  A throw-away record in front
        # takes that attachment; the real start event then gets a marker of its own, stamped when everything before it has ended.
        torch.cuda.Event(enable_timing=True).record()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out_ = launch()
        e1.record()
        events.append((name, e0, e1, meta))
        return out_

    if graphed is None:
        ops.KERNEL_TIMER, ops.TIMER_ALL = timer, False
    barrier()
    t0 = time.perf_counter()
    out = None
    for i in range(args.steps):
        out = timed_step(i)
    t_enqueued = time.perf_counter() - t0          # host side done (diagnostic: is the Python launch path ahead of the GPU?)
    torch.cuda.synchronize()
    own_elapsed = time.perf_counter() - t0         # this rank's own K steps, before it waits for the others
    barrier()
    elapsed = time.perf_counter() - t0
    ops.KERNEL_TIMER = None
    log(f"timed region: {args.steps} steps in {elapsed:.4f} s (all launches enqueued after {t_enqueued:.4f} s)")
    status = int(out["status"].item())
    assert status == 0, f"recursion status {status}"
    if args.dump_outputs and rank == 0:
        # (now: every replay after this overwrites the tape's output buffers)
        write_outputs(args.dump_outputs, recursion_outputs(out))
    per_rank = pdist.gather_floats(own_elapsed / args.steps * 1e3)  # every rank's own ms per step (load imbalance: slides differ)
    elapsed = pdist.max_over_ranks(elapsed, dev_reduce)
    x6, planes = gemm_split(cfg, slides)
    line = {
        "metric": "slides_per_sec_5level_K%d_D1024" % K, "value": round(spg * world * args.steps / elapsed, 2), "unit": "slides/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
        "per_rank_ms_per_step": [round(v, 3) for v in per_rank], "rank_imbalance_max_over_min": round(max(per_rank) / max(min(per_rank), 1e-9), 4),
        "vs_baseline": None, "dtype": infer_dtype(x6, planes), "data": "synthetic",
        "config": {"workload": f"5-level PATHS recursion (forward, eval): K={K} patches/level (level-0 grid "
                               f"{BASE_SHAPES[K][0]}x{BASE_SHAPES[K][1]}, top_k {K // 4}, 10% background), D=1024 "
                               f"features, trans_dim 128 x 4 heads x 2 layers, LSTM ctx 256; {spg} HBM-resident slides per GPU",
                   "slides_per_gpu": spg, "global_batch": spg * world, "levels": cfg.num_levels,
                   "resident_batches_rotated": nrot,
                   "parallelism": f"slide-sharded x{world} (no data-path collective)",
                   "gemm_mode": infer_gemm_mode(x6, planes)},
        "host": {"launch_mode": launch_mode, "t_enqueued_over_elapsed": round(t_enqueued / max(elapsed, 1e-9), 3)},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(line), flush=True)
        close_process_group()
        return
    single = None
    if nrot > 1:
        # the same K steps on ONE batch (the round-2 headline): every step re-reads the rows the previous one touched
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            out = timed_step(0)
        barrier()
        el1 = pdist.max_over_ranks(time.perf_counter() - t1, dev_reduce)
        single = {"slides_per_s": round(spg * world * args.steps / el1, 2), "ms_per_step": round(el1 / args.steps * 1e3, 3),
                  "note": "same launch mode, one resident batch replayed (warm L2 / Infinity Cache for its rows)"}
    eager = None
    if graphed is not None:
        # kernel-level event timing needs launches issued one by one (events inside a captured graph cannot be timed): the same
        # K steps again, eagerly, right after the timed region, with the dominant kernel and the aggregator span bracketed
        for _ in range(2):
            step()
        ops.KERNEL_TIMER, ops.TIMER_ALL = timer, False
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        t_enq_e = time.perf_counter() - t1
        barrier()
        el_e = time.perf_counter() - t1
        ops.KERNEL_TIMER = None
        eager = {"ms_per_step": round(el_e / args.steps * 1e3, 3), "slides_per_s": round(spg * args.steps / el_e, 2),
                 "t_enqueued_over_elapsed": round(t_enq_e / max(el_e, 1e-9), 3)}
        log(f"eager instrumented pass: {args.steps} steps in {el_e:.4f} s (enqueued after {t_enq_e:.4f} s)")
    live = {}
    for name, e0, e1, meta in events:
        live.setdefault(name, []).append((e0.elapsed_time(e1), meta))
    events.clear()

    # ---- launch modes side by side on the SAME rotation of resident batches: replay = one recorded tape per
    # batch (the headline), rebind = ONE tape re-pointed at the next batch before every step (TapedRecursion.rebind: what a stream of
    # distinct slides pays), eager = every launch through the Python path, un-instrumented
    launch_modes = None
    if replays is not None and not args.graph and nrot > 1 and world == 1:
        lm_steps = max(args.steps, 150)               # (10 steps = 22 ms read +- 3 % from run to run: too short to compare modes)

        def timed_loop(fn):
            for i in range(nrot):
                fn(i)
            barrier()
            t1_ = time.perf_counter()
            for i in range(lm_steps):
                fn(i)
            barrier()
            return time.perf_counter() - t1_
        one = replays[0]
        el_rb = timed_loop(lambda i: one.rebind(batches[i % nrot]).replay())
        assert one.tape is not None and one._rec_batch is not None, "rebind dropped the tape on a same-shape batch"
        one.rebind(batches[0])
        el_rp = timed_loop(lambda i: replays[i % nrot].replay())
        el_eg = timed_loop(lambda i: step(batch=batches[i % nrot]))
        # consecutive steps on ALTERNATING stream triples, each tape without its final join (TapedRecursion(lane=k), replay(join=False)):
        # step i+1's selection chain starts while step i's last aggregator still runs - what a serving loop with two in-flight
        # batches does.  Measured beside the headline, which keeps one stream triple (each step complete before the next starts).
        pipe = putils.PipelinedRecursion(model, batches, cfg.top_k_patches, cfg.num_levels)
        el_2l = timed_loop(lambda i: pipe.submit(i % nrot))
        torch.cuda.synchronize()
        ref_out = replays[0].replay()
        two = pipe.result(0)
        assert torch.equal(two["logits"], ref_out["logits"]), "two-lane replay changed the results"
        pipe.close()
        del pipe
        torch.cuda.synchronize()
        launch_modes = {"steps": lm_steps, "batches_rotated": nrot,
                        "replay_slides_per_s": round(spg * lm_steps / el_rp, 2), "rebind_slides_per_s": round(spg * lm_steps / el_rb, 2),
                        "eager_slides_per_s": round(spg * lm_steps / el_eg, 2),
                        "replay_two_lanes_slides_per_s": round(spg * lm_steps / el_2l, 2),
                        "note": "replay: one tape per resident batch; rebind: ONE tape, table tensors re-pointed at the next batch before "
                                "every step (no re-recording); eager: Python launch path; replay_two_lanes: consecutive steps on alternating "
                                "stream triples without the per-step join (two batches in flight: step i+1's selection chain starts under step "
                                "i's last aggregator) - NOT the headline, which completes each step before the next starts"}
        log(f"launch modes: replay {launch_modes['replay_slides_per_s']}, rebind {launch_modes['rebind_slides_per_s']}, eager {launch_modes['eager_slides_per_s']}, "
            f"two lanes {launch_modes['replay_two_lanes_slides_per_s']} slides/s")

    # ---- sustained figure: the same step for >= --sustain seconds (DVFS-steady clocks; the 20-step region above lasts ~50 ms)
    sustained = None
    if args.sustain > 0:
        n_sus = max(args.steps, int(args.sustain / max(elapsed / args.steps, 1e-4)) + 1)
        barrier()
        t1 = time.perf_counter()
        for i in range(n_sus):
            out = timed_step(i)
        barrier()
        el2 = pdist.max_over_ranks(time.perf_counter() - t1, dev_reduce)
        sustained = {"steps": n_sus, "seconds": round(el2, 3), "slides_per_s": round(spg * world * n_sus / el2, 2),
                     "ms_per_step": round(el2 / n_sus * 1e3, 3)}
        log(f"sustained: {n_sus} steps in {el2:.3f} s")

    # ---- per-level valid rows / tokens of this rank's batch (the algorithmic work of one step)
    trace = []
    step(trace)
    torch.cuda.synchronize()
    nims = [lv["num_ims"].cpu().numpy().astype("float64") for lv in trace]
    valid = [float(n.sum()) for n in nims]
    d_t, L_t = cfg.model_config.trans_dim, cfg.model_config.trans_layers
    # F_layer = 24 T d^2 + 4 T^2 d per slide (QKV 6Td^2, out 2Td^2, FFN 16Td^2, QK^T + PV 4T^2 d), T = valid patches + 1
    f_agg = [float(sum(L_t * (24.0 * (n + 1) * d_t * d_t + 4.0 * (n + 1) ** 2 * d_t) for n in lv)) for lv in nims]
    # FUSE_QKV (default): decoder layer 0's in_proj runs inside the importance / projection finish on the selection stream, OUTSIDE the
    # timed aggregator span - its algorithmic FLOPs (6 T d^2 per slide) leave the span's numerator with it
    fused_qkv = ops.FUSE_QKV in (1, 2) and ops.fast_path(cfg.model_config) and ops.GEMM_MODE == "h3"
    f_inproj0 = [float(sum(6.0 * (n + 1) * d_t * d_t for n in lv)) for lv in nims]
    if fused_qkv:
        f_agg_full, f_agg = f_agg, [a - b for a, b in zip(f_agg, f_inproj0)]

    def gemm_o_roofline(samples):
        flop = sum(2.0 * valid[i % cfg.num_levels] * m["K"] * m["Ncols"] for i, (_, m) in enumerate(samples))
        ms = sum(t for t, _ in samples)
        return flop, ms, max(1, len(samples))

    # ---- serialised breakdown pass (one stream, every kernel group bracketed): what each kernel takes with the chip to itself
    breakdown = None
    rep_span = None
    ser_span = {}
    if args.breakdown_steps > 0:
        saved_overlap, putils.OVERLAP_AGGREGATOR = putils.OVERLAP_AGGREGATOR, False
        # pass A: only the dominant kernel and the aggregator span are bracketed (as in the live pass): inner event pairs would sit
        # INSIDE the span and lengthen it (~2 us per pair)
        ops.KERNEL_TIMER, ops.TIMER_ALL = timer, False
        for _ in range(args.breakdown_steps):
            step()
        torch.cuda.synchronize()
        for name, e0, e1, meta in events:
            ser_span.setdefault(name, []).append((e0.elapsed_time(e1), meta))
        events.clear()
        # pass B: every kernel group bracketed
        ops.KERNEL_TIMER, ops.TIMER_ALL = timer, True
        for _ in range(args.breakdown_steps):
            step()
        torch.cuda.synchronize()
        ops.KERNEL_TIMER, ops.TIMER_ALL = None, False
        # pass C: the same single-stream step REPLAYED from a recorded launch list (a C call every ~2 us instead of a Python launch
        # every 10-20 us), events only around each level's aggregator launches: the span with the chip to itself AND no host-paced
        # gaps between its four launches (pass A's in_proj kernel is shorter than the Python call that enqueues the attention)
        rep_span = None
        try:
            from paths_amd import _lib as plib
            with torch.no_grad():
                tser = putils.TapedRecursion(model, batches[0], cfg.top_k_patches, cfg.num_levels).record()
            tp = tser.tape
            # the span starts at the aggregator's first launch: the attention (FUSE_QKV: in_proj lives in the importance / projection
            # finish), or the in_proj launch in front of it (PATHS_FUSE_QKV=0)
            starts = [i - 1 if tp[i - 1][2] == "paths_token_layer_ws" else i for i in range(1, len(tp)) if tp[i][2] == "paths_attention_h3_img"]
            ends = []
            for i in starts:
                ends.append(next(j for j in range(i, len(tp)) if tp[j][2] == "paths_token0_tail_ws"))
            if len(starts) == cfg.num_levels and all(tp[k][2] != "paths_stream_wait" for k in range(len(tp))):
                sset, eset = set(starts), set(ends)
                evs = []
                for rep in range(2 + args.breakdown_steps):
                    for k, (fn, a, name) in enumerate(tp):
                        if k in sset and rep >= 2:
                            torch.cuda.Event(enable_timing=True).record()
                            e0 = torch.cuda.Event(enable_timing=True); e0.record()
                        if fn(*a) != 0:
                            raise RuntimeError(name)
                        if k in eset and rep >= 2:
                            e1 = torch.cuda.Event(enable_timing=True); e1.record()
                            evs.append((e0, e1))
                torch.cuda.synchronize()
                rep_span = [(a.elapsed_time(b), {}) for a, b in evs]
            tser.close()
        except Exception as e:                       # a diagnostic: never lose the headline to it
            log(f"replayed serialised span skipped: {type(e).__name__}: {e}")
        putils.OVERLAP_AGGREGATOR = saved_overlap
        ser = {}
        for name, e0, e1, meta in events:
            ser.setdefault(name, []).append((e0.elapsed_time(e1), meta))
        events.clear()
        breakdown = {"steps": args.breakdown_steps,
                     "note": "single stream, events around every kernel group (each figure includes the launch gaps either side and its "
                             "own event pair; 'aggregator' here contains the four inner pairs - roofline_attn_ffn.serialized_span_us is "
                             "the same span measured without them); us per launch, launches per step",
                     "us_per_launch": {k: round(sum(t for t, _ in v) * 1e3 / len(v), 2) for k, v in sorted(ser.items())},
                     "launches_per_step": {k: len(v) // args.breakdown_steps for k, v in sorted(ser.items())}}
        breakdown["us_per_step_sum"] = round(sum(breakdown["us_per_launch"][k] * breakdown["launches_per_step"][k]
                                                 for k in ser if k != "aggregator"), 1)
    else:
        ser = {}

    # ---- roofline of the dominant kernel: algorithmic FLOP = 2 * valid_rows * K * N per launch
    samples_o = live.get("lstm_gate_o", [])
    flop, ms, n_launch = gemm_o_roofline(samples_o)
    achieved = flop / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    meta0 = samples_o[0][1] if samples_o else {}
    x6 = bool(meta0.get("x6"))
    planes = int(meta0.get("planes", 3)) if x6 else 0
    if samples_o and (x6, planes) != gemm_split(cfg, slides):
        log(f"the instrumented output-gate launches ran x6={x6} planes={planes}; the line's dtype follows {gemm_split(cfg, slides)}")
    traffic = None            # HBM-side bytes per launch from the committed PMC passes (separate --pmc runs, profiles/)
    prof = {2: PMC_PROFILE_H3, 3: "r01e_pmc_traffic.json"}.get(planes, "r01_pmc_traffic.json")
    try:
        with open(os.path.join(ROOT, "profiles", prof)) as fh:
            kstat = json.load(fh)["kernels"]["EpiLstmO"]
        traffic = kstat["traffic_bytes_per_launch"]
    except (OSError, KeyError, ValueError):
        pass
    if x6:
        nprod = MFMA_PER_PRODUCT[planes]
        peak = PEAK_BF16_MFMA_TFLOPS / nprod
        what = ("2 fp16 planes (hi + lo), hi*hi + hi*lo + lo*hi = 3 x v_mfma_f32_32x32x16_f16" if planes == 2 else
                "3 bf16 planes (hi + mid + lo), 6 x v_mfma_f32_32x32x16_bf16")
        roofline = {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                    "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": f"profiles/{prof} (separate --pmc passes)",
                    "kernel": f"gemm_x6_kernel<{planes},4,4,1,EpiLstmO> (LSTM output-gate GEMM, fp32 operands split into {what} "
                              "per product block, fp32 accumulate)",
                    "peak_basis": f"dense 16-bit MFMA peak 2500 TFLOP/s / {nprod} MFMAs per fp32 product block; achieved counts "
                                  "ALGORITHMIC flops 2MNK, so frac == 16-bit MFMA flops issued / 2500",
                    "mfma_issue_tflops": round(achieved * nprod, 1),
                    "vs_f32_matrix_peak": round(achieved / PEAK_F32_MFMA_TFLOPS, 3),
                    "avg_launch_us": round(ms * 1e3 / n_launch, 2), "launches": n_launch,
                    "algorithmic_gflop_per_launch": round(flop / n_launch / 1e9, 3)}
        mp = measured_peaks()
        if mp is not None and planes == 2:
            pm = mp["derived"]["h3_fp32_equivalent_tflops"]
            roofline["peak_measured"] = pm
            roofline["frac_of_measured_peak"] = round(achieved / pm, 4)
            roofline["peak_measured_basis"] = ("profiles/roofline.json: back-to-back v_mfma_f32_32x32x16_f16 issue on random operands, all "
                                               f"CUs = {mp['derived']['mfma_f16_issue_tflops']} TFLOP/s (tools/peaks.hip) / 3")
        if ser_span.get("lstm_gate_o"):
            f2, ms2, n2 = gemm_o_roofline(ser_span["lstm_gate_o"])
            src = "pass A (only this kernel and the aggregator span bracketed)"
            # Cross-check against pass B (every kernel group bracketed: the same launches, each figure ~2 us longer).  An event pair can
            # attach to an EARLIER kernel's completion (seen once in round 4: 355 us = the whole selection chain, against 97 in pass B
            # and 102-111 in every other run); a pass-A figure more than 1.25 x pass B's is that artefact, not the kernel.
            if ser.get("lstm_gate_o"):
                fb, msb, nb = gemm_o_roofline(ser["lstm_gate_o"])
                if ms2 / n2 > 1.25 * msb / nb:
                    f2, ms2, n2, src = fb, msb, nb, "pass B (every kernel group bracketed; pass A's event pair spanned earlier kernels)"
            roofline["serialized_us"] = round(ms2 * 1e3 / n2, 2)          # measured in this run (breakdown pass), not from a file
            roofline["serialized_frac"] = round(f2 / (ms2 * 1e-3) / 1e12 / peak, 4)
            roofline["serialized_source"] = src
    else:
        peak = PEAK_F32_MFMA_TFLOPS
        roofline = {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_F32_MFMA_TFLOPS, 4), "traffic": traffic,
                    "kernel": "gemm_f32_kernel<2,2,2,2,EpiLstmO> (LSTM output-gate GEMM, v_mfma_f32_32x32x2_f32)",
                    "avg_launch_us": round(ms * 1e3 / n_launch, 2), "launches": n_launch,
                    "algorithmic_gflop_per_launch": round(flop / n_launch / 1e9, 3)}

    # ---- what an event pair costs by itself on this box: the bracket of the timer above around NOTHING, and around one trivial launch.
    # A bracketed span contains the completion-side latency of its two event packets and the dispatch latency of its first kernel;
    # rocprofv3's kernel trace of the same three launches back to back reads ~12 us less than the bracket (profiles/r05u_agg_gaps.txt).
    ev_overhead = None
    try:
        tiny = torch.zeros((64,), device=dev)
        pairs = {"empty": [], "one_launch": []}
        for kind in ("empty", "one_launch"):
            for _ in range(30):
                torch.cuda.synchronize()
                torch.cuda.Event(enable_timing=True).record()
                a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a_.record()
                if kind == "one_launch":
                    _lib.call("paths_memset_zero", tiny.data_ptr(), 256, _lib.stream())
                b_.record()
                torch.cuda.synchronize()
                pairs[kind].append(a_.elapsed_time(b_) * 1e3)
        med = lambda v: sorted(v)[len(v) // 2]
        ev_overhead = {"empty_pair_us": round(med(pairs["empty"]), 2), "pair_around_one_trivial_launch_us": round(med(pairs["one_launch"]), 2)}
    except Exception as e:                               # a diagnostic only
        log(f"event overhead calibration skipped: {type(e).__name__}: {e}")

    # ---- roofline of the attention + FFN kernels (north_star target: >= 0.50): the aggregator span of every level (in_proj,
    # attention, token-layer chain, token-0 tail) event-timed on ITS stream inside the timed region; algorithmic FLOPs = L * F_layer
    def agg_roofline(samples):
        fl = sum(f_agg[i % cfg.num_levels] for i in range(len(samples)))
        ms_ = sum(t for t, _ in samples)
        return fl, ms_, max(1, len(samples))

    roofline_attn = None
    if live.get("aggregator"):
        fl, ms_a, n_a = agg_roofline(live["aggregator"])
        ach = fl / (ms_a * 1e-3) / 1e12 if ms_a > 0 else 0.0
        roofline_attn = {"bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                         "kernels": ("attention + token-layer chain (out_proj, LN x3, FFN) + token-0 tail (last layer, one launch), per level; the "
                                     "first layer's in_proj runs inside the importance / projection finish (paths_importance_qkv_x6) and is "
                                     "counted neither in the span nor in its FLOPs") if fused_qkv else
                                    "token-layer in_proj + attention + token-layer chain (out_proj, LN x3, FFN) + token-0 tail (last layer, one "
                                    "launch), per level",
                         "in_proj_fused_into_finish": bool(fused_qkv),
                         "fuse_qkv_mode": ops.FUSE_QKV if fused_qkv else 0,
                         "fuse_qkv_note": (None if not fused_qkv else
                                           "mode 1: ONE finish of the importance / projection GEMM on the selection stream writes importance, tokens and "
                                           "layer 0's q | k | v operand images; mode 2 (default): an importance-only finish on the selection stream "
                                           "(the top-K waits for nothing else), tokens + images by a second finish at the head of the aggregator "
                                           "stream (serialized_breakdown: agg_tokens_qkv) - the successor of the round-4 finish kernel, which was "
                                           "never part of this span either"),
                         "algorithmic_gflop_in_proj0_excluded": round(sum(f_inproj0) / len(f_inproj0) / 1e9, 3) if fused_qkv else 0.0,
                         "algorithmic_gflop_per_level_launch": round(fl / n_a / 1e9, 3), "avg_span_us": round(ms_a * 1e3 / n_a, 2),
                         "spans": n_a,
                         "flops_basis": "SURVEY 8(d): L * (24 T d^2 + 4 T^2 d) per slide, T = valid patches + 1, all L layers counted in "
                                        "full; the build computes the LAST layer at token 0 only (its other rows are never read, "
                                        "reference model/aggregator.py:75), so executed FLOPs are ~0.52 of the algorithmic count",
                         "timing": "live: the span shares the chip with the selection chain of the next level (second stream)",
                         "event_bracket_overhead": ev_overhead}
        if ser_span.get("aggregator"):
            fl2, ms2, n2 = agg_roofline(ser_span["aggregator"])
            roofline_attn["serialized_span_us"] = round(ms2 * 1e3 / n2, 2)
            roofline_attn["serialized_frac"] = round(fl2 / (ms2 * 1e-3) / 1e12 / peak, 4)
            # the same by level of the recursion (sample i of the pass = level i % num_levels): level 0 of the synthetic slides has no
            # background cells - 2,048 patches + the special token = 2,049 tokens = 8 x 256 queries + 1, 32 x 64 token rows + 1: the
            # stray query block / token tile of a completely full slide is a second round of workgroups
            Lv = cfg.num_levels
            sp = ser_span["aggregator"]
            by = [[t for i, (t, _) in enumerate(sp) if i % Lv == l] for l in range(Lv)]
            roofline_attn["serialized_span_by_level_us"] = [round(sum(v) * 1e3 / len(v), 2) if v else None for v in by]
            roofline_attn["serialized_frac_by_level"] = [round(f_agg[l] / (sum(v) / len(v) * 1e-3) / 1e12 / peak, 4) if v else None for l, v in enumerate(by)]
            roofline_attn["valid_patches_by_level"] = [int(v) for v in valid]
            if ev_overhead is not None:
                # the same span net of the bracket's own cost (the pair around one trivial launch): what the three kernels take back to
                # back - REPORTED BESIDE serialized_frac, never instead of it
                net = ms2 * 1e3 / n2 - ev_overhead["pair_around_one_trivial_launch_us"]
                if net > 0:
                    roofline_attn["serialized_span_net_of_bracket_us"] = round(net, 2)
                    roofline_attn["serialized_frac_net_of_bracket"] = round(fl2 / n2 / (net * 1e-6) / 1e12 / peak, 4)
            if rep_span:
                fl3, ms3, n3 = agg_roofline(rep_span)
                roofline_attn["serialized_span_replayed_us"] = round(ms3 * 1e3 / n3, 2)
                roofline_attn["serialized_frac_replayed"] = round(fl3 / (ms3 * 1e-3) / 1e12 / peak, 4)
                roofline_attn["serialized_note"] = ("serialized_span_us: single stream, the four launches issued through the Python launch path "
                                                    "(host-paced gaps between them); serialized_span_replayed_us: the same launches replayed "
                                                    "from a recorded launch list, events around them only - the GPU-side span")
            mp = measured_peaks()
            if mp is not None and planes == 2:
                pm = mp["derived"]["h3_16x16x32_fp32_equivalent_tflops"]
                roofline_attn["peak_measured"] = pm
                roofline_attn["serialized_frac_of_measured_peak"] = round(fl2 / (ms2 * 1e-3) / 1e12 / pm, 4)
                roofline_attn["frac_of_measured_peak"] = round(ach / pm, 4)

    train = None
    if args.train_steps > 0:
        try:
            train = train_probe(cfg, model, slides, world, dev_reduce, pdist, putils, args.train_steps, 5)
            log(f"train probe: {train['ms_per_step']} ms per step, all-reduce {train['allreduce_ms']} ms")
            # the same step with the OTHER gradient-operand setting (the fp32-accurate three-plane split unless that is the default)
            other = 3 if train["train_planes"] == 4 else 4
            t2 = train_probe(cfg, model, slides, world, dev_reduce, pdist, putils, args.train_steps, 3, planes=other)
            train[f"planes{other}"] = {k: t2[k] for k in ("ms_per_step", "slides_per_s", "train_planes", "dtype")}
            log(f"train probe (PATHS_TRAIN_PLANES={other}): {t2['ms_per_step']} ms per step")
        except Exception as e:       # the headline (already measured above) must not be lost to a failure of the secondary probe
            train = {"error": f"{type(e).__name__}: {e}"[:400]}
            log(f"train probe FAILED: {train['error']}")
    # ---- BASELINE.json configs[1]: the same recursion at K = 1024 patches per level (same weights, top_k 256, level-0 grid 32 x 32)
    k1024 = None
    if K == 2048 and args.k1024_steps > 0:
        try:
            k1024 = k1024_probe(model, cfg, spg, rank, world, dev, dev_reduce, pdist, putils, args.k1024_steps)
            log(f"k1024: {k1024['slides_per_s']} slides/s at {k1024['slides_per_gpu']} slides per step, {k1024['at_headline_batch']['slides_per_s']} at {spg}")
        except Exception as e:
            k1024 = {"error": f"{type(e).__name__}: {e}"[:400]}
            log(f"k1024 probe FAILED: {k1024['error']}")
    # ---- the reference's dataclass-default aggregator width on the headline workload (second-class speed is visible in the record)
    td192 = None
    if K == 2048 and args.td192_steps > 0:
        try:
            td192 = td192_probe(slides, K, spg, rank, world, dev, dev_reduce, pdist, putils, args.td192_steps)
            log(f"trans_dim 192: {td192['slides_per_s']} slides/s")
        except Exception as e:
            td192 = {"error": f"{type(e).__name__}: {e}"[:400]}
            log(f"trans_dim 192 probe FAILED: {td192['error']}")
    # ---- BASELINE.json configs[4]: the stress geometry, accurate path + the opt-in e4m3 variants, so the driver's record carries it
    stress = None
    replayed_launches = graphed is not None
    if world == 1 and args.stress_steps > 0:
        try:
            replays = graphed = batches = None          # (free the K = 2048 tapes and rotated batches: 43 GiB back to the allocator)
            torch.cuda.empty_cache()
            stress = {"workload": "one level over 8192 patches x 1536 features per slide (full quadratic attention over 8193 tokens), "
                                  f"{spg} slides per step (BASELINE.json configs[4])",
                      "td128_h4": stress_measure(128, 4, True, args.stress_steps, 2, spg, rank, world, dev, dev_reduce, pdist, putils),
                      "td1536_h24": stress_measure(1536, 24, True, args.stress_steps, 2, spg, rank, world, dev, dev_reduce, pdist, putils),
                      # SURVEY 8(d) writes the wide stress row as 1536 / 4 heads = head_dim 384: accurate path on csrc/attn_wide.hip,
                      # e4m3 attention on the wide instantiation of csrc/attn_fp8.hip (round 5)
                      "td1536_h4": stress_measure(1536, 4, True, max(2, args.stress_steps // 2), 1, spg, rank, world, dev, dev_reduce, pdist, putils)}
            for k_ in ("td128_h4", "td1536_h24", "td1536_h4"):
                f8 = stress[k_].get("fp8_aggregator") or {}
                log(f"stress {k_}: accurate {stress[k_]['ms_per_step']} ms per step, e4m3 aggregator {f8.get('ms_per_step')} ms "
                    f"(frac of fp8 peak {(f8.get('roofline') or {}).get('frac')}, logit diff {f8.get('max_logit_diff_vs_accurate_path')})")
        except Exception as e:
            stress = {"error": f"{type(e).__name__}: {e}"[:400]}
            log(f"stress probe FAILED: {stress['error']}")
    per_rank_valid = pdist.gather_floats(float(sum(valid)))      # valid patches per step of every rank (what its step time follows)
    if rank == 0:
        line["per_rank_valid_patches_per_step"] = [int(v) for v in per_rank_valid]
        line["roofline"] = dict(roofline, attn_ffn=None if roofline_attn is None else {
            k: roofline_attn.get(k) for k in ("achieved", "peak", "unit", "frac", "avg_span_us", "serialized_span_us", "serialized_frac",
                                               "serialized_span_replayed_us", "serialized_frac_replayed", "serialized_note",
                                               "serialized_frac_of_measured_peak", "algorithmic_gflop_per_level_launch",
                                               "in_proj_fused_into_finish", "algorithmic_gflop_in_proj0_excluded", "fuse_qkv_mode",
                                               "event_bracket_overhead", "serialized_frac_net_of_bracket", "serialized_span_by_level_us",
                                               "serialized_frac_by_level", "valid_patches_by_level")})
        line["roofline_attn_ffn"] = roofline_attn
        line["host"].update(eager_instrumented_pass=eager, launch_modes=launch_modes,
                            note="roofline / roofline_attn_ffn event timings come from the eager instrumented pass of the same K steps "
                                 "(the replayed launch sequence carries no events)" if replayed_launches else None)
        if single is not None:
            line["single_batch"] = single
        if train is not None:
            line["train"] = train
        if sustained is not None:
            line["sustained"] = sustained
        if k1024 is not None:
            line["k1024"] = k1024
        if td192 is not None:
            line["trans_dim_192"] = td192
        if stress is not None:
            line["stress"] = stress
        if breakdown is not None:
            line["serialized_breakdown"] = breakdown
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"], ids, otrace, ohz = cpu_baseline(cfg, sd, K, args.cpu_slides, args.cpu_reps)
            line["parity_checked"] = parity_check(cfg, model, K, ids, otrace, ohz, dev)
        print(json.dumps(line), flush=True)
    close_process_group()


if __name__ == "__main__":
    main()
