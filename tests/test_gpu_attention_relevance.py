"""The special token's gradient-weighted attention relevance on the GPU (csrc/attn_relevance.hip, paths_amd/saliency.py:
attention_relevance): seed and step on identical fp32 operands against the float64 restatement (tests/relevance_ref.py),
the whole pass against float64 autograd over the oracle's own token sequences, its properties, and that nothing else moves."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import relevance_ref as R
from tests.test_gpu_attention_rollout import SMALL, build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16 = torch.float16
KERNEL_TOL = 1e-5            # |r_out - ref| <= KERNEL_TOL |ref - r_in| per slide: 6-10 x what plain fp32 torch reaches on the same formula
E2E_TOL = 2e-3               # the project's norm-wise recursion-gradient bar (tests/test_gpu_saliency.py), against the |.| envelope
RELEVANCE_CALLS = ("paths_attention_relevance_seed", "paths_attention_relevance_step")


# ------------------------------------------------------------------------------------------------
# 1. the kernels on identical fp32 operands
# ------------------------------------------------------------------------------------------------
def _operands(T, nh, hd, B=3):
    """q, k ~ N(0, 1.5^2) (scores qscale q . k in the log2 domain, qscale = log2(e) / sqrt(hd)); dO, v ~ N(0, 1), so the increment is of
    the order of r_in.  Head-major [B, H, T, hd] fp32; num_ims ragged with a 0."""
    gen = torch.Generator().manual_seed(T * 1009 + nh * 101 + hd)
    q, k = (torch.randn((B, nh, T, hd), generator=gen) * 1.5 for _ in range(2))
    v = torch.randn((B, nh, T, hd), generator=gen)
    d_o = torch.randn((B, T, nh * hd), generator=gen)
    r_in = torch.rand((B, T), generator=gen)
    num_ims = torch.tensor([T - 1, 0, (T - 1) // 2][:B], dtype=torch.int64)
    return q, k, v, d_o, r_in, num_ims, math.log2(math.e) / math.sqrt(hd)


def _nan_padding(num_ims, *tensors_and_dims):
    """Clones with NaN on every row past num_ims[b] along the given token dimension."""
    out = []
    for t, dim in tensors_and_dims:
        t = t.clone()
        for b in range(t.shape[0]):
            idx = [b] + [slice(None)] * (t.dim() - 1)
            idx[dim] = slice(int(num_ims[b]) + 1, None)
            t[tuple(idx)] = float("nan")
        out.append(t)
    return out


def _layouts(dev, q, k, v, d_o, qscale):
    """The two operand forms on the device: head-major with pre-scaled q (qscale 1) and token-major qkv [B, T, 3 di] views with the
    unscaled q; d_o with a row wider than H * hd in the second.  Each with the fp32 operands the float64 reference must read."""
    B, nh, T, hd = q.shape
    qs = q * np.float32(qscale)
    yield "head-major", (qs.to(dev), k.to(dev), v.to(dev)), 1.0, d_o.to(dev), (qs, k, v)
    di = nh * hd
    qkv = torch.cat([t.permute(0, 2, 1, 3).reshape(B, T, di) for t in (q, k, v)], dim=-1).contiguous().to(dev)
    views = tuple(qkv[:, :, i * di:(i + 1) * di].view(B, T, nh, hd).permute(0, 2, 1, 3) for i in range(3))
    wide = torch.full((B, T, di + 8), float("nan"))
    wide[:, :, :di] = d_o
    yield "token-major", views, qscale, wide.to(dev), (q, k, v)


def _slide_errors(got, want, base, num_ims):
    """Per slide (|got - want|_2, |want - base|_2) over the valid rows."""
    out = []
    for b in range(got.shape[0]):
        n1 = int(num_ims[b]) + 1
        out.append((float((got[b, :n1].double() - want[b, :n1]).norm()), float((want[b, :n1] - base[b, :n1].double()).norm())))
    return out


@pytest.mark.parametrize("nh,hd", [(4, 32), (1, 16), (3, 48), (2, 64)])
@pytest.mark.parametrize("T", [1, 2, 16, 17, 64, 65, 130])
def test_kernels_vs_float64(dev, T, nh, hd):
    from paths_amd.saliency import relevance_seed, relevance_step
    q, k, v, d_o, r_in, num_ims, qscale = _operands(T, nh, hd)
    B = q.shape[0]
    q, k, v, d_o, r_in = _nan_padding(num_ims, (q, 2), (k, 2), (v, 2), (d_o, 1), (r_in, 1))    # NaN in every padding row
    nd = num_ims.to(dev)
    e_s = torch.zeros((B, T), dtype=torch.float64)
    e_s[:, 0] = 1.0
    for name, (qd, kd, vd), qsc, dod, (qr, kr, vr) in _layouts(dev, q, k, v, d_o, qscale):
        lse = R.lse64(qr, kr, num_ims, qsc).float()                   # float64 statistic of the same fp32 q, k, rounded to fp32
        lse_d = lse.to(dev)
        # ---- step
        got = relevance_step(qd, kd, vd, qsc, dod, lse_d, nd, r_in.to(dev))
        again = relevance_step(qd, kd, vd, qsc, dod, lse_d, nd, r_in.to(dev))
        rel, rel_self = relevance_step(qd, kd, vd, qsc, dod, lse_d, nd, r_in.to(dev), outputs=True)
        torch.cuda.synchronize()
        got, again, rel, rel_self = got.cpu(), again.cpu(), rel.cpu(), rel_self.cpu()
        want = R.step64(qr, kr, vr, d_o, num_ims, qsc, r_in)
        assert torch.equal(got, again), name                          # deterministic
        assert torch.equal(rel_self, got[:, 0]) and torch.equal(rel, got[:, 1:]), name     # output form: patch j = row 1 + j
        for b, (err, scale) in enumerate(_slide_errors(got, want, r_in.nan_to_num(0.0), num_ims)):
            print(f"step  {name} T={T} H={nh} hd={hd} slide {b}: err {err:.3e} scale {scale:.3e} ratio {err / scale if scale else 0.0:.3e}")
            assert err <= KERNEL_TOL * scale, (name, b, err, scale)
            assert (got[b, int(num_ims[b]) + 1:] == 0).all(), (name, b)    # padding exactly 0 (and no NaN got through)
            if int(num_ims[b]) == 0:
                assert float(got[b, 0]) == float(r_in[b, 0])            # a slide without patches keeps its r
        assert torch.isfinite(got).all(), name
        # ---- seed: da0 = the output gradient of token 0, lse0 = row 0 of the statistic (strided view: the generic form)
        da0 = d_o[:, 0].contiguous()
        sd = relevance_seed(qd, kd, vd, qsc, da0.to(dev), lse_d[:, :, 0], nd)
        sd2 = relevance_seed(qd, kd, vd, qsc, da0.to(dev), lse_d[:, :, 0].contiguous(), nd)
        srel, sself = relevance_seed(qd, kd, vd, qsc, da0.to(dev), lse_d[:, :, 0], nd, outputs=True)
        torch.cuda.synchronize()
        sd, sd2, srel, sself = sd.cpu(), sd2.cpu(), srel.cpu(), sself.cpu()
        want = R.seed64(qr, kr, vr, da0, num_ims, qsc)
        assert torch.equal(sd, sd2) and torch.equal(sself, sd[:, 0]) and torch.equal(srel, sd[:, 1:]), name
        for b, (err, scale) in enumerate(_slide_errors(sd, want, e_s, num_ims)):
            print(f"seed  {name} T={T} H={nh} hd={hd} slide {b}: err {err:.3e} scale {scale:.3e} ratio {err / scale if scale else 0.0:.3e}")
            assert err <= KERNEL_TOL * scale, (name, b, err, scale)
            assert (sd[b, int(num_ims[b]) + 1:] == 0).all(), (name, b)
        assert float(sd[1, 0]) == 1.0 and torch.isfinite(sd).all()


def test_kernels_clamp_num_ims(dev):
    """num_ims outside [0, T-1] is clamped on the device (no read past the slide's rows)."""
    from paths_amd.saliency import relevance_seed, relevance_step
    T, nh, hd = 65, 4, 32
    q, k, v, d_o, r_in, _, qscale = _operands(T, nh, hd, B=2)
    inside = torch.tensor([T - 1, 0])
    lse = R.lse64(q, k, torch.tensor([T - 1, T - 1]), qscale).float().to(dev)
    args = (q.to(dev), k.to(dev), v.to(dev), qscale)
    outside = torch.tensor([1000, -5], device=dev)
    got = relevance_step(*args, d_o.to(dev), lse, outside, r_in.to(dev))
    want = relevance_step(*args, d_o.to(dev), lse, inside.to(dev), r_in.to(dev))
    assert torch.equal(got, want) and torch.isfinite(got).all()
    assert float(got[1, 0]) == float(r_in[1, 0]) and not got[1, 1:].any()
    da0 = d_o[:, 0].contiguous().to(dev)
    got = relevance_seed(*args, da0, lse[:, :, 0], outside)
    want = relevance_seed(*args, da0, lse[:, :, 0], inside.to(dev))
    assert torch.equal(got, want) and torch.isfinite(got).all() and float(got[1, 0]) == 1.0


# ------------------------------------------------------------------------------------------------
# 2. the whole pass against float64 autograd over the oracle's token sequences
# ------------------------------------------------------------------------------------------------
def _smoke_slides(dev, n=2):
    from paths_amd.data_utils.slide import DeviceSlide
    return [DeviceSlide.synthetic(21, s, (8, 8), num_levels=3, device=dev) for s in range(n)]


def _oracle_levels(monkeypatch, params, ocfg, slides):
    """(xs, num_ims, locs) of every level of the oracle's own recursion over the slides (orc.process_level's probe)."""
    from oracle import paths_oracle as orc
    probes = []
    orig = orc.process_level

    def spy(p, c, depth, fts, locs, num_ims, ctx_slide, ctx_patch, probe=None):
        pr = {}
        res = orig(p, c, depth, fts, locs, num_ims, ctx_slide, ctx_patch, probe=pr)
        probes.append((depth, pr["xs"], num_ims.clone(), locs.clone()))
        return res

    monkeypatch.setattr(orc, "process_level", spy)
    with torch.no_grad():
        orc.inference_end2end(params, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], None, [])
    monkeypatch.setattr(orc, "process_level", orig)
    assert [p[0] for p in probes] == list(range(len(probes)))
    return probes


VARIANTS = {"default": {}, "td192": {"trans_dim": 192}, "layers1": {"trans_layers": 1}, "layers3": {"trans_layers": 3},
            "concat": {"slide_ctx_mode": "concat"}, "none": {"slide_ctx_mode": "none"}}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_recursion_relevance_vs_float64(dev, monkeypatch, variant):
    """The smoke() case (3 levels, B = 2, 8 x 8 base grid, top-k 16) against tests/relevance_ref.py:decoder_relevance64 on the
    oracle's own token sequences, rows matched by location; per level |r - ref|_2 <= 2e-3 |env - e_s|_2 with env the same float64
    computation with |.| in place of (.)^+.  Measured: DESIGN 18."""
    from paths_amd.saliency import attention_relevance, parse_target
    over = dict(SMALL, model_config=VARIANTS[variant]) if VARIANTS[variant] else SMALL
    cfg, model, params = build_model(dev, 5, over)
    mc = cfg.model_config
    slides = _smoke_slides(dev)
    probes = _oracle_levels(monkeypatch, params, H.oracle_config(over), slides)
    assert len(probes) == 3
    for target in ("risk", "logit:1"):
        out, trace = attention_relevance(model, slides, cfg.top_k_patches, 3, target=target)
        assert int(out["status"].item()) == 0 and len(trace) == 3
        ref = R.decoder_relevance64(params, [(xs, nim) for _, xs, nim, _ in probes], mc.trans_heads, mc.trans_layers, mc.slide_ctx_mode,
                                    parse_target(target))
        for (depth, xs, nim, locs), ((rr, rs), (er, es)) in zip(probes, ref):
            rec = trace[depth]
            rel, rel_self = rec["attention_relevance"].cpu().double(), rec["attention_relevance_self"].cpu().double()
            glocs = rec["locs"].cpu()
            err2 = env2 = 0.0
            for b in range(2):
                n = int(nim[b])
                assert int(rec["num_ims"][b]) == n
                where = {tuple(r): i for i, r in enumerate(glocs[b, :n].tolist())}
                idx = torch.tensor([where[tuple(r)] for r in locs[b, :n].tolist()], dtype=torch.long)
                err2 += float(((rel[b, idx] - rr[b, :n]) ** 2).sum() + (rel_self[b] - rs[b]) ** 2)
                env2 += float((er[b, :n] ** 2).sum() + (es[b] - 1.0) ** 2)
                assert (rel[b, n:] == 0).all()
            print(f"e2e {variant} {target} level {depth}: err {math.sqrt(err2):.3e} envelope {math.sqrt(env2):.3e} "
                  f"ratio {math.sqrt(err2) / math.sqrt(env2) if env2 else 0.0:.3e}")
            assert math.sqrt(err2) <= E2E_TOL * math.sqrt(env2), (variant, target, depth, math.sqrt(err2), math.sqrt(env2))
            if variant == "none" and depth < 2:           # no path from this level's aggregator to the target: exactly e_s
                assert not rec["attention_relevance"].any() and (rec["attention_relevance_self"] == 1).all()
            else:
                assert env2 > 0 and float(rec["attention_relevance"].sum()) > 0


# ------------------------------------------------------------------------------------------------
# 3. properties
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def smoke_case(dev):
    """The smoke() case with three slides: model, slides and ONE attention_relevance pass that the tests below share (read only)."""
    from paths_amd.saliency import attention_relevance
    cfg, model, _ = build_model(dev, 5, SMALL)
    slides = _smoke_slides(dev, 3)
    out, trace = attention_relevance(model, slides, cfg.top_k_patches, 3)
    return cfg, model, slides, out, trace


def test_signs_and_padding(smoke_case):
    _, _, slides, out, trace = smoke_case
    assert int(out["status"].item()) == 0
    for rec in trace:
        rel, rel_self, nim = rec["attention_relevance"], rec["attention_relevance_self"], rec["num_ims"]
        assert rel.shape == rec["importance"].shape and rel_self.shape == (len(slides),)
        assert torch.isfinite(rel).all() and (rel >= 0).all() and (rel_self >= 1).all()
        for b in range(len(slides)):
            assert not rel[b, int(nim[b]):].any()
        assert float(rel.sum()) > 0


def test_one_layer_is_linear_in_the_target(dev):
    """trans_layers = 1: the backward is linear in d_logits and a factor 2 is exact, so 2 * risk gives twice the patch relevances, bit
    for bit."""
    from paths_amd.saliency import attention_relevance, risk_score
    cfg, model, _ = build_model(dev, 5, dict(SMALL, model_config={"trans_layers": 1}))
    slides = _smoke_slides(dev)
    with H.spy_calls() as calls:
        _, t1 = attention_relevance(model, slides, cfg.top_k_patches, 3, target="risk")
    assert calls.count(RELEVANCE_CALLS[0]) == 3 and RELEVANCE_CALLS[1] not in calls          # L = 1 needs no T x T pass
    _, t2 = attention_relevance(model, slides, cfg.top_k_patches, 3, target=lambda lg: 2 * risk_score(lg))
    for a, b in zip(t1, t2):
        assert float(a["attention_relevance"].sum()) > 0
        assert torch.equal(2 * a["attention_relevance"], b["attention_relevance"])
        # (self = 1 + x rounds once more: twice the increment up to that rounding)
        assert (2 * (a["attention_relevance_self"].double() - 1) - (b["attention_relevance_self"].double() - 1)).abs().max() <= 1e-6


def test_slides_do_not_interact(smoke_case):
    """A batch of 3 equals each slide alone within 1e-5 (the bar of tests/test_gpu_saliency.py:test_slides_do_not_interact)."""
    from paths_amd.saliency import attention_relevance
    from tests.test_gpu_backward import rel_err
    cfg, model, slides, _, trace = smoke_case
    for b, s in enumerate(slides):
        _, t1 = attention_relevance(model, [s], cfg.top_k_patches, 3)
        for l, (ra, rb) in enumerate(zip(t1, trace)):
            n = int(ra["num_ims"][0])
            assert n == int(rb["num_ims"][b]) and torch.equal(ra["locs"][0, :n], rb["locs"][b, :n])
            e = rel_err(ra["attention_relevance"][0, :n], rb["attention_relevance"][b, :n])
            assert e < 1e-5, (b, l, e)
            assert rel_err(ra["attention_relevance_self"], rb["attention_relevance_self"][b:b + 1]) < 1e-5


def test_fp16_grids_and_host_slides_are_bitwise_the_fp32_resident_result(dev):
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    from paths_amd.saliency import attention_relevance
    cfg, model, _ = build_model(dev, 5, SMALL)
    host16 = [HostSlide.synthetic(21, sid, (8, 8), num_levels=3, device=dev, dtype=F16) for sid in range(2)]
    dev16 = [s.to_device() for s in host16]
    dev32 = [DeviceSlide([g.float() for g in s.grids], patch_size=s.patch_size) for s in dev16]
    ref_out, ref = attention_relevance(model, dev32, cfg.top_k_patches, 3)
    assert float(ref[0]["attention_relevance"].sum()) > 0
    for name, slides in (("fp16 resident", dev16), ("fp16 host", host16)):
        out, tr = attention_relevance(model, slides, cfg.top_k_patches, 3)
        assert torch.equal(out["logits"], ref_out["logits"]) and torch.equal(out["target"], ref_out["target"]), name
        for l, (a, b) in enumerate(zip(tr, ref)):
            assert torch.equal(a["num_ims"], b["num_ims"]), (name, l)
            for key in ("attention_relevance", "attention_relevance_self", "grad_x_input", "grad_norm"):
                assert torch.equal(a[key], b[key]), (name, l, key)
    del host16
    torch.cuda.synchronize()
    empty = getattr(torch._C, "_host_emptyCache", None)
    if empty is not None:
        empty()


def test_zero_children_slides_take_the_careful_path(dev):
    """Slides whose kept patches have no tissue children (tests/test_gpu_saliency.py:test_input_gradients_on_zero_children_slides): the
    pass repeats on the careful path, as input_gradients does, and the records are those of the repeat."""
    from paths_amd.saliency import attention_relevance, input_gradients
    from tests.test_gpu_saliency import _setup
    cfg, model, params, slides, ocfg = _setup(dev, None, wseed=9, dseed=57, top_k=2, base=(4, 4), n_slides=4, p_bg=0.93)
    L = cfg.model_config.trans_layers
    with H.spy_calls() as calls:
        out, trace = attention_relevance(model, slides, cfg.top_k_patches, 5)
    assert "paths_fallback_all_cells" in calls and calls.count("paths_saliency_rows") == 10      # optimistic pass + careful re-run
    assert calls.count(RELEVANCE_CALLS[0]) == 10 and calls.count(RELEVANCE_CALLS[1]) == 10 * (L - 1)
    ref_out, ref = input_gradients(model, slides, cfg.top_k_patches, 5)
    assert torch.equal(out["logits"], ref_out["logits"]) and len(trace) == 5
    for a, b in zip(trace, ref):
        assert torch.equal(a["grad_x_input"], b["grad_x_input"]) and torch.equal(a["num_ims"], b["num_ims"])
        assert (a["attention_relevance"] >= 0).all() and (a["attention_relevance_self"] >= 1).all()
        for s in range(4):
            assert not a["attention_relevance"][s, int(a["num_ims"][s]):].any()


def test_parameter_gradients_and_mode_are_untouched(smoke_case):
    from paths_amd.saliency import attention_relevance
    cfg, model, slides, _, _ = smoke_case
    dev = slides[0].device if hasattr(slides[0], "device") else torch.device("cuda:0")
    model.train()
    try:
        assert all(p.grad is None for p in model.parameters())
        attention_relevance(model, slides, cfg.top_k_patches, 3)
        assert all(p.grad is None for p in model.parameters()) and model.training and all(m.training for m in model.modules())
        g = torch.Generator().manual_seed(1)
        preset = {}
        for i, (n, p) in enumerate(model.named_parameters()):
            if i % 3 == 0:
                p.grad = torch.randn(p.shape, generator=g).to(p.device)
                preset[n] = p.grad.clone()
        model.eval()
        with torch.no_grad():                                    # (the call enables gradients for itself)
            _, trace = attention_relevance(model, slides, cfg.top_k_patches, 3, target="logit:0")
        assert not model.training and float(trace[0]["attention_relevance"].sum()) > 0
        for n, p in model.named_parameters():
            assert (torch.equal(p.grad, preset[n]) if n in preset else p.grad is None), n
        assert all(p.requires_grad for p in model.parameters())
    finally:
        model.zero_grad(set_to_none=True)
        model.eval()


# ------------------------------------------------------------------------------------------------
# 4. nothing else moves
# ------------------------------------------------------------------------------------------------
def test_launch_lists(dev, smoke_case):
    """input_gradients and a training step launch no relevance kernel; attention_relevance launches input_gradients' list, in order,
    plus one seed and L - 1 steps per level with an aggregator gradient, and its other results are input_gradients' bit for bit."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlideBatch
    from paths_amd.saliency import attention_relevance, input_gradients
    cfg, model, slides, out, trace = smoke_case
    L = cfg.model_config.trans_layers
    assert L == 2
    with H.spy_calls() as plain:
        ref_out, ref = input_gradients(model, slides, cfg.top_k_patches, 3)
    assert not any(c in RELEVANCE_CALLS for c in plain) and plain.count("paths_saliency_rows") == 3
    with H.spy_calls() as calls:
        out2, trace2 = attention_relevance(model, slides, cfg.top_k_patches, 3)
    assert [c for c in calls if c not in RELEVANCE_CALLS] == plain
    assert calls.count(RELEVANCE_CALLS[0]) == 3 and calls.count(RELEVANCE_CALLS[1]) == 3 * (L - 1)
    for o in (out, out2):
        assert torch.equal(o["logits"], ref_out["logits"]) and torch.equal(o["target"], ref_out["target"])
    for a, a2, b in zip(trace, trace2, ref):
        assert set(a) == set(b) | {"attention_relevance", "attention_relevance_self"}
        for key in ("grad_x_input", "grad_norm", "logits", "importance", "num_ims"):
            assert torch.equal(a[key], b[key]) and torch.equal(a2[key], b[key]), key
        assert torch.equal(a["attention_relevance"], a2["attention_relevance"])          # reruns are bit-identical
        assert torch.equal(a["attention_relevance_self"], a2["attention_relevance_self"])
    # slide_ctx_mode "none": only the last level has an aggregator gradient
    cfg_n, model_n, _ = build_model(dev, 5, dict(SMALL, model_config={"slide_ctx_mode": "none"}))
    with H.spy_calls() as calls:
        attention_relevance(model_n, slides[:2], cfg_n.top_k_patches, 3)
    assert calls.count(RELEVANCE_CALLS[0]) == 1 and calls.count(RELEVANCE_CALLS[1]) == L - 1
    # one training step
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
    batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    model.train()
    try:
        opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
        with H.spy_calls() as train_calls:
            loss = putils.train_step(model, opt, batch, 3, cfg.top_k_patches)
        assert math.isfinite(float(loss)) and len(train_calls) > 100 and not any(c in RELEVANCE_CALLS for c in train_calls)
    finally:
        model.zero_grad(set_to_none=True)
        model.eval()


# ------------------------------------------------------------------------------------------------
# 5. the curves take the new entry
# ------------------------------------------------------------------------------------------------
def test_perturbation_curves_accept_the_relevance(smoke_case):
    """perturbation_curves ranks by the new [B, N] trace entry; the end points are shared whatever the order."""
    from paths_amd.saliency import perturbation_curves
    cfg, model, slides, _, trace = smoke_case
    own = [dict(rec) for rec in trace]                               # (the curves add their rank to the records: not to the shared ones)
    imp = [dict(rec) for rec in trace]
    a, ta = perturbation_curves(model, slides, cfg.top_k_patches, 3, scores="attention_relevance", trace=own, steps=4)
    b, _ = perturbation_curves(model, slides, cfg.top_k_patches, 3, scores="importance", trace=imp, steps=4)
    assert a["deletion"].shape == (3, 5) and a["insertion"].shape == (3, 5)
    for name in ("deletion", "insertion"):
        assert torch.equal(a[name][:, 0], b[name][:, 0]) and torch.equal(a[name][:, -1], b[name][:, -1])
    assert torch.equal(a["target"], b["target"]) and torch.equal(a["target_baseline"], b["target_baseline"])
    assert all("perturbation_rank" in rec for rec in ta) and torch.isfinite(a["deletion"]).all()
