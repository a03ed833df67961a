"""GPU tests of the hand-written backward kernels against torch autograd (float64) over the oracle's formulas."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def make_level_inputs(B, N, num_ims, depth, D=1024, Dp=1280, seed=0):
    g = torch.Generator().manual_seed(seed)
    valid = torch.arange(N)[None, :] < torch.tensor(num_ims)[:, None]
    fts = (torch.rand(B, N, D, generator=g) * 2 - 1) * math.sqrt(3) * valid[..., None]
    locs = torch.stack((torch.randint(0, 40, (B, N), generator=g), torch.randint(0, 40, (B, N), generator=g)), -1) * 256
    state = (torch.rand(B, N, Dp, generator=g) - 0.5) * valid[..., None] if depth > 0 else None
    return fts, locs, torch.tensor(num_ims), state, valid


def test_gemm_tn_colsum_transpose(dev, monkeypatch):
    from paths_amd import backward as bw, ops
    monkeypatch.setattr(ops, "TRAIN_PLANES", 3)          # (plumbing of panels / accumulate / flags at the exact split; the two-plane default: test_gemm_tn_x6_matches_fp64)
    torch.manual_seed(0)
    M, N1, N2 = 1000, 256, 384
    a, b0, b1 = torch.randn(M, N1), torch.randn(M, 256), torch.randn(M, 128)
    ad, b0d, b1d = a.to(dev), b0.to(dev), b1.to(dev)
    out = torch.full((N1, N2), 7.0, device=dev)
    bw.gemm_tn(ad, N1, b0d, 256, out, M, N1, N2, b1=b1d, ldb1=128, nb0=256)
    ref = a.double().t() @ torch.cat((b0, b1), 1).double()
    assert rel_err(out, ref) < 2e-6
    bw.gemm_tn(ad, N1, b0d, 256, out, M, N1, N2, b1=b1d, ldb1=128, nb0=256, accumulate=True)
    assert rel_err(out, 2 * ref) < 2e-6
    cs = bw.colsum(ad, N1, M, N1)
    assert rel_err(cs, a.double().sum(0)) < 2e-6
    wt = bw.transpose(b0d, M, 256)
    assert torch.equal(wt.cpu(), b0.t())
    # NT with residual / mask / accumulate
    w = torch.randn(128, N1)
    res, mask = torch.randn(M, 128), (torch.randn(M, 128) > 0).float()
    o = torch.ones(M, 128, device=dev)
    wd, resd, maskd = w.to(dev), res.to(dev), mask.to(dev)
    bw.gemm_nt(ad, N1, wd, o, 128, M, 128, N1, residual=resd, ldr=128, mask=maskd, ldm=128, accumulate=True)
    ref = (a.double() @ w.double().t()) * mask.double() + res.double() + 1.0
    assert rel_err(o, ref) < 2e-6
    # a handful of rows (the token-0 chain, M = slides per batch): the one-wave-per-column kernel, strided rows, relu, bias
    for Ms, Ks, Ns in ((8, 512, 128), (3, 128, 512), (16, 384, 128)):
        a_s = torch.randn(Ms, 2, Ks)[:, 0, :]                       # row stride 2 K
        w_s, b_s = torch.randn(Ns, Ks), torch.randn(Ns)
        res_s, mask_s = torch.randn(Ms, Ns), (torch.randn(Ms, Ns) > 0).float()
        full = torch.randn(Ms, 2, Ks)
        full[:, 0, :] = a_s
        fd = full.to(dev)
        o_s = torch.full((Ms, Ns), 2.0, device=dev)
        bw.gemm_nt(fd.data_ptr(), 2 * Ks, w_s.to(dev), o_s, Ns, Ms, Ns, Ks, bias=b_s.to(dev), act=1, residual=res_s.to(dev), ldr=Ns,
                   mask=mask_s.to(dev), ldm=Ns, accumulate=True)
        ref_s = torch.relu(a_s.double() @ w_s.double().t() + b_s.double()) * mask_s.double() + res_s.double() + 2.0
        assert rel_err(o_s, ref_s) < 2e-6, (Ms, Ks, Ns)


@pytest.mark.parametrize("M,N1,N2", [(1000, 192, 576), (5000, 320, 1024), (8, 128, 576), (700, 96, 64), (2049, 768, 192)])
def test_gemm_tn_and_nt_ragged_widths(dev, monkeypatch, M, N1, N2):
    """Widths that are not multiples of 128 (trans_dim 192: 192 / 576 / 768 columns): the f32 TN kernel's edge tiles and the NT
    wrapper's zero-padded weight rows, plain and accumulating, against float64."""
    from paths_amd import backward as bw, ops
    monkeypatch.setattr(ops, "TRAIN_PLANES", 3)
    g = torch.Generator().manual_seed(M + N1)
    a, b = torch.randn(M, N1, generator=g), torch.randn(M, N2, generator=g)
    ad, bd = a.to(dev), b.to(dev)
    out = torch.full((N1, N2), 3.0, device=dev)
    bw.gemm_tn(ad, N1, bd, N2, out, M, N1, N2)
    ref = a.double().t() @ b.double()
    assert rel_err(out, ref) < 2e-6
    bw.gemm_tn(ad, N1, bd, N2, out, M, N1, N2, accumulate=True)
    assert rel_err(out, 2 * ref) < 2e-6
    if N1 % 32 == 0:
        w, bias = torch.randn(N2, N1, generator=g), torch.randn(N2, generator=g)
        o = torch.full((M, N2), 1.0, device=dev)
        bw.gemm_nt(ad, N1, w.to(dev), o, N2, M, N2, N1, bias=bias.to(dev), act=1, accumulate=True)
        assert rel_err(o, torch.relu(a.double() @ w.double().t() + bias.double()) + 1.0) < 2e-6
        wt = bw.transpose(w.to(dev), N2, N1, pad_to=N2 + 32)                 # [N1, N2 + 32], zero padded K
        assert torch.equal(wt[:, :N2].cpu(), w.t()) and float(wt[:, N2:].abs().max()) == 0.0


@pytest.mark.parametrize("M,N1,N2,nb0,pad", [(4096, 256, 512, 256, 0), (1000, 256, 384, 256, 0), (2500, 512, 512, 0, 0),
                                             (777, 128, 128, 0, 0), (5003, 256, 768, 512, 64), (16384, 1792, 2048, 1024, 256)])
@pytest.mark.parametrize("planes", [3, 4])
def test_gemm_tn_x6_matches_fp64(dev, monkeypatch, planes, M, N1, N2, nb0, pad):
    """Split-bf16 weight-gradient kernel vs float64: both tile sizes, ragged M (zero rows past the end come from the buffer range
    check), two-panel B with a row stride wider than the panel, gradients spanning 12 binades, accumulate, bit-reproducible.
    planes 3 = three exact bf16 planes per operand (as accurate as the f32 MFMA), 4 = the training default: two planes, 16 significant
    bits per operand (error of a product ~2e-5, of a sum over M rows well below that)."""
    from paths_amd import backward as bw, ops
    monkeypatch.setattr(ops, "TRAIN_PLANES", planes)
    tol = 2e-6 if planes == 3 else 2e-5
    g = torch.Generator().manual_seed(M + N1)
    a = torch.randn(M, N1, generator=g) * torch.exp2(torch.randint(-30, -18, (M, 1), generator=g).float())
    b = torch.randn(M, N2, generator=g)
    ad = a.to(dev)
    if nb0:
        b0s = torch.zeros(M, nb0 + pad)
        b0s[:, :nb0] = b[:, :nb0]
        b1s = torch.zeros(M, N2 - nb0 + pad)
        b1s[:, :N2 - nb0] = b[:, nb0:]
        b0d, b1d = b0s.to(dev), b1s.to(dev)
        kw = dict(b1=b1d, ldb1=b1s.shape[1], nb0=nb0)
        ldb0 = b0s.shape[1]
    else:
        b0d, kw, ldb0 = b.to(dev), {}, N2
    ref = a.double().t() @ b.double()
    assert bw.TN_MODE == "x6"
    out = torch.full((N1, N2), 3.0, device=dev)
    bw.gemm_tn(ad, N1, b0d, ldb0, out, M, N1, N2, **kw)
    f32 = torch.empty((N1, N2), device=dev)
    bw.TN_MODE = "f32"
    try:
        bw.gemm_tn(ad, N1, b0d, ldb0, f32, M, N1, N2, **kw)
    finally:
        bw.TN_MODE = "x6"
    e6, e32 = rel_err(out, ref), rel_err(f32, ref)
    assert e6 < tol and (planes == 4 or e6 < 1.5 * e32 + 1e-8), (e6, e32)      # three planes: no worse than the f32 MFMA
    out2 = out.clone()
    bw.gemm_tn(ad, N1, b0d, ldb0, out2, M, N1, N2, accumulate=True, **kw)
    assert rel_err(out2, 2 * ref) < tol
    out3 = torch.empty_like(out)
    bw.gemm_tn(ad, N1, b0d, ldb0, out3, M, N1, N2, **kw)
    assert torch.equal(out3, out)


@pytest.mark.parametrize("depth", [0, 2])
def test_selection_chain_backward(dev, depth):
    """LSTM cell + importance MLP + proj_in: gradients of all parameters and of the previous (h|c) state."""
    from oracle import paths_oracle as orc
    from paths_amd import backward as bw, ops
    cfg, model, params = build_model(dev, 21)
    mc = cfg.model_config
    B, N = 2, 160
    fts, locs, num_ims, state, valid = make_level_inputs(B, N, [160, 117], depth, seed=3 + depth)
    lp, vp = ops.pack_lstm(model.lstm), ops.pack_level(model.procs[depth])
    sv = bw.selection_forward_train(mc, lp, vp, fts.to(dev), locs.to(dev), num_ims.to(dev),
                                    state.to(dev) if state is not None else None)
    g = torch.Generator().manual_seed(99)
    tokvalid = torch.cat((torch.ones(B, 1, dtype=torch.bool), valid), 1)
    G_tok = torch.randn(B, N + 1, 128, generator=g) * tokvalid[..., None]
    G_state = torch.randn(B, N, 1280, generator=g) * valid[..., None]
    grads, dprev = bw.selection_backward(mc, lp, vp, sv, G_tok.to(dev), G_state.to(dev))
    lg = bw.unpack_lstm_grads(model.lstm, grads)

    # ---- float64 autograd reference over the oracle's formulas
    p = {k: v.double().requires_grad_(True) for k, v in params.items()}
    X = fts.double()
    pre = f"procs.{depth}."
    if depth == 0:
        h0, c0 = torch.zeros(B, N, 1024, dtype=torch.float64), torch.zeros(B, N, 256, dtype=torch.float64)
        sp = None
    else:
        sp = state.double().requires_grad_(True)
        h0, c0 = sp[..., :1024], sp[..., 1024:]
    hs, cs = orc.lstm_cell(p, X, h0, c0)
    Y = X + hs
    state_out = torch.cat((hs, cs), -1)
    hid = torch.relu(F.linear(Y, p[pre + "importance_mlp.0.weight"], p[pre + "importance_mlp.0.bias"]))
    alpha = torch.sigmoid(F.linear(hid, p[pre + "importance_mlp.2.weight"], p[pre + "importance_mlp.2.bias"]))[..., 0] * valid
    gk = pre + "global_agg."
    pl = torch.div(locs, 256, rounding_mode="floor")
    pe = orc.positional_encoding_2d_from_pos(pl[..., 0].reshape(-1), pl[..., 1].reshape(-1), 128).view(B, N, 128).double()
    tok = F.linear(Y * alpha[..., None], p[gk + "proj_in.weight"], p[gk + "proj_in.bias"]) + pe
    tok = torch.cat((p[gk + "special_token"].view(1, 1, -1).repeat(B, 1, 1), tok), 1)
    # forward parity of the saved tensors
    assert rel_err(sv["tokens"][tokvalid], tok.detach()[tokvalid]) < 1e-5
    assert rel_err(sv["state_out"][valid], state_out.detach()[valid]) < 1e-5
    L = (tok * G_tok.double()).sum() + (state_out * G_state.double()).sum()
    L.backward()
    tol = 2e-4
    for name in ("forget_gate", "remember_gate", "remember_map", "out_select_gate", "mem_to_out"):
        for leaf in ("weight", "bias"):
            ref = p[f"lstm.{name}.0.{leaf}"].grad
            assert rel_err(lg[f"{name}.0.{leaf}"], ref) < tol, (name, leaf)
    w_ip_ref = torch.cat((p[pre + "importance_mlp.0.weight"].grad, p[gk + "proj_in.weight"].grad), 0)
    assert rel_err(grads["w_ip"], w_ip_ref) < tol
    assert rel_err(grads["b1"], p[pre + "importance_mlp.0.bias"].grad) < tol
    assert rel_err(grads["w2"], p[pre + "importance_mlp.2.weight"].grad) < tol
    assert rel_err(grads["b2"], p[pre + "importance_mlp.2.bias"].grad) < tol
    assert rel_err(grads["bp"], p[gk + "proj_in.bias"].grad) < tol
    assert rel_err(grads["special"], p[gk + "special_token"].grad) < tol
    if depth > 0:
        assert rel_err(dprev, sp.grad) < tol
        assert float(dprev[~valid.to(dev)].abs().max()) == 0.0
    else:
        assert dprev is None


def test_transformer_backward(dev):
    """Aggregator (2 post-LN decoder layers over an empty memory, last layer at token 0, decoder.norm, residual,
    classifier): gradients of every live parameter, of the token sequence and of the previous slide context."""
    from oracle import paths_oracle as orc
    from paths_amd import backward as bw, ops
    cfg, model, params = build_model(dev, 33)
    mc = cfg.model_config
    depth, B, N = 1, 3, 150
    num_ims = torch.tensor([150, 97, 31])
    T = N + 1
    g = torch.Generator().manual_seed(5)
    tokvalid = torch.arange(T)[None, :] < (num_ims + 1)[:, None]
    tokens = torch.randn(B, T, 128, generator=g) * tokvalid[..., None]
    ctx_prev = torch.randn(B, 128, generator=g)
    vp = ops.pack_level(model.procs[depth])
    sv = bw.transformer_forward_train(mc, vp, tokens.to(dev), num_ims.to(dev), ctx_prev.to(dev))
    G_log = torch.randn(B, 4, generator=g)
    G_ctx = torch.randn(B, 128, generator=g)
    grads, d_tok, d_ctx = bw.transformer_backward(mc, vp, sv, G_log.to(dev), G_ctx.to(dev))

    p = {k: v.double().requires_grad_(True) for k, v in params.items()}
    tk = tokens.double().requires_grad_(True)
    cp = ctx_prev.double().requires_grad_(True)
    pre = f"procs.{depth}."
    key_pad = ~tokvalid
    S = orc.decoder_stack(p, pre + "global_agg.transformer", tk, key_pad, 4, 2)
    F_ = S[:, 0] + cp
    logits = F.linear(F_, p[pre + "classification_layer.weight"], p[pre + "classification_layer.bias"])
    assert rel_err(sv["logits"], logits.detach()) < 1e-5 and rel_err(sv["ctx_out"], F_.detach()) < 1e-5
    ((logits * G_log.double()).sum() + (F_ * G_ctx.double()).sum()).backward()
    tol = 3e-4
    assert rel_err(d_tok[tokvalid.to(dev)], tk.grad[tokvalid]) < tol
    assert float(d_tok[~tokvalid.to(dev)].abs().max()) == 0.0
    assert rel_err(d_ctx, cp.grad) < tol
    assert rel_err(grads["wcls"], p[pre + "classification_layer.weight"].grad) < tol
    assert rel_err(grads["bcls"], p[pre + "classification_layer.bias"].grad) < tol
    t = pre + "global_agg.transformer.decoder."
    assert rel_err(grads["lnfg"], p[t + "norm.weight"].grad) < tol and rel_err(grads["lnfb"], p[t + "norm.bias"].grad) < tol
    names = {"wqkv": "self_attn.in_proj_weight", "bqkv": "self_attn.in_proj_bias", "wo": "self_attn.out_proj.weight",
             "bo": "self_attn.out_proj.bias", "cab": "multihead_attn.out_proj.bias", "ln1g": "norm1.weight", "ln1b": "norm1.bias",
             "ln2g": "norm2.weight", "ln2b": "norm2.bias", "ln3g": "norm3.weight", "ln3b": "norm3.bias",
             "w1": "linear1.weight", "b1": "linear1.bias", "w2": "linear2.weight", "b2": "linear2.bias"}
    for l in range(2):
        for k, name in names.items():
            ref = p[t + f"layers.{l}.{name}"].grad
            if l == 1 and k in ("wqkv", "bqkv"):
                pass            # last layer: q gradient exists for token 0 only; k,v for all tokens — same tensors, same check
            assert rel_err(grads["layers"][l][k], ref) < tol, (l, k, rel_err(grads["layers"][l][k], ref))


@pytest.mark.parametrize("over", [{}, {"trans_dim": 192}], ids=["shipped", "td192"])
def test_standalone_aggregator_is_differentiable(dev, over):
    """``TransformerAggregator.forward`` (reference model/aggregator.py:58-76) called on its own under autograd: output and the
    gradients of the input sequence, the special token and every decoder parameter against the oracle's float64 autograd."""
    from oracle import paths_oracle as orc
    cfg, model, params = build_model(dev, 21, {"model_config": over} if over else None)
    d = cfg.model_config.trans_dim
    depth, B, N = 2, 2, 90
    lengths = torch.tensor([90, 41])
    g = torch.Generator().manual_seed(9)
    seq = torch.randn(B, N, d, generator=g)
    G_out = torch.randn(B, d, generator=g)
    agg = model.procs[depth].global_agg
    model.train()                                        # (dropout is 0 in the test config: train mode only selects the saving forward)
    x = seq.to(dev).requires_grad_(True)
    out = agg(torch.zeros((B, 0, d), device=dev), x, None, lengths.to(dev))
    (out * G_out.to(dev)).sum().backward()
    p = {k: v.double().requires_grad_(True) for k, v in params.items()}
    pre = f"procs.{depth}.global_agg."
    xs = seq.double().requires_grad_(True)
    S = torch.cat((p[pre + "special_token"].view(1, 1, -1).repeat(B, 1, 1), xs), dim=1)
    key_pad = torch.arange(N + 1)[None, :] >= (lengths + 1)[:, None]
    want = orc.decoder_stack(p, pre + "transformer", S, key_pad, cfg.model_config.trans_heads, cfg.model_config.trans_layers)[:, 0]
    (want * G_out.double()).sum().backward()
    assert rel_err(out.detach(), want.detach()) < 1e-5
    tol = 3e-4
    valid = ~key_pad[:, 1:]
    assert rel_err(x.grad[valid.to(dev)], xs.grad[valid]) < tol
    assert float(x.grad[~valid.to(dev)].abs().max()) == 0.0
    assert rel_err(agg.special_token.grad, p[pre + "special_token"].grad) < tol
    for name, prm in agg.transformer.decoder.named_parameters():
        ref = p[pre + "transformer.decoder." + name].grad
        if "multihead_attn" in name and not name.endswith("out_proj.bias"):
            assert prm.grad is None                      # dead cross-attention matrices: no path to the output
            continue
        assert prm.grad is not None and rel_err(prm.grad, ref) < tol, (name, rel_err(prm.grad, ref))


def _train_setup(dev, wseed=3, dseed=14, top_k=64, base=(16, 16), n_slides=4, cfg_over=None):
    from paths_amd import synthetic as syn
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    cfg, model, params = build_model(dev, wseed, cfg_over, top_k_patches=[top_k] * 4)
    slides = [DeviceSlide.synthetic(dseed, sid, base, p_bg=0.1, device=dev) for sid in range(n_slides)]
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
    batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    return cfg, model, params, slides, batch


def test_recursion_gradients_vs_oracle_autograd(dev):
    """Full 5-level training forward/backward on the device vs torch autograd through the oracle (fp32 CPU)."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils, autograd as pag
    cfg, model, params, slides, batch = _train_setup(dev, top_k=16, base=(6, 7), n_slides=3)
    model.train()
    out = putils.recurse_train(model, batch["slide"], cfg.top_k_patches, 5)
    hazards, loss = putils.loss_from_logits(out["logits"], batch, "survival")
    loss.backward()
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ocfg = H.oracle_config(top_k_patches=[16] * 4)
    labels = {"survival_bin": batch["survival_bin"], "censored": batch["censored"]}
    hz, oloss = orc.inference_end2end(p, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], labels)
    oloss.backward()
    assert abs(float(loss.detach()) - float(oloss.detach())) < 2e-5
    sd = dict(model.named_parameters())
    live = 0
    for k, ref in p.items():
        g = sd[k].grad
        if ref.grad is None:
            assert g is None, k
            continue
        if float(ref.grad.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, k       # dead parameters
            continue
        assert g is not None, k
        assert rel_err(g, ref.grad) < 2e-3, (k, rel_err(g, ref.grad))
        live += 1
    assert live > 100


@pytest.mark.parametrize("over", [{}, {"model_config": {"trans_dim": 192}}, {"model_config": {"lstm": False}}], ids=["default", "td192", "nolstm"])
def test_deferred_slab_reductions_are_bitwise_the_single_launches(dev, monkeypatch, over):
    """csrc/reduce_multi.hip: with the slab reductions of a level's parameter gradients deferred into one launch (the default) every
    gradient equals, bit for bit, the one from a launch per reduction (PATHS_DEFER_REDUCTIONS=0) - same per-element summation order -
    incl. the touch-ups that wait for the flush (proj_in.bias = all rows - special rows, the folded q scale), dropout on."""
    from paths_amd import utils as putils, backward as bw

    def grads(defer):
        monkeypatch.setattr(bw, "DEFER_REDUCTIONS", defer)
        cfg, model, params, slides, batch = _train_setup(dev, top_k=16, base=(6, 7), n_slides=3, cfg_over=dict(over))
        for proc in model.procs:
            proc.config.dropout = 0.05
        model.train()
        torch.manual_seed(5)                         # (restarts the dropout seed sequence: autograd.next_dropout_seed)
        out = putils.recurse_train(model, batch["slide"], cfg.top_k_patches, 5)
        _, loss = putils.loss_from_logits(out["logits"], batch, "survival")
        loss.backward()
        torch.cuda.synchronize()
        assert bw._DEFER["depth"] == 0 and not bw._DEFER["keep"] and not bw._DEFER["post"]
        return {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}, float(loss)

    (g1, l1), (g0, l0) = grads(True), grads(False)
    assert l1 == l0 and g1.keys() == g0.keys() and len(g1) > 50
    for k in g1:
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize("case", range(8))
def test_random_small_training_steps_vs_oracle_autograd(dev, case):
    """A seeded sweep over shapes for the differentiable path (grid shape, background rate incl. fallback slides, batch size, level
    count, top-K incl. keep-all): loss and every live parameter gradient against torch autograd through the oracle."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    rng = np.random.RandomState(2000 + case)
    levels = int(rng.choice([2, 3, 5]))
    base = (int(rng.randint(2, 8)), int(rng.randint(2, 8)))
    B = int(rng.choice([1, 2, 4]))
    p_bg = float(rng.choice([0.0, 0.3, 0.6, 0.85]))
    keeps = [int(rng.choice([-1, 1, 3, 7, 16])) for _ in range(levels - 1)]
    over = {"num_levels": levels}
    cfg, model, params = build_model(dev, 60 + case, over, top_k_patches=keeps)
    slides = [DeviceSlide.synthetic(400 + case, sid, base, num_levels=levels, p_bg=p_bg, device=dev) for sid in range(B)]
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
    batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    model.train()
    _, loss = putils.forward_backward(model, batch, levels, keeps, "survival")
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ocfg = H.oracle_config(over, top_k_patches=keeps)
    hz, oloss = orc.inference_end2end(p, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides],
                                      {"survival_bin": batch["survival_bin"], "censored": batch["censored"]})
    oloss.backward()
    tag = (levels, base, B, p_bg, keeps)
    assert abs(float(loss.detach()) - float(oloss.detach())) < 2e-5, tag
    sd = dict(model.named_parameters())
    live = 0
    for k, ref in p.items():
        g = sd[k].grad
        if ref.grad is None or float(ref.grad.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, (k, tag)
            continue
        assert g is not None, (k, tag)
        assert rel_err(g, ref.grad) < 2e-3, (k, rel_err(g, ref.grad), tag)
        live += 1
    assert live > 20, (live, tag)


def test_recursion_gradients_at_headline_size_vs_oracle_autograd(dev):
    """BASELINE configs[3] shape: the K = 2048 x 5-level training step (top_k 512, the bench's weights and two of its oracle-screened
    slides) - loss and every live parameter gradient of the HIP forward + backward against torch autograd through the oracle (fp32
    CPU), dropout off so that both sides compute the same function."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    K = 2048
    cfg, model, params = build_model(dev, 0, None, top_k_patches=[K // 4] * 4)
    slides = [DeviceSlide.synthetic(1234, sid, (32, 64), device=dev) for sid in (10003, 10004)]
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
    batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    model.train()
    _, loss = putils.forward_backward(model, batch, 5, cfg.top_k_patches, "survival")
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ocfg = H.oracle_config(top_k_patches=[K // 4] * 4)
    hz, oloss = orc.inference_end2end(p, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides],
                                      {"survival_bin": batch["survival_bin"], "censored": batch["censored"]})
    oloss.backward()
    assert abs(float(loss.detach()) - float(oloss.detach())) < 2e-5
    sd = dict(model.named_parameters())
    live, worst = 0, 0.0
    for k, ref in p.items():
        g = sd[k].grad
        if ref.grad is None or float(ref.grad.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        assert g is not None, k
        e = rel_err(g, ref.grad)
        worst = max(worst, e)
        # The last level's importance MLP (first layer) is the one ill-conditioned gradient of this shape: sum over 3,700 rows of
        # (hid > 0) dz w2 with dz = (d_tokens . P) alpha (1 - alpha), two nested cancelling sums.  Measured on the device: inputs that
        # agree to 1e-6 between the split-fp16 and the f32-MFMA forward (each reproduced to 1e-7 by float64 on its own saved tensors)
        # give gradients 1.3e-2 apart; the oracle's fp32 CPU arithmetic is a third such perturbation.
        tol = 3e-2 if k.startswith("procs.4.importance_mlp.0.") else 2e-3
        assert e < tol, (k, e)
        live += 1
    assert live > 100, (live, worst)


def _is_dead(k: str) -> bool:
    """The reference's dead nn.Transformer parameters (encoder, cross-attention matrices): zero gradients there, SURVEY 3.3."""
    return ".encoder." in k or "multihead_attn.in_proj" in k or "multihead_attn.out_proj.weight" in k


@pytest.mark.parametrize("over", [{"lstm": False}, {"slide_ctx_mode": "concat"}, {"lstm": False, "slide_ctx_mode": "concat"},
                                  {"slide_ctx_mode": "none"}, {"importance_mode": "none"}, {"lstm": False, "slide_ctx_mode": "none"}],
                         ids=["nolstm", "concat", "nolstm_concat", "ctx_none", "imp_none", "nolstm_ctx_none"])
def test_variant_training_gradients_vs_oracle_autograd(dev, over):
    """the non-default model variants train on the HIP path too (reference model/paths.py:49-54,101-109: RNN
    hierarchical context instead of the LSTM; :34-37,134-137: slide contexts concatenated into the classifier): 5-level training
    forward / backward on the device vs torch autograd through the oracle, every live parameter."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    cfg_over = {"model_config": dict(over)}
    cfg, model, params, slides, batch = _train_setup(dev, top_k=16, base=(6, 7), n_slides=3, cfg_over=cfg_over)
    model.train()
    _, loss = putils.forward_backward(model, batch, 5, cfg.top_k_patches, "survival")
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ocfg = H.oracle_config(cfg_over, top_k_patches=[16] * 4)
    labels = {"survival_bin": batch["survival_bin"], "censored": batch["censored"]}
    hz, oloss = orc.inference_end2end(p, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], labels)
    oloss.backward()
    assert abs(float(loss.detach()) - float(oloss.detach())) < 2e-5
    sd = dict(model.named_parameters())
    live = 0
    for k, ref in p.items():
        g = sd[k].grad
        if ref.grad is None or float(ref.grad.abs().max()) == 0.0:
            # unused by the oracle's graph: either really unused (grad None) or one of the reference's dead nn.Transformer
            # parameters, which forward_backward fills with the reference's zero gradients
            assert g is None or float(g.abs().max()) == 0.0, k
            # a parameter WITHOUT a path to the loss keeps grad None, as in the reference (torch autograd through the oracle): AdamW
            # must not touch it, weight decay included (importance MLP under importance_mode "none", the earlier levels'
            # aggregators under slide_ctx_mode "none", the classifiers of the non-final levels)
            if ref.grad is None and not _is_dead(k):
                assert g is None, k
            continue
        assert g is not None, k
        assert rel_err(g, ref.grad) < 2e-3, (k, rel_err(g, ref.grad))
        live += 1
    assert live > (15 if over.get("slide_ctx_mode") == "none" else 80)      # ("none": the earlier levels' aggregators do not reach the loss)
    # one AdamW step: parameters the reference leaves alone (grad None) are bit-unchanged, weight decay included; and the fixed
    # all-reduce list is exactly the set of non-dead parameters that got a gradient
    from paths_amd import autograd as pag
    assert {id(q) for q in pag.live_grad_params(model, 5)} == {id(q) for k, q in sd.items() if q.grad is not None and not _is_dead(k)}
    untouched = {k: q.detach().clone() for k, q in sd.items() if p[k].grad is None and not _is_dead(k)}
    assert untouched
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
    assert np.isfinite(float(putils.train_step(model, opt, batch, 5, cfg.top_k_patches)))
    for k, before in untouched.items():
        assert torch.equal(sd[k].detach(), before), k


@pytest.mark.parametrize("over", [{"trans_dim": 192}, {"trans_dim": 64, "trans_heads": 2, "importance_mlp_hidden_dim": 64},
                                  {"trans_dim": 192, "trans_heads": 3, "importance_mlp_hidden_dim": 96, "slide_ctx_mode": "concat"},
                                  {"trans_dim": 96, "trans_heads": 6, "importance_mode": "none", "pos_encoding_mode": "1d"},
                                  {"trans_dim": 192, "lstm": False}, {"trans_dim": 64, "trans_heads": 1, "importance_mlp_hidden_dim": 36, "lstm": False},
                                  {"trans_dim": 256, "trans_heads": 2}, {"trans_dim": 384, "trans_heads": 1, "importance_mlp_hidden_dim": 64},
                                  {"trans_dim": 1536, "trans_heads": 4}, {"trans_dim": 160, "trans_heads": 4}, {"trans_dim": 320, "trans_heads": 4},
                                  {"trans_dim": 128, "trans_heads": 16}],
                         ids=["td192_default", "td64_h2_hi64", "td192_h3_hi96_concat", "td96_h6_impnone_pe1d", "td192_nolstm", "td64_h1_hi36_nolstm",
                              "td256_h2_hd128", "td384_h1_hd384", "td1536_h4_hd384", "td160_h4_hd40_padded", "td320_h4_hd80_padded", "td128_h16_hd8_padded"])
def test_training_other_aggregator_geometries_vs_oracle_autograd(dev, over):
    """the reference's config surface (config.py:30-36) trains too - trans_dim 192 / head_dim 48 is its dataclass
    default.  5-level training forward / backward on the shape-generic kernels (csrc/generic.hip TRAIN attention, csrc/generic_bwd.hip)
    vs torch autograd through the oracle, every live parameter; then one AdamW step."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    cfg_over = {"model_config": dict(over)}
    cfg, model, params, slides, batch = _train_setup(dev, top_k=16, base=(6, 7), n_slides=3, cfg_over=cfg_over)
    model.train()
    with H.spy_calls() as calls:
        _, loss = putils.forward_backward(model, batch, 5, cfg.top_k_patches, "survival")
    wide = over["trans_dim"] // over.get("trans_heads", 4) > 64        # head_dim > 64: csrc/attn_wide.hip
    assert ({"paths_attention_wide_bwd", "paths_attention_wide_fwd"} if wide else {"paths_attention_bwd_any", "paths_attention_any_train"}) <= set(calls)
    assert ("paths_importance_rows_bwd_any" if over.get("lstm") is False else "paths_importance_bwd_any") in calls
    assert not {"paths_attention_bwd_x6_dropout", "paths_attention_bwd_x6_planes", "paths_importance_bwd", "paths_importance_rows_bwd", "paths_importance_proj"} & set(calls)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ocfg = H.oracle_config(cfg_over, top_k_patches=[16] * 4)
    labels = {"survival_bin": batch["survival_bin"], "censored": batch["censored"]}
    hz, oloss = orc.inference_end2end(p, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], labels)
    oloss.backward()
    assert abs(float(loss.detach()) - float(oloss.detach())) < 2e-5
    sd = dict(model.named_parameters())
    live = 0
    for k, ref in p.items():
        g = sd[k].grad
        if ref.grad is None or float(ref.grad.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, k
            if ref.grad is None and not _is_dead(k):
                assert g is None, k
            continue
        assert g is not None, k
        # importance hidden 36 without the LSTM: the one-element output biases of the importance MLP (each the sum over every row
        # of its level of a cancelling term) are the ill-conditioned gradients of this geometry.  Measured on the device against a
        # float64 evaluation of the oracle: levels 1 and 3 at 2.69e-3 and 2.17e-3 (every other parameter of all twelve geometries
        # <= 1.6e-3); the fp32 oracle itself lands up to 2.2e-3 away from the float64 value there, depending on the host's thread
        # count, so the earlier 2e-3 held or failed with the CPU that ran the oracle.
        tol = 3e-3 if over.get("importance_mlp_hidden_dim") == 36 and k.endswith("importance_mlp.2.bias") else 2e-3
        assert rel_err(g, ref.grad) < tol, (k, rel_err(g, ref.grad))
        live += 1
    assert live > 80
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
    assert np.isfinite(float(putils.train_step(model, opt, batch, 5, cfg.top_k_patches)))


def test_training_td192_at_k256_vs_oracle_autograd(dev):
    """The shape-generic training kernels at sequence lengths that span many key / query blocks (K = 256: up to 1,025 tokens per slide,
    ragged num_ims): loss and every live gradient of the reference-default geometry against torch autograd through the oracle."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    cfg_over = {"model_config": {"trans_dim": 192}}
    cfg, model, params, slides, batch = _train_setup(dev, wseed=8, dseed=23, top_k=256, base=(18, 20), n_slides=2, cfg_over=cfg_over)
    model.train()
    _, loss = putils.forward_backward(model, batch, 5, cfg.top_k_patches, "survival")
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ocfg = H.oracle_config(cfg_over, top_k_patches=[256] * 4)
    labels = {"survival_bin": batch["survival_bin"], "censored": batch["censored"]}
    hz, oloss = orc.inference_end2end(p, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], labels)
    oloss.backward()
    assert abs(float(loss.detach()) - float(oloss.detach())) < 2e-5
    sd = dict(model.named_parameters())
    live = 0
    for k, ref in p.items():
        if ref.grad is None or float(ref.grad.abs().max()) == 0.0:
            continue
        assert sd[k].grad is not None and rel_err(sd[k].grad, ref.grad) < 2e-3, (k, rel_err(sd[k].grad, ref.grad))
        live += 1
    assert live > 100


def test_training_on_zero_children_slides_takes_the_fallback(dev):
    """the training path reads the recursion's status word too.  Slides whose kept patches have no tissue children
    (reference fallback to all cells with zero parent state, data_utils/slide.py:336-352) train through the careful
    differentiable pass: loss and every live gradient equal torch autograd through the oracle."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    cfg, model, params = build_model(dev, 9, None, top_k_patches=[2] * 4)
    slides = [DeviceSlide.synthetic(57, sid, (4, 4), p_bg=0.93, device=dev) for sid in range(4)]
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
    batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    model.train()
    fast = putils.recurse_train(model, batch["slide"], cfg.top_k_patches, 5)
    assert int(fast["status"].item()) & 1, "test slides should trigger the fallback"
    model.zero_grad(set_to_none=True)
    _, loss = putils.forward_backward(model, batch, 5, cfg.top_k_patches, "survival")
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ocfg = H.oracle_config(top_k_patches=[2] * 4)
    hz, oloss = orc.inference_end2end(p, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides],
                                      {"survival_bin": batch["survival_bin"], "censored": batch["censored"]})
    oloss.backward()
    assert abs(float(loss.detach()) - float(oloss.detach())) < 2e-5
    sd = dict(model.named_parameters())
    live = 0
    for k, ref in p.items():
        if ref.grad is None or float(ref.grad.abs().max()) == 0.0:
            continue
        assert sd[k].grad is not None and rel_err(sd[k].grad, ref.grad) < 2e-3, (k, rel_err(sd[k].grad, ref.grad))
        live += 1
    assert live > 100


@pytest.mark.parametrize("M,N,K", [(2048, 1024, 1792), (1500, 128, 512), (4099, 256, 128), (1024, 384, 128)])
@pytest.mark.parametrize("planes", [3, 4])
def test_gemm_nt_train_planes_matches_fp64(dev, monkeypatch, planes, M, N, K):
    """dX = dY W on the split-bf16 kernel at BOTH training settings against float64 (the two-plane default of the dX
    GEMM had no unit test): gradient rows spread over 24 binades, bias, relu, mask, residual, accumulate, ragged M.  planes 3 =
    three exact bf16 planes (fp32-accurate), 4 = two planes (16 significant bits per operand: a product ~2e-5)."""
    from paths_amd import backward as bw, ops
    monkeypatch.setattr(ops, "TRAIN_PLANES", planes)
    tol = 2e-6 if planes == 3 else 3e-5
    g = torch.Generator().manual_seed(M + N + K)
    dy = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-28, -4, (M, 1), generator=g).float())
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g) * 2.0 ** -16
    res = torch.randn(M, N, generator=g) * 2.0 ** -16
    mask = (torch.rand(M, N, generator=g) > 0.3).float()
    dyd, wd = dy.to(dev), w.to(dev)
    assert M >= bw.NT_X6_MIN_M and N % bw.NT_X6_MIN_N == 0 and K % 128 == 0      # (the split kernel is the one that runs)
    o = torch.empty(M, N, device=dev)
    bw.gemm_nt(dyd, K, wd, o, N, M, N, K)
    ref = dy.double() @ w.double().t()
    row_rel = ((o.cpu().double() - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-300)).max().item()      # PER ROW: small-gradient rows count
    assert row_rel < 3 * tol, row_rel         # (max-norm per row: fp32 accumulation over K = 1792 alone is ~2.5e-6 there)
    assert rel_err(o, ref) < tol
    o2 = torch.full((M, N), 2.0 ** -16, device=dev)
    bw.gemm_nt(dyd, K, wd, o2, N, M, N, K, bias=bias.to(dev), act=1, residual=res.to(dev), ldr=N, mask=mask.to(dev), ldm=N, accumulate=True)
    ref2 = torch.relu(ref + bias.double()) * mask.double() + res.double() + 2.0 ** -16
    assert rel_err(o2, ref2) < tol
    o3 = torch.empty_like(o)
    bw.gemm_nt(dyd, K, wd, o3, N, M, N, K)
    assert torch.equal(o3, o)


@pytest.mark.parametrize("name,forced", [("g6_train_16x16_top64", False), ("g13_train_td192_8x8_top16", False), ("g13_train_td64_h2_hi32_8x8_top16", False),
                                         ("g14_train_td256_h2_8x8_top16", False), ("g15_train_td160_h4_8x8_top16", False),
                                         ("g6_train_16x16_top64", True), ("g13_train_td192_8x8_top16", True)])
def test_three_adamw_steps_match_reference_g6(dev, monkeypatch, name, forced):
    """Reference train-step semantics (train.py:49-50,59-68): losses of 3 AdamW steps vs the fixtures captured from the
    reference (G6: the shipped geometry; G13: its dataclass-default trans_dim 192 and a small free geometry, on the shape-generic
    training kernels), dead parameters included in weight decay, unused classifiers left with grad None.
    ``forced``: the row-count thresholds of the split-bf16 gradient GEMMs lowered to 64 rows, so that the TWO-PLANE kernels of
    the training default (PATHS_TRAIN_PLANES=4) - which these small fixtures otherwise hardly reach - produce every eligible dX / dW
    of the three steps; the same 1e-5 loss bar."""
    from paths_amd import utils as putils, backward as bw, ops
    from tests.conftest import load_golden
    if forced:
        assert ops.TRAIN_PLANES == 4 or os.environ.get("PATHS_TRAIN_PLANES") == "3"
        monkeypatch.setattr(bw, "NT_X6_MIN_M", 64)         # (the fixtures' levels have B x 64 ... B x 257 rows; the 8-row token-0 chain
        monkeypatch.setattr(bw, "TN_X6_MIN_M", 64)         #  keeps its one-wave-per-column kernel)
        calls = {"nt": 0, "tn": 0}
        real_call = bw._lib.call

        def counting_call(fname, *a):
            if fname == "paths_gemm_nt_x6":
                calls["nt"] += 1
            elif fname == "paths_gemm_tn_x6":
                calls["tn"] += 1
            return real_call(fname, *a)
        monkeypatch.setattr(bw._lib, "call", counting_call)
    g, info = load_golden(name)
    cfg, model, params, slides, batch = _train_setup(dev, info["wseed"], info["dseed"], info["top_k"], tuple(info["base_shape"]), info["B"],
                                                     cfg_over=info.get("cfg_over") or None)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=info["lr"], weight_decay=info["weight_decay"])
    losses = []
    for _ in range(len(g["losses"])):
        losses.append(float(putils.train_step(model, opt, batch, 5, cfg.top_k_patches)))
    np.testing.assert_allclose(losses, g["losses"], atol=1e-5, rtol=0)      # SURVEY 8(a) row T bar; measured: <= 4e-7
    none = sorted(n for n, p_ in model.named_parameters() if p_.grad is None)
    assert none == sorted(info["grad_none"])
    if forced:
        assert calls["nt"] >= 15 and calls["tn"] >= 15, calls      # the split kernels really produced the gradients


def _adamw_pair(dev, shapes, flavor=None, **kw):
    from paths_amd import optim as popt
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(*sh, generator=g) * (10.0 ** float(torch.randint(-4, 2, (1,), generator=g))) for sh in shapes]
    pa = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    pb = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    if flavor is not None:
        popt.FLAVOR = flavor
    return pa, pb, torch.optim.AdamW(pa, foreach=True, **kw), popt.HipAdamW(pb, **kw), g


def test_hip_adamw_is_bitwise_torch_foreach(dev):
    """paths_amd.optim.HipAdamW (one launch per step, csrc/optim.hip) against torch.optim.AdamW(foreach=True) - the reference's
    optimizer (train.py:49-50) - BIT FOR BIT over 6 steps: parameters, exp_avg, exp_avg_sq; odd sizes (unaligned tails, scalars),
    gradients over 12 binades, a parameter whose grad is None on some steps (its step count lags, as the non-final classifiers'),
    weight decay on and off, lr changed between steps (ExponentialLR), state_dict round trip into torch's class."""
    from paths_amd import optim as popt
    shapes = [(1792, 2048), (1024,), (3, 5, 7), (1,), (4097,), (128, 128), (513, 3)]
    for wd in (0.01, 0.0):
        pa, pb, oa, ob, g = _adamw_pair(dev, shapes, lr=2e-3, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
        for it in range(6):
            for i, (a, b) in enumerate(zip(pa, pb)):
                if i == 2 and it in (1, 4):
                    a.grad = b.grad = None
                    continue
                gr = (torch.randn(a.shape, generator=g) * torch.exp2(torch.randint(-20, 4, (1,), generator=g).float())).to(dev)
                a.grad, b.grad = gr.clone(), gr.clone()
            oa.step(); ob.step()
            if it == 2:
                for o in (oa, ob):
                    o.param_groups[0]["lr"] *= 0.93
            for i, (a, b) in enumerate(zip(pa, pb)):
                assert torch.equal(a, b), (wd, it, i, float((a - b).abs().max()))
                assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]), (wd, it, i)
                assert float(oa.state[a]["step"]) == float(ob.state[b]["step"])
        # torch's class loads our state and continues identically (checkpoint compatibility, reference utils / train.py save + reload)
        oc = torch.optim.AdamW(pb, foreach=True, lr=oa.param_groups[0]["lr"], weight_decay=wd)
        oc.load_state_dict(ob.state_dict())
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g).to(dev)
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step(); oc.step()
        assert all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_hip_adamw_five_param_groups_without_host_sync(dev):
    """HipAdamW as a drop-in for ``torch.optim.AdamW`` (reference train.py:49-50) in a loop that NEVER synchronises, with five
    parameter groups (own lr / weight decay each): 12 steps enqueued back to back - gradients pre-generated on the device, so the
    host runs ahead of the GPU by the whole loop and every pinned staging slot is rewritten while older copies are still queued
    (the 4-slot ring is per parameter map and waits for the slot's own copy event).  Bit-identical to torch's foreach
    update at the end."""
    from paths_amd import optim as popt
    shapes = [(1792, 2048), (1024,), (513, 3), (4097,), (128, 128), (1,), (3, 5, 7), (256, 1024), (64,), (1000, 130)]
    g = torch.Generator().manual_seed(11)
    base = [torch.randn(*sh, generator=g) * 0.1 for sh in shapes]
    pa = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    pb = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    groups = lambda ps: [{"params": ps[2 * i:2 * i + 2], "lr": 1e-3 * (i + 1), "weight_decay": 0.01 * (i % 3)} for i in range(5)]
    oa, ob = torch.optim.AdamW(groups(pa), foreach=True), popt.HipAdamW(groups(pb))
    steps = 12
    grads = [[(torch.randn(sh, generator=g) * 2.0 ** float(torch.randint(-12, 2, (1,), generator=g))).to(dev) for sh in shapes] for _ in range(steps)]
    big = torch.randn((4096, 4096), device=dev)
    torch.cuda.synchronize()
    for _ in range(40):                      # ~10 ms of queued device work: the optimizer loops below are enqueued far ahead of the GPU
        big = big @ big * 1e-3
    for it in range(steps):
        for b, gr in zip(pb, grads[it]):
            b.grad = gr
        ob.step()
    for it in range(steps):
        for a, gr in zip(pa, grads[it]):
            a.grad = gr
        oa.step()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]), i


def test_data_parallel_shards_sum_to_global_batch(dev):
    """Two simulated ranks on one GPU (RCCL refuses two ranks of one communicator on the same device): the sum of the
    shards' gradients (each loss scaled by local/global batch) equals the single-rank global-batch gradient."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlideBatch
    from paths_amd.distributed import shard_range
    cfg, model, params, slides, batch = _train_setup(dev, top_k=16, base=(8, 8), n_slides=4)
    model.train()

    def grads_for(idx, global_batch):
        model.zero_grad(set_to_none=True)
        sub = {"slide": DeviceSlideBatch([slides[i] for i in idx]), "survival_bin": batch["survival_bin"][idx],
               "censored": batch["censored"][idx]}
        out = putils.recurse_train(model, sub["slide"], cfg.top_k_patches, 5)
        _, loss = putils.loss_from_logits(out["logits"], sub, "survival", global_batch)
        loss.backward()
        return {n: p_.grad.clone() for n, p_ in model.named_parameters() if p_.grad is not None}, float(loss)

    full, lf = grads_for(list(range(4)), 4)
    parts = [grads_for(list(shard_range(4, r, 2)), 4) for r in range(2)]
    assert abs(lf - (parts[0][1] + parts[1][1])) < 1e-6
    for n, gfull in full.items():
        s = parts[0][0][n] + parts[1][0][n]
        assert rel_err(s, gfull) < 2e-5, n


def test_dropin_process_is_differentiable(dev):
    """``model(depth, PatchBatch)`` under grad mode (the reference's host loop + loss.backward(), train.py:62-65)."""
    from oracle import paths_oracle as orc
    from paths_amd.data_utils.patch_batch import PatchBatch
    cfg, model, params = build_model(dev, 12)
    model.train()
    depth, B, N = 2, 2, 64
    fts, locs, num_ims, state, valid = make_level_inputs(B, N, [64, 40], depth, seed=8)
    ctx_patch = torch.zeros(B, N, depth, 1280); ctx_patch[:, :, -1] = state
    ctx_slide = torch.randn(B, depth, 128, generator=torch.Generator().manual_seed(2))
    cp_d = ctx_patch.to(dev).requires_grad_(True)
    cs_d = ctx_slide.to(dev).requires_grad_(True)
    pb = PatchBatch(locs=locs.to(dev), num_ims=num_ims.to(dev), parent_inds=torch.zeros(B, N, dtype=torch.int64, device=dev),
                    ctx_slide=cs_d, ctx_patch=cp_d, fts=fts.to(dev))
    out = model(depth, pb)
    G1 = torch.randn(B, 4, generator=torch.Generator().manual_seed(3))
    G2 = torch.randn(B, N, 1280, generator=torch.Generator().manual_seed(4)) * valid[..., None]
    ((out["logits"] * G1.to(dev)).sum() + (out["ctx_patch"] * G2.to(dev)).sum()).backward()
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    cp, cs = ctx_patch.clone().requires_grad_(True), ctx_slide.clone().requires_grad_(True)
    ref = orc.process_level(p, H.oracle_config(), depth, fts, locs, num_ims, cs, cp)
    ((ref["logits"] * G1).sum() + (ref["ctx_patch"] * G2).sum()).backward()
    assert rel_err(cs_d.grad, cs.grad) < 1e-3 and rel_err(cp_d.grad[:, :, -1][valid], cp.grad[:, :, -1][valid]) < 1e-3
    sd = dict(model.named_parameters())
    for k in ("lstm.forget_gate.0.weight", "procs.2.importance_mlp.0.weight", "procs.2.global_agg.proj_in.weight",
              "procs.2.global_agg.transformer.decoder.layers.0.linear1.weight", "procs.2.classification_layer.weight"):
        assert rel_err(sd[k].grad, p[k].grad) < 2e-3, k


def test_train_loop_harness(dev, tmp_path):
    """reference train.py:31-116 semantics end to end on synthetic slides: loss goes down, checkpoints are written in
    the reference's format, a second call resumes from the saved epoch, the test split is evaluated."""
    import os, pickle
    from paths_amd.config import Config
    from paths_amd.train import synthetic_dataset, train_loop
    cfg = Config.load(os.path.join(os.path.dirname(__file__), "golden", "sample"), test_mode=True)
    cfg.model_config.dropout = 0.0
    cfg.num_levels, cfg.top_k_patches, cfg.batch_size = 3, [8, 8], [4, 4, 4]
    cfg.num_epochs, cfg.lr, cfg.early_stopping, cfg.eval_epochs = 3, 2e-4, True, 1
    torch.manual_seed(0)
    model = cfg.get_model().to(dev)
    ds = synthetic_dataset(14, (6, 6), 3, dev, seed=77)
    logs = []
    stats = train_loop(model, ds[6:], ds[:3], ds[3:6], cfg, str(tmp_path), log=logs.append)
    tl = [stats["train_loss"][e] for e in (1, 2, 3)]
    assert tl[2] < tl[0], tl
    assert set(stats["val_c-index"].keys()) == {1, 2, 3} and all(0.0 <= v <= 1.0 for v in stats["val_c-index"].values())
    assert "test" in stats and "test_c-index" in stats["test"]
    assert os.path.isfile(tmp_path / "model.pt") and pickle.load(open(tmp_path / "train_stats.pkl", "rb"))["epoch"] == 3
    # resume: nothing left to train (start epoch 3 == num_epochs -> one more epoch as in the reference's inclusive range)
    cfg.early_stopping = False
    model2 = cfg.get_model().to(dev)
    stats2 = train_loop(model2, ds[6:], None, None, cfg, str(tmp_path), log=logs.append)
    assert stats2["epoch"] == 3 and 3 in stats2["train_loss"]


# ------------------------------------------------------------------------------------------------
# dropout (reference nn.Transformer(..., dropout=p), model/aggregator.py:25-33; shipped configs: p = 0.05)
# ------------------------------------------------------------------------------------------------
def _mask(dev, key, n, p):
    from paths_amd import _lib
    m = torch.empty(n, device=dev)
    _lib.call("paths_dropout_mask", m.data_ptr(), n, key, p, _lib.stream())
    return m


def test_dropout_mask_statistics(dev):
    """Counter-based masks: keep rate 1 - p, reproducible from (key, index), independent across sites / layers / levels / seeds and
    along the index (no lattice structure at the strides the kernels use)."""
    from paths_amd import backward as bw
    n, p = 1 << 22, 0.05
    d0 = bw.Drop(p, 12345, 1)
    m = _mask(dev, d0.key(0, bw.Drop.SA_OUT), n, p)
    assert torch.equal(m, _mask(dev, d0.key(0, bw.Drop.SA_OUT), n, p))                       # a function of (key, index) only
    rate = 1.0 - float(m.mean())
    p16 = round(p * 65536) / 65536.0                                                         # one 32-bit hash serves two elements: 16-bit threshold
    assert abs(p16 - p) < 1e-5 and abs(rate - p16) < 4 * np.sqrt(p * (1 - p) / n), rate     # 4 sigma
    others = [d0.key(0, bw.Drop.CA_OUT), d0.key(1, bw.Drop.SA_OUT), bw.Drop(p, 12345, 2).key(0, bw.Drop.SA_OUT),
              bw.Drop(p, 12346, 1).key(0, bw.Drop.SA_OUT)]
    keep = m - m.mean()
    for k in others:
        o = _mask(dev, k, n, p)
        corr = float((keep * (o - o.mean())).mean()) / (p * (1 - p))
        assert abs(corr) < 5 / np.sqrt(n), corr                                            # uncorrelated masks
    for lag in (1, 4, 128, 512, 2049, 128 * 2049):                                         # neighbours in a row / column / key row
        corr = float((keep[:-lag] * keep[lag:]).mean()) / (p * (1 - p))
        assert abs(corr) < 5 / np.sqrt(n), (lag, corr)
    assert float(_mask(dev, d0.key(0, 0), 1000, 0.0).min()) == 1.0                         # p = 0: everything kept


@pytest.mark.parametrize("geo", [{}, {"trans_dim": 192}, {"trans_dim": 128, "trans_heads": 2}, {"trans_dim": 64, "trans_heads": 4}],
                         ids=["shipped_128x4", "td192_hd48", "td128_hd64", "td64_hd16"])
def test_dropout_forward_backward_vs_fp64_with_exported_masks(dev, geo):
    """All five dropout sites of both decoder layers (the last one at token 0 only): forward outputs and every gradient of the HIP
    training path against float64 autograd through a reference that multiplies by the SAME masks (exported by paths_dropout_mask).
    The shipped geometry runs the 128-wide kernels, the others the shape-generic ones (csrc/generic.hip TRAIN attention,
    csrc/generic_bwd.hip): same mask element indices at every site."""
    from paths_amd import ops as _ops
    if _ops.GEMM_MODE == "f32":
        pytest.skip("dropout needs the split-operand attention kernel: PATHS_GEMM_MODE=f32 rejects it loudly (backward.py)")
    from paths_amd import backward as bw, ops
    cfg, model, params = build_model(dev, 33, {"model_config": dict(geo)} if geo else None)
    mc = cfg.model_config
    depth, B, N, H, pd = 1, 3, 150, mc.trans_heads, 0.1
    d = mc.trans_dim
    hd = d // H
    num_ims = torch.tensor([150, 97, 31])
    T = N + 1
    g = torch.Generator().manual_seed(5)
    tokvalid = torch.arange(T)[None, :] < (num_ims + 1)[:, None]
    tokens = torch.randn(B, T, d, generator=g) * tokvalid[..., None]
    ctx_prev = torch.randn(B, d, generator=g)
    vp = ops.pack_level(model.procs[depth])
    drop = bw.Drop(pd, 0xC0FFEE, depth)
    sv = bw.transformer_forward_train(mc, vp, tokens.to(dev), num_ims.to(dev), ctx_prev.to(dev), drop)
    G_log = torch.randn(B, 4, generator=g)
    G_ctx = torch.randn(B, d, generator=g)
    grads, d_tok, d_ctx = bw.transformer_backward(mc, vp, sv, G_log.to(dev), G_ctx.to(dev))

    sc = 1.0 / (1.0 - round(pd * 65536) / 65536.0)      # the rate actually applied: a 16-bit threshold (csrc/dropout.h)

    def mk(layer, site, shape):
        if site == bw.Drop.ATTN:                         # attention rows are T rounded up to even elements apart (drop_attn_stride)
            stride = (shape[-1] + 1) & ~1
            m = _mask(dev, drop.key(layer, site), int(np.prod(shape[:-1])) * stride, pd).cpu().double().view(*shape[:-1], stride)
            return m[..., :shape[-1]] * sc
        return (_mask(dev, drop.key(layer, site), int(np.prod(shape)), pd).cpu().double() * sc).view(*shape)

    p = {k: v.double().requires_grad_(True) for k, v in params.items()}
    tk = tokens.double().requires_grad_(True)
    cp = ctx_prev.double().requires_grad_(True)
    pre = f"procs.{depth}."
    t = pre + "global_agg.transformer.decoder."

    def layer(l, S, rows_q):
        """S [B,T,d]; returns the layer output for query rows rows_q (slice(None) = all, or [0]); masks indexed like the kernels"""
        q_ = t + f"layers.{l}."
        qkv = F.linear(S, p[q_ + "self_attn.in_proj_weight"], p[q_ + "self_attn.in_proj_bias"])
        qq, kk, vv = [x.view(B, T, H, hd).transpose(1, 2) for x in qkv.split(d, dim=-1)]
        scores = (qq @ kk.transpose(-1, -2)) / np.sqrt(float(hd))
        scores = scores.masked_fill(~tokvalid[:, None, None, :], float("-inf"))
        A = torch.softmax(scores, dim=-1) * mk(l, bw.Drop.ATTN, (B, H, T, T))
        att = (A @ vv).transpose(1, 2).reshape(B, T, d)[:, rows_q]
        x = S[:, rows_q]
        R = x.shape[1]
        sa = F.linear(att, p[q_ + "self_attn.out_proj.weight"], p[q_ + "self_attn.out_proj.bias"])
        x = F.layer_norm(x + sa * mk(l, bw.Drop.SA_OUT, (B, R, d)), (d,), p[q_ + "norm1.weight"], p[q_ + "norm1.bias"])
        x = F.layer_norm(x + p[q_ + "multihead_attn.out_proj.bias"] * mk(l, bw.Drop.CA_OUT, (B, R, d)), (d,), p[q_ + "norm2.weight"], p[q_ + "norm2.bias"])
        hid = torch.relu(F.linear(x, p[q_ + "linear1.weight"], p[q_ + "linear1.bias"])) * mk(l, bw.Drop.FF_INNER, (B, R, 4 * d))
        ff = F.linear(hid, p[q_ + "linear2.weight"], p[q_ + "linear2.bias"])
        return F.layer_norm(x + ff * mk(l, bw.Drop.FF_OUT, (B, R, d)), (d,), p[q_ + "norm3.weight"], p[q_ + "norm3.bias"])

    S1 = layer(0, tk, slice(None))
    x3 = layer(1, S1, slice(0, 1))[:, 0]                 # the last layer is only read at token 0 (reference model/aggregator.py:75)
    F_ = F.layer_norm(x3, (d,), p[t + "norm.weight"], p[t + "norm.bias"]) + cp
    logits = F.linear(F_, p[pre + "classification_layer.weight"], p[pre + "classification_layer.bias"])
    assert rel_err(sv["logits"], logits.detach()) < 1e-5 and rel_err(sv["ctx_out"], F_.detach()) < 1e-5
    plain = bw.transformer_forward_train(mc, vp, tokens.to(dev), num_ims.to(dev), ctx_prev.to(dev))
    assert rel_err(sv["logits"], plain["logits"]) > 1e-3                                   # the masks do something
    ((logits * G_log.double()).sum() + (F_ * G_ctx.double()).sum()).backward()
    tol = 3e-4
    assert rel_err(d_tok[tokvalid.to(dev)], tk.grad[tokvalid]) < tol
    assert rel_err(d_ctx, cp.grad) < tol
    assert rel_err(grads["wcls"], p[pre + "classification_layer.weight"].grad) < tol
    assert rel_err(grads["lnfg"], p[t + "norm.weight"].grad) < tol and rel_err(grads["lnfb"], p[t + "norm.bias"].grad) < tol
    names = {"wqkv": "self_attn.in_proj_weight", "bqkv": "self_attn.in_proj_bias", "wo": "self_attn.out_proj.weight",
             "bo": "self_attn.out_proj.bias", "cab": "multihead_attn.out_proj.bias", "ln1g": "norm1.weight", "ln1b": "norm1.bias",
             "ln2g": "norm2.weight", "ln2b": "norm2.bias", "ln3g": "norm3.weight", "ln3b": "norm3.bias",
             "w1": "linear1.weight", "b1": "linear1.bias", "w2": "linear2.weight", "b2": "linear2.bias"}
    for l in range(2):
        for k, name in names.items():
            ref = p[t + f"layers.{l}.{name}"].grad
            assert rel_err(grads["layers"][l][k], ref) < tol, (l, k, rel_err(grads["layers"][l][k], ref))


def test_training_with_shipped_dropout_config(dev):
    """models/sample/config.json as shipped (dropout 0.05) trains: the masks follow torch.manual_seed (same seed -> bit-identical
    loss and gradients, another seed -> different), eval mode is untouched by the dropout setting."""
    from paths_amd import ops as _ops
    if _ops.GEMM_MODE == "f32":
        pytest.skip("dropout needs the split-operand attention kernel: PATHS_GEMM_MODE=f32 rejects it loudly (backward.py)")
    from paths_amd import utils as putils
    cfg, model, params, slides, batch = _train_setup(dev, top_k=16, base=(6, 7), n_slides=3)
    for proc in model.procs:
        proc.config.dropout = 0.05
    model.eval()
    with torch.no_grad():
        ev = putils.recurse(model, batch["slide"], cfg.top_k_patches, 5)["logits"].clone()
    model.train()

    def run(seed):
        torch.manual_seed(seed)
        model.zero_grad(set_to_none=True)
        _, loss = putils.forward_backward(model, batch, 5, cfg.top_k_patches, "survival")
        return float(loss.detach()), {n: p_.grad.clone() for n, p_ in model.named_parameters() if p_.grad is not None}

    l1, g1 = run(7)
    l2, g2 = run(7)
    l3, g3 = run(8)
    assert l1 == l2 and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert l1 != l3 and np.isfinite(l3) and all(torch.isfinite(v).all() for v in g3.values())
    for proc in model.procs:
        proc.config.dropout = 0.0
    l0, _ = run(7)
    assert abs(l0 - l1) > 1e-6 and abs(l0 - l1) < 0.5 * abs(l0)                             # dropout perturbs, does not destroy
    model.eval()
    with torch.no_grad():
        assert torch.equal(putils.recurse(model, batch["slide"], cfg.top_k_patches, 5)["logits"], ev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    for proc in model.procs:
        proc.config.dropout = 0.05
    model.train()
    torch.manual_seed(0)
    losses = [float(putils.train_step(model, opt, batch, 5, cfg.top_k_patches)) for _ in range(3)]
    assert all(np.isfinite(l) for l in losses)


@pytest.mark.parametrize("over", [{}, {"lstm": False}])
def test_training_steps_do_not_leak_device_memory(dev, over):
    """The activations saved for a step's backward die with the step: device memory after step 9 is what it was after step 3 (a
    ctx -> saved dict -> returned tensor -> grad_fn -> ctx cycle once kept every level's activations alive forever: one step's worth
    per step), and a forward whose backward never runs is freed once its outputs go out of scope."""
    import gc
    from paths_amd import utils as putils
    cfg, model, params, slides, batch = _train_setup(dev, top_k=16, base=(6, 7), n_slides=3, cfg_over={"model_config": dict(over)} if over else None)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)

    def steps(n):
        for _ in range(n):
            putils.train_step(model, opt, batch, 5, cfg.top_k_patches)
        torch.cuda.synchronize()
        gc.collect()
        return torch.cuda.memory_allocated()

    gc.collect()
    m3 = steps(3)
    m9 = steps(6)
    out = putils.recurse_train(model, batch["slide"], cfg.top_k_patches, 5)
    held = torch.cuda.memory_allocated()
    del out
    gc.collect()
    one_step = held - m9                 # what one step's saved activations occupy
    assert one_step > (8 << 20)
    assert m9 - m3 < one_step // 8, (m3, m9, one_step)          # six more steps: nothing like a step's activations was kept
    assert torch.cuda.memory_allocated() - m9 < one_step // 8


def test_epoch_loop_matches_reference_g10(dev, tmp_path):
    """paths_amd.train.train_loop against the reference's own epoch loop (train.py:31-116, fixture G10 captured by
    tools/make_goldens.py: DataLoader shuffle order, AdamW + ExponentialLR, per-epoch train / validation losses, early-stopping
    save + reload, final test evaluation) on the same synthetic slides, weights and seeds."""
    import os, pickle
    from paths_amd import synthetic as syn
    from paths_amd.config import Config
    from paths_amd import train as ptrain
    from tests.conftest import load_golden
    g, info = load_golden("g10_epoch_loop_6x6_top8")
    cfg = Config.load(os.path.join(os.path.dirname(__file__), "golden", "sample"), test_mode=True)
    cfg.model_config.dropout = 0.0
    cfg.num_levels, cfg.top_k_patches, cfg.batch_size = 3, [info["top_k"]] * 2, [info["batch_size"]] * 3
    cfg.num_epochs, cfg.lr, cfg.early_stopping, cfg.eval_epochs, cfg.min_epochs = info["num_epochs"], info["lr"], True, 1, 0
    cfg.lr_decay_per_epoch = info["lr_decay_per_epoch"]
    model = cfg.get_model()
    sd = syn.make_state_dict(info["wseed"], {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev)
    ds = ptrain.synthetic_dataset(info["n_slides"], tuple(info["base_shape"]), 3, dev, seed=info["dseed"])
    order = []
    orig = ptrain.epoch_permutation

    def spy(n, shuffle):
        perm = orig(n, shuffle)
        if shuffle:
            order.extend(info["train_ids"][i] for i in perm)
        return perm

    ptrain.epoch_permutation = spy
    try:
        torch.manual_seed(info["seed"])
        logs = []
        stats = ptrain.train_loop(model, [ds[i] for i in info["train_ids"]], [ds[i] for i in info["val_ids"]],
                                  [ds[i] for i in info["test_ids"]], cfg, str(tmp_path), log=logs.append)
    finally:
        ptrain.epoch_permutation = orig
    assert order == g["order"].tolist()                                                    # DataLoader(shuffle=True) order, 3 epochs
    np.testing.assert_allclose([stats["train_loss"][e] for e in (1, 2, 3)], g["train_loss"], atol=3e-5, rtol=0)
    np.testing.assert_allclose([stats["val_loss"][e] for e in (1, 2, 3)], g["val_loss"], atol=3e-5, rtol=0)
    np.testing.assert_allclose([stats["val_c-index"][e] for e in (1, 2, 3)], g["val_cindex"], atol=1e-12, rtol=0)
    np.testing.assert_allclose([stats["train_c-index"][e] for e in (1, 2, 3)], g["train_cindex"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(stats["test"]["test_loss"], float(g["test_loss"]), atol=3e-5, rtol=0)
    saved = pickle.load(open(tmp_path / "train_stats.pkl", "rb"))
    assert saved["epoch"] == info["epoch_saved"] and sorted(saved.keys()) >= sorted(info["stats_keys"])
    # final weights = the early-stopping checkpoint re-loaded after the last epoch (reference train.py:96-98)
    for k, v in model.state_dict().items():
        ref = g["digest." + k]
        got = np.asarray([float(v.double().sum()), float(v.double().abs().sum())])
        # (Adam's first steps move every element by ~lr whatever its gradient's size, so elements whose gradient is pure rounding
        # noise - e.g. the key bias of in_proj, whose exact gradient is 0 - step in implementation-dependent directions: a few
        # times lr = 2e-4 per tensor (measured on in_proj_bias: 2.3e-3 with the attention backward on three bf16 planes, 2.5e-3 on two -
        # which noise the 128 zero-gradient key-bias elements see depends on the operand split).  The bar still separates the epoch-1
        # checkpoint from the epoch-3 weights by orders of magnitude)
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5 * ref[1] + 4e-3, err_msg=k)
