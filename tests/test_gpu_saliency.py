"""Gradient x input attributions on the GPU (paths_amd/saliency.py): the row kernel against float64 (tests/saliency_ref.py), the feature
gradient of one level against float64 autograd over the oracle's formulas, and the whole pass against torch autograd through the
oracle over dense grids that require a gradient."""
import gc
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H
from tests import saliency_ref as S
from tests.test_gpu_backward import make_level_inputs, rel_err
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16 = torch.float16
WEIGHT_GRAD_ENTRIES = ("paths_gemm_tn_x6", "paths_gemm_tn_f32", "paths_colsum_f32")


# ------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 384, 1024])
def test_saliency_rows_kernel_vs_float64(dev, D):
    """Ragged num_ims incl. 0 and N, strided rows, magnitudes over 16 binades.  Bounds (derived, u = 2^-24): a D-term fp32 dot product
    in ANY order is within gamma_D sum|dx x| of the exact one; the sum of squares within a factor (1 +- gamma_D), so its square root -
    rounded once more - within gamma_(D+1)/2 + 2u relative.  Padded rows hold NaN: they are not read and come out as exact zeros."""
    from paths_amd import _lib
    B, N = 4, 37
    num_ims = torch.tensor([0, N, 17, 1])
    ldd, ldx = D + 8, D + 132
    g = torch.Generator().manual_seed(D)
    valid = torch.arange(N)[None, :] < num_ims[:, None]

    def rows(ld):
        t = torch.randn(B, N, ld, generator=g) * torch.exp2(torch.randint(-12, 4, (B, N, 1), generator=g).float())
        t[~valid] = float("nan")
        return t

    dxs, xs = rows(ldd), rows(ldx)
    dxd, xd, nd = dxs.to(dev), xs.to(dev), num_ims.to(dev)
    outs = []
    for _ in range(2):
        gxi = torch.full((B, N), 7.0, device=dev)
        gnorm = torch.full((B, N), 7.0, device=dev)
        _lib.call("paths_saliency_rows", dxd.data_ptr(), ldd, xd.data_ptr(), ldx, nd.data_ptr(), N, D, B, gxi.data_ptr(), gnorm.data_ptr(),
                  _lib.stream())
        outs.append((gxi.cpu(), gnorm.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])       # bit-reproducible
    gxi, gnorm = outs[0]
    dx64 = torch.nan_to_num(dxs[..., :D]).numpy()
    x64 = torch.nan_to_num(xs[..., :D]).numpy()
    rg, rn, absdot = S.saliency_rows(dx64, x64, num_ims.numpy())
    pad = ~valid.numpy()
    assert not gxi.numpy()[pad].view(np.uint32).any() and not gnorm.numpy()[pad].view(np.uint32).any()      # bitwise +0
    err = np.abs(gxi.double().numpy() - rg)
    bound = S.gamma(D) * absdot
    print(f"D={D}: gxi max err/bound = {np.max(err[~pad] / bound[~pad]):.3g}")
    assert (err <= bound).all()
    reln = np.abs(gnorm.double().numpy() - rn)[~pad] / rn[~pad]
    print(f"D={D}: gnorm max rel err = {reln.max():.3g} (bound {S.gamma(D + 1) / 2 + 2 * S.U:.3g})")
    assert (reln <= S.gamma(D + 1) / 2 + 2 * S.U).all()
    # the wrapper: contiguous views of strided storage go through with their strides
    from paths_amd.saliency import saliency_rows
    w_gxi, w_gnorm = saliency_rows(dxd[..., :D], xd[..., :D], nd)
    assert torch.equal(w_gxi.cpu(), gxi) and torch.equal(w_gnorm.cpu(), gnorm)


# ------------------------------------------------------------------------------------------------
# 2. the feature gradient of one level
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0, 2])
def test_selection_backward_feature_gradient(dev, depth):
    """dX = dG W_gates[:, :D] + dY of the LSTM cell + importance MLP + proj_in chain against float64 autograd over the oracle's formulas
    (the setup and the 2e-4 of test_gpu_backward.test_selection_chain_backward, which holds d_state_prev to it); asking for dX changes
    no other result."""
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
    with H.spy_calls() as off:
        grads0, dprev0 = bw.selection_backward(mc, lp, vp, sv, G_tok.to(dev), G_state.to(dev))
    with H.spy_calls() as on:
        grads, dprev, dx = bw.selection_backward(mc, lp, vp, sv, G_tok.to(dev), G_state.to(dev), want_dx=True)
    assert dx.shape == (B, N, 1024) and dx.dtype == torch.float32
    assert grads.keys() == grads0.keys() and all(torch.equal(grads[k], grads0[k]) for k in grads)
    assert (dprev is None and dprev0 is None) or torch.equal(dprev, dprev0)
    nt = lambda calls: sum(c.startswith("paths_gemm_nt_") for c in calls)
    assert nt(on) == nt(off) + 1 and "paths_saliency_rows" not in on

    p = {k: v.double() for k, v in params.items()}
    X = fts.double().requires_grad_(True)
    pre = f"procs.{depth}."
    if depth == 0:
        h0, c0 = torch.zeros(B, N, 1024, dtype=torch.float64), torch.zeros(B, N, 256, dtype=torch.float64)
    else:
        h0, c0 = state.double()[..., :1024], state.double()[..., 1024:]
    hs, cs = orc.lstm_cell(p, X, h0, c0)
    Y = X + hs
    state_out = torch.cat((hs, cs), -1)
    hid = torch.relu(F.linear(Y, p[pre + "importance_mlp.0.weight"], p[pre + "importance_mlp.0.bias"]))
    alpha = torch.sigmoid(F.linear(hid, p[pre + "importance_mlp.2.weight"], p[pre + "importance_mlp.2.bias"]))[..., 0] * valid
    gk = pre + "global_agg."
    tok = F.linear(Y * alpha[..., None], p[gk + "proj_in.weight"], p[gk + "proj_in.bias"])      # (+ PE: no gradient to X)
    ((tok * G_tok[:, 1:].double()).sum() + (state_out * G_state.double()).sum()).backward()
    e = rel_err(dx[valid.to(dev)], X.grad[valid])
    print(f"depth {depth}: dX rel err {e:.3g}")
    assert e < 2e-4


# ------------------------------------------------------------------------------------------------
# 3.-5. the whole pass against the oracle
# ------------------------------------------------------------------------------------------------
def _oracle_targets(name, logits):
    if name == "risk":
        return -torch.cumprod(1 - torch.sigmoid(logits), dim=1).sum(dim=1)
    assert name.startswith("logit:")
    return logits[:, int(name[6:])]


def _oracle_gradients(params, ocfg, specs, targets):
    """Oracle recursion over DenseGrids whose tensors require a gradient.  Returns (grids [slide][level], {target: [slide][level] grid
    gradient or None}, trace)."""
    from oracle import paths_oracle as orc
    L = ocfg.num_levels
    grids = [[torch.from_numpy(sp.grid(l)).requires_grad_(True) for l in range(L)] for sp in specs]
    otrace = []
    orc.inference_end2end(params, ocfg, [orc.DenseGrids(g) for g in grids], None, otrace)
    logits = otrace[-1]["logits"]                              # (a clone of the last level's logits: still on the graph)
    flat = [t for g in grids for t in g]
    out = {}
    for name in targets:
        gs = torch.autograd.grad(_oracle_targets(name, logits).sum(), flat, retain_graph=True, allow_unused=True)
        out[name] = [list(gs[j * L:(j + 1) * L]) for j in range(len(specs))]
    return grids, out, otrace, logits.detach()


def _check_against_oracle(trace, out, target, grids, ograds, otrace, ologits, patch_size=256, label=""):
    """Rows matched by location (identical sets required).  Per level over all slides' valid rows: grad rel_err < 2e-3 norm-wise (the
    project's recursion-gradient bar); grad_x_input within 2e-3 of || (||dX_r|| ||X_r||)_r || (Cauchy-Schwarz on every row's
    (dX_r - ref_r) . X_r); grad_norm rel_err < 2e-3."""
    assert rel_err(out["logits"], ologits) < 1e-4
    assert rel_err(out["target"], _oracle_targets(target, ologits)) < 1e-4
    assert len(trace) == len(otrace)
    B = out["logits"].shape[0]
    for l, (rec, orec) in enumerate(zip(trace, otrace)):
        num = rec["num_ims"].cpu()
        assert torch.equal(num, orec["num_ims"]), f"level {l}: num_ims"
        got_dx, ref_dx, xs, got_gxi, got_gn = [], [], [], [], []
        for b in range(B):
            n = int(num[b])
            cells = torch.div(rec["locs"][b, :n].cpu(), patch_size, rounding_mode="floor")
            ocells = torch.div(orec["locs"][b, :n], patch_size, rounding_mode="floor")
            key = lambda c: sorted(map(tuple, c.tolist()))
            assert key(cells) == key(ocells), f"level {l} slide {b}: the location sets differ"
            gr = ograds[b][l]
            ref = gr[cells[:, 0], cells[:, 1]] if gr is not None else torch.zeros((n, grids[b][l].shape[2]))
            ref_dx.append(ref.double())
            xs.append(grids[b][l].detach()[cells[:, 0], cells[:, 1]].double())
            got_dx.append(rec["grad"][b, :n].double().cpu())
            got_gxi.append(rec["grad_x_input"][b, :n].double().cpu())
            got_gn.append(rec["grad_norm"][b, :n].double().cpu())
            assert float(rec["grad_x_input"][b, n:].abs().sum()) == 0.0 and float(rec["grad_norm"][b, n:].abs().sum()) == 0.0
        got_dx, ref_dx, xs = torch.cat(got_dx), torch.cat(ref_dx), torch.cat(xs)
        got_gxi, got_gn = torch.cat(got_gxi), torch.cat(got_gn)
        assert float(ref_dx.norm()) > 0, f"level {l}: the oracle's gradient is identically zero (a vacuous check)"
        e_dx = rel_err(got_dx, ref_dx)
        ref_gxi = (ref_dx * xs).sum(1)
        scale = float((ref_dx.norm(dim=1) * xs.norm(dim=1)).norm())
        e_gxi = float((got_gxi - ref_gxi).norm()) / scale
        e_gn = rel_err(got_gn, ref_dx.norm(dim=1))
        print(f"{label} {target} level {l}: grad {e_dx:.3g}  grad_x_input {e_gxi:.3g} (of the Cauchy-Schwarz scale)  grad_norm {e_gn:.3g}")
        assert e_dx < 2e-3, (l, e_dx)
        assert e_gxi <= 2e-3, (l, e_gxi)
        assert e_gn < 2e-3, (l, e_gn)


def _setup(dev, cfg_over=None, wseed=3, dseed=14, top_k=16, base=(6, 7), n_slides=3, p_bg=0.1):
    from paths_amd.data_utils.slide import DeviceSlide
    cfg, model, params = build_model(dev, wseed, cfg_over, top_k_patches=[top_k] * 4)
    slides = [DeviceSlide.synthetic(dseed, sid, base, p_bg=p_bg, device=dev) for sid in range(n_slides)]
    ocfg = H.oracle_config(cfg_over, top_k_patches=[top_k] * 4)
    return cfg, model, params, slides, ocfg


TARGETS = ("risk", "logit:1")


@pytest.mark.parametrize("variant", ["shipped", "td192", "concat", "impnone"])
def test_input_gradients_vs_oracle_autograd(dev, variant):
    """3 synthetic slides, base (6, 7), top-16, 5 levels; the shipped geometry and trans_dim 192, slide_ctx_mode "concat",
    importance_mode "none"; targets "risk" and "logit:1"."""
    from paths_amd.saliency import input_gradients
    over = {"td192": {"model_config": {"trans_dim": 192}}, "concat": {"model_config": {"slide_ctx_mode": "concat"}},
            "impnone": {"model_config": {"importance_mode": "none"}}}.get(variant)
    cfg, model, params, slides, ocfg = _setup(dev, over)
    grids, ograds, otrace, ologits = _oracle_gradients(params, ocfg, [s.synthetic_spec for s in slides], TARGETS)
    for target in TARGETS:
        out, trace = input_gradients(model, slides, cfg.top_k_patches, 5, target=target, keep_gradients=True)
        assert int(out["status"].item()) == 0 and len(trace) == 5
        assert all("fts" not in rec and rec["grad"].shape[:2] == rec["grad_norm"].shape for rec in trace)
        assert all(("keep_idx" in rec) == (l < 4) for l, rec in enumerate(trace))
        _check_against_oracle(trace, out, target, grids, ograds[target], otrace, ologits, label=variant)
    # without keep_gradients: the same reductions, no gradient tensors; a callable target
    out2, trace2 = input_gradients(model, slides, cfg.top_k_patches, 5, target=lambda lg: lg[:, 1])
    assert all("grad" not in rec for rec in trace2)
    assert all(torch.equal(a["grad_x_input"], b["grad_x_input"]) and torch.equal(a["grad_norm"], b["grad_norm"]) for a, b in zip(trace, trace2))
    with pytest.raises(ValueError):
        input_gradients(model, slides, cfg.top_k_patches, 5, target=lambda lg: lg)
    del grids, ograds
    gc.collect()


def test_input_gradients_on_zero_children_slides(dev):
    """Slides whose kept patches have no tissue children (test_gpu_backward.test_training_on_zero_children_slides_takes_the_fallback):
    the pass repeats on the careful path and gives the oracle's gradients."""
    from paths_amd import utils as putils
    from paths_amd.saliency import input_gradients
    cfg, model, params, slides, ocfg = _setup(dev, None, wseed=9, dseed=57, top_k=2, base=(4, 4), n_slides=4, p_bg=0.93)
    model.train()
    fast = putils.recurse_train(model, slides, cfg.top_k_patches, 5)
    assert int(fast["status"].item()) & 1, "test slides should trigger the fallback"
    del fast
    grids, ograds, otrace, ologits = _oracle_gradients(params, ocfg, [s.synthetic_spec for s in slides], ("risk",))
    assert any(any(rec["fallback"]) for rec in otrace)
    with H.spy_calls() as calls:
        out, trace = input_gradients(model, slides, cfg.top_k_patches, 5, keep_gradients=True)
    assert "paths_fallback_all_cells" in calls and calls.count("paths_saliency_rows") == 10      # optimistic pass + careful re-run
    assert model.training and len(trace) == 5
    _check_against_oracle(trace, out, "risk", grids, ograds["risk"], otrace, ologits, label="zero-children")


# ------------------------------------------------------------------------------------------------
# 6.-7. batches, grid dtypes, host slides
# ------------------------------------------------------------------------------------------------
def test_slides_do_not_interact(dev):
    """A batch of 3 equals each slide alone: 1e-5 relative per level (the kernels' per-row results do not depend on the batch;
    a launch may pick another tile shape for another row count)."""
    from paths_amd.saliency import input_gradients
    cfg, model, params, slides, ocfg = _setup(dev)
    out, trace = input_gradients(model, slides, cfg.top_k_patches, 5, keep_gradients=True)
    for b, s in enumerate(slides):
        o1, t1 = input_gradients(model, [s], cfg.top_k_patches, 5, keep_gradients=True)
        assert rel_err(o1["target"], out["target"][b:b + 1]) < 1e-5
        for l, (ra, rb) in enumerate(zip(t1, trace)):
            n = int(ra["num_ims"][0])
            assert n == int(rb["num_ims"][b]) and torch.equal(ra["locs"][0, :n], rb["locs"][b, :n])
            for key in ("grad", "grad_x_input", "grad_norm"):
                e = rel_err(ra[key][0, :n], rb[key][b, :n])
                assert e < 1e-5, (b, l, key, e)


def test_fp16_grids_and_host_slides_are_bitwise_the_fp32_resident_result(dev):
    """Features that fp16 represents exactly: the training path gathers fp32 copies, so fp16 grids, pinned host grids (fp16 and fp32)
    and resident fp32 grids give the same bits."""
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    from paths_amd.saliency import input_gradients
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[16] * 4)
    host16 = [HostSlide.synthetic(14, sid, (6, 7), device=dev, dtype=F16) for sid in range(3)]
    dev16 = [s.to_device() for s in host16]
    dev32 = [DeviceSlide([g.float() for g in s.grids], patch_size=s.patch_size) for s in dev16]
    host32 = [HostSlide([g.float().pin_memory() for g in s.grids], device=dev, patch_size=s.patch_size) for s in host16]
    assert dev16[0].dtype == F16 and dev32[0].dtype == torch.float32 and host32[0].dtype == torch.float32
    ref_out, ref = input_gradients(model, dev32, cfg.top_k_patches, 5, keep_gradients=True)
    assert float(ref[0]["grad_norm"].sum()) > 0
    for name, slides in (("fp16 resident", dev16), ("fp16 host", host16), ("fp32 host", host32)):
        out, tr = input_gradients(model, slides, cfg.top_k_patches, 5, keep_gradients=True)
        assert torch.equal(out["logits"], ref_out["logits"]) and torch.equal(out["target"], ref_out["target"]), name
        for l, (a, b) in enumerate(zip(tr, ref)):
            assert torch.equal(a["num_ims"], b["num_ims"]), (name, l)
            valid = (torch.arange(a["grad"].shape[1], device=dev)[None, :] < a["num_ims"][:, None])
            assert torch.equal(a["locs"][valid], b["locs"][valid]), (name, l)
            for key in ("grad_x_input", "grad_norm"):
                assert torch.equal(a[key], b[key]), (name, l, key)
            assert torch.equal(a["grad"][valid], b["grad"][valid]), (name, l)
    del host16, host32
    gc.collect()
    torch.cuda.synchronize()
    empty = getattr(torch._C, "_host_emptyCache", None)
    if empty is not None:
        empty()


# ------------------------------------------------------------------------------------------------
# 8.-9. what the call leaves alone, and what it launches
# ------------------------------------------------------------------------------------------------
def test_parameter_gradients_and_mode_are_untouched(dev):
    from paths_amd.saliency import input_gradients
    cfg, model, params, slides, ocfg = _setup(dev)
    model.train()
    assert all(p.grad is None for p in model.parameters())
    input_gradients(model, slides, cfg.top_k_patches, 5)
    assert all(p.grad is None for p in model.parameters()) and model.training and all(m.training for m in model.modules())
    g = torch.Generator().manual_seed(1)
    preset = {}
    for i, (n, p) in enumerate(model.named_parameters()):
        if i % 3 == 0:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
            preset[n] = p.grad.clone()
    model.eval()
    with torch.no_grad():                                    # (the call enables gradients for itself)
        out, trace = input_gradients(model, slides, cfg.top_k_patches, 5, target="logit:0")
    assert not model.training and float(trace[0]["grad_norm"].sum()) > 0
    for n, p in model.named_parameters():
        if n in preset:
            assert torch.equal(p.grad, preset[n]), n
        else:
            assert p.grad is None, n
    assert all(p.requires_grad for p in model.parameters())


def test_launch_lists(dev):
    """input_gradients: one paths_saliency_rows per level and no weight-gradient entry point; a training step: no paths_saliency_rows;
    LevelFn with and without a gradient wanted for the features: the same launches but for the one dX product."""
    from paths_amd import autograd as pag, utils as putils
    from paths_amd.data_utils.slide import DeviceSlideBatch
    from paths_amd.saliency import input_gradients
    cfg, model, params, slides, ocfg = _setup(dev)
    with H.spy_calls() as calls:
        out, _ = input_gradients(model, slides, cfg.top_k_patches, 5)
    assert int(out["status"].item()) == 0
    assert calls.count("paths_saliency_rows") == 5
    assert not [c for c in calls if c in WEIGHT_GRAD_ENTRIES or c in ("paths_flush_reductions", "paths_reduce_slabs_f32")]
    assert getattr(model, "_paths_dead_zero", None) is None          # (fill_dead_grads did not run)

    labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
    batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    with H.spy_calls() as train_calls:
        loss = putils.train_step(model, opt, batch, 5, cfg.top_k_patches)
    assert math.isfinite(float(loss)) and "paths_saliency_rows" not in train_calls
    assert sum(c in WEIGHT_GRAD_ENTRIES for c in train_calls) > 50           # (the spy does see them where they run)
    model.zero_grad(set_to_none=True)

    B, N = 2, 160
    fts, locs, num_ims, _, _ = make_level_inputs(B, N, [160, 117], 0, seed=3)

    def level(want_dx):
        x = fts.to(dev).requires_grad_(want_dx)
        with H.spy_calls() as c:
            logits, ctx_slide, state_out, _ = pag.level_apply(model.procs[0], model.lstm, x, locs.to(dev), num_ims.to(dev), None, None)
            (logits.sum() + state_out.sum()).backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        return c, grads, x.grad

    level(False)                                             # (the first pass also packs the weight images)
    c_off, g_off, dx_off = level(False)
    c_on, g_on, dx_on = level(True)
    assert dx_off is None and dx_on is not None and dx_on.shape == (B, N, 1024)
    assert g_off.keys() == g_on.keys() and len(g_off) > 30 and all(torch.equal(g_off[k], g_on[k]) for k in g_off)
    nt = lambda calls: sum(c.startswith("paths_gemm_nt_") for c in calls)
    assert nt(c_on) == nt(c_off) + 1
    extra = list(c_on)
    for c in c_off:                                          # the launches without dX, in order, are a subsequence of those with it
        while extra and extra[0] != c:
            assert extra.pop(0) in ("paths_gemm_nt_f32", "paths_gemm_nt_x6", "paths_transpose_f32", "paths_x6_pack_weights_t")
        assert extra and extra.pop(0) == c
    assert all(c in ("paths_gemm_nt_f32", "paths_gemm_nt_x6", "paths_transpose_f32", "paths_x6_pack_weights_t") for c in extra)
    assert "paths_saliency_rows" not in c_on and "paths_saliency_rows" not in c_off
