"""Integrated gradients and SmoothGrad along the frozen path on the GPU (paths_amd/saliency.py, csrc/path_rows.hip): the two
row kernels against their float64 restatement (tests/path_ref.py), the frozen pass against the free pass, and both methods against
the oracle run along its own recorded path."""
import gc

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import path_ref as R
from tests import saliency_ref as S
from tests.test_cpu_path_attributions import IG_STEPS, KEYS
from tests.test_gpu_backward import rel_err
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)
from tests.test_gpu_saliency import _setup

pytestmark = pytest.mark.gpu

U = S.U
B_, C_, N_ = 2, 3, 37
NUMS = ([0, 37], [19, 1])


def _rows(g, B, N, ld, num_ims, binades=True):
    """[B,N,ld] rows over 16 binades, NaN on padded rows (they must not be read)."""
    t = torch.randn(B, N, ld, generator=g)
    if binades:
        t = t * torch.exp2(torch.randint(-12, 4, (B, N, 1), generator=g).float())
    valid = torch.arange(N)[None, :] < torch.as_tensor(num_ims)[:, None]
    t[~valid] = float("nan")
    return t, valid


def _key64(lo, hi):
    return (hi << 32) | lo


def _keys_tensor(keys, dev):
    return torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)).to(dev)


# ------------------------------------------------------------------------------------------------
# 1. paths_path_points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_ims", NUMS)
@pytest.mark.parametrize("D", [128, 384])
def test_path_points_kernel_vs_float64(dev, D, num_ims):
    from paths_amd.saliency import path_points
    g = torch.Generator().manual_seed(D + num_ims[0])
    ldx = D + 132
    xs, valid = _rows(g, B_, N_, ldx, num_ims)
    xd = xs.to(dev)[..., :D]                                              # a strided view
    x64 = torch.nan_to_num(xs[..., :D]).double().numpy()
    nd = torch.tensor(num_ims, device=dev)
    base = torch.randn(D, generator=g)
    alpha = torch.tensor([0.0, 0.3, 1.0]) + torch.tensor([0.0, 1e-3, 0.0]) * torch.rand(3, generator=g)
    zero = torch.zeros(C_, device=dev)
    keys = [_key64(lo, hi) for lo, hi in KEYS]
    kd = _keys_tensor(keys, dev)
    pad = ~valid.numpy()

    # noise-free: one rounding for t, one for the fma, slack for second order
    out = path_points(xd, base.to(dev), alpha.to(dev), zero, None, nd).cpu()
    ref, det, _ = R.path_points(x64, base.double().numpy(), alpha.double().numpy(), [0.0] * C_, None, num_ims)
    assert out.shape == (C_ * B_, N_, D)
    err = np.abs(out.double().numpy() - ref)
    print(f"D={D} {num_ims}: noise-free max err / (u scale) = {np.max(err / np.maximum(det, 1e-300)) / U:.3g}")
    assert (err <= 3 * U * det).all()
    for c in range(C_):
        assert not out[c * B_:(c + 1) * B_].numpy()[pad].view(np.uint32).any()            # padded rows: bitwise +0
    # the identity: alpha = 1, sigma = 0, base = NULL returns x bit for bit
    one = torch.ones(1, device=dev)
    ident = path_points(xd, None, one, zero[:1], None, nd).cpu()
    assert torch.equal(ident[valid], xs[..., :D][valid]) and not ident.numpy()[pad].view(np.uint32).any()

    # the draws: rows of ones (rms = 1 exactly), alpha = 0, sigma = 1 -> z
    ones = torch.ones((B_, N_, D), device=dev)
    sig1 = torch.ones(C_, device=dev)
    z = path_points(ones, None, zero, sig1, kd, nd).cpu()
    zref, _, _ = R.path_points(np.ones((B_, N_, D)), None, [0.0] * C_, [1.0] * C_, keys, num_ims)
    zerr = np.abs(z.double().numpy() - zref)
    print(f"D={D} {num_ims}: max |z - ref| = {zerr.max():.3g}, max |z| = {np.abs(zref).max():.3g}")
    assert (zerr <= 1e-5).all() and np.abs(zref).max() > 3.0
    z2 = path_points(ones, None, zero, sig1, kd, nd).cpu()
    assert torch.equal(z, z2)                                              # bit-reproducible
    for c in range(C_):                                                    # ... in any chunking
        z1 = path_points(ones, None, zero[:1], sig1[:1], kd[c * B_:(c + 1) * B_], nd).cpu()
        assert torch.equal(z1, z[c * B_:(c + 1) * B_])
    # the general rms: rms z within gamma_(D+2) relative (+ the draw's own 1e-5) of float64
    nz = path_points(xd, None, zero, sig1, kd, nd).cpu()
    nref, _, rms = R.path_points(x64, None, [0.0] * C_, [1.0] * C_, keys, num_ims)
    bound = S.gamma(D + 2) * np.abs(nref) + 1e-5 * np.tile(rms, (C_, 1))[..., None]
    assert (np.abs(nz.double().numpy() - nref) <= bound).all()
    assert not nz.numpy()[np.tile(pad, (C_, 1))].view(np.uint32).any()


# ------------------------------------------------------------------------------------------------
# 2. paths_path_accumulate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_ims", NUMS)
@pytest.mark.parametrize("D", [128, 384])
def test_path_accumulate_kernel_vs_float64(dev, D, num_ims):
    from paths_amd.saliency import path_accumulate
    g = torch.Generator().manual_seed(7 * D + num_ims[0])
    Sn = 2 * C_
    xs, valid = _rows(g, B_, N_, D + 8, num_ims)
    dxs = [_rows(g, C_ * B_, N_, D + 132, num_ims * C_)[0] for _ in range(2)]
    base = torch.randn(D, generator=g)
    w = torch.randn(Sn, generator=g)
    nd = torch.tensor(num_ims, device=dev)
    xd, bd, wd = xs.to(dev)[..., :D], base.to(dev), w.to(dev)
    dxd = [t.to(dev)[..., :D] for t in dxs]
    pad = ~valid.numpy()

    def run():
        gxi, sq = torch.full((B_, N_), 7.0, device=dev), torch.full((B_, N_), 7.0, device=dev)
        adx = torch.full((B_, N_, D), 7.0, device=dev)
        path_accumulate(dxd[0], xd, bd, wd[:C_], nd, True, gxi, sq, adx)
        after_init = (gxi.cpu().clone(), sq.cpu().clone(), adx.cpu().clone())
        path_accumulate(dxd[1], xd, bd, wd[C_:], nd, False, gxi, sq, adx)
        return after_init, (gxi.cpu(), sq.cpu(), adx.cpu())

    first, (gxi, sq, adx) = run()
    _, again = run()
    assert all(torch.equal(a, b) for a, b in zip((gxi, sq, adx), again))                 # bit-reproducible
    for t in first + (gxi, sq, adx):
        assert not t.numpy()[pad].view(np.uint32).any()                                   # padded rows: zero after init
    x64 = torch.nan_to_num(xs[..., :D]).double().numpy()
    dx64 = np.concatenate([torch.nan_to_num(t[..., :D]).double().numpy() for t in dxs])
    rg, rq, rdx, ag, aq = R.path_accumulate(dx64, x64, base.double().numpy(), w.double().numpy(), num_ims)
    eg, eq = np.abs(gxi.double().numpy() - rg), np.abs(sq.double().numpy() - rq)
    gam = S.gamma(D + Sn + 3)
    ok = ~pad
    if ok.any():
        print(f"D={D} {num_ims}: acc_gxi err/bound {np.max(eg[ok] / (gam * ag[ok])):.3g}  acc_sq err/bound {np.max(eq[ok] / (gam * aq[ok])):.3g}")
    assert (eg <= gam * ag).all() and (eq <= gam * aq).all()
    absdx = (np.abs(w.double().numpy())[:, None, None, None] * np.abs(dx64.reshape(Sn, B_, N_, D))).sum(0) * valid.numpy()[..., None]
    assert (np.abs(adx.double().numpy() - rdx) <= S.gamma(Sn + 1) * absdx).all()
    # without init padded rows are not touched, valid rows continue from what the buffers hold; acc_dx is optional
    g2, q2 = torch.full((B_, N_), 7.0, device=dev), torch.full((B_, N_), 7.0, device=dev)
    path_accumulate(dxd[0], xd, None, wd[:C_], nd, False, g2, q2, None)
    assert bool((g2.cpu()[~valid] == 7.0).all()) and bool((q2.cpu()[~valid] == 7.0).all())
    r0 = R.path_accumulate(dx64[:C_ * B_], x64, None, w[:C_].double().numpy(), num_ims)
    assert (np.abs(g2.double().cpu().numpy() - 7.0 - r0[0])[ok] <= (gam * (r0[3] + 7.0))[ok]).all()


# ------------------------------------------------------------------------------------------------
# the small setting and its oracle trace, shared
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dev):
    from oracle import paths_oracle as orc
    cfg, model, params, slides, ocfg = _setup(dev)
    grids = [orc.LazyGrids(s.synthetic_spec) for s in slides]
    otrace = []
    with torch.no_grad():
        orc.inference_end2end(params, ocfg, grids, None, otrace)
    return dict(cfg=cfg, model=model, params=params, slides=slides, ocfg=ocfg, grids=grids, otrace=otrace, rows=R.recorded_rows(grids, otrace))


def _valid_rows(t, num):
    return torch.cat([t[b, :int(num[b])] for b in range(len(num))])


def _reference_ig(st, target, alphas, weights, base):
    """Float64 quadrature over the oracle's fp32 gradients along its own path.  Per level: attributions [B,N], mean gradient
    [B,N,D]; F(X), F(baseline)."""
    rows = st["rows"]
    bs = torch.zeros(rows[0].shape[-1], dtype=torch.float64) if base is None else base.double()
    fp = lambda pts: R.frozen_path(st["params"], st["ocfg"], st["grids"], st["otrace"], pts, target)
    valid = [(torch.arange(x.shape[1])[None, :] < rec["num_ims"][:, None])[..., None] for x, rec in zip(rows, st["otrace"])]
    point = lambda al: [((bs + al * (x.double() - bs)) * v).float() for x, v in zip(rows, valid)]
    f1, f0 = fp(point(1.0))["target"].double(), fp(point(0.0))["target"].double()
    gbar = [torch.zeros(x.shape, dtype=torch.float64) for x in rows]
    for al, wt in zip(alphas, weights):
        for acc, gl in zip(gbar, fp(point(float(al)))["grads"]):
            acc += float(wt) * gl.double()
    attr = [(gb * (x.double() - bs) * v).sum(-1) for gb, x, v in zip(gbar, rows, valid)]
    return attr, gbar, f1, f0


def _check_level_attributions(got, ref, gnorm, xnorm, num, what):
    """The metric and bar _check_against_oracle applies to grad_x_input: 2e-3 of the Cauchy-Schwarz scale || (||g_r|| ||x_r||)_r ||."""
    scale = float(_valid_rows(gnorm * xnorm, num).norm())
    assert scale > 0, f"{what}: a vacuous check"
    e = float(_valid_rows(got.double() - ref, num).norm()) / scale
    print(f"{what}: {e:.3g} of the Cauchy-Schwarz scale")
    assert e <= 2e-3, (what, e)


# ------------------------------------------------------------------------------------------------
# 3. the frozen path equals the free pass
# ------------------------------------------------------------------------------------------------
def test_frozen_path_equals_the_free_pass(dev, small):
    from paths_amd import utils as putils
    model, slides, keep = small["model"], small["slides"], small["cfg"].top_k_patches
    with torch.no_grad():
        t1, t2 = [], []
        putils.recurse_train(model, slides, keep, 5)          # the weight images are packed once per model: not part of either list
        with H.spy_calls() as free_calls:
            o1 = putils.recurse_train(model, slides, keep, 5, trace=t1)
        path = [(rec["keep_idx"], rec["keep_count"]) for rec in t1[:-1]]
        with H.spy_calls() as calls:
            o2 = putils.recurse_train(model, slides, keep, 5, trace=t2, path=path, points=None)
    assert int(o1["status"].item()) == 0 and int(o2["status"].item()) == 0
    assert free_calls.count("paths_topk") == 4 and "paths_topk" not in calls
    assert [c for c in free_calls if c != "paths_topk"] == calls
    assert torch.equal(o1["logits"], o2["logits"])
    for a, b in zip(t1, t2):
        assert torch.equal(a["num_ims"], b["num_ims"]) and torch.equal(a["locs"], b["locs"]) and torch.equal(a["logits"], b["logits"])
        assert torch.equal(a["fts"], b["fts"])
    # the identity hook changes nothing either; a path of the wrong shape is refused
    with torch.no_grad():
        o3 = putils.recurse_train(model, slides, keep, 5, path=path, points=lambda level, fts, num_ims: fts.clone())
    assert torch.equal(o1["logits"], o3["logits"])
    with pytest.raises(ValueError, match="path"):
        putils.recurse_train(model, slides, keep, 5, path=[(ki[:, :-1].contiguous(), kc) for ki, kc in path])


# ------------------------------------------------------------------------------------------------
# 4. integrated gradients against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["risk", "logit:1", "baseline-midpoint"])
def test_integrated_gradients_vs_oracle(dev, small, variant):
    from paths_amd.saliency import integrated_gradients, quadrature
    st = small
    target = "risk" if variant == "baseline-midpoint" else variant
    rule = "midpoint" if variant == "baseline-midpoint" else "gausslegendre"
    base = torch.randn(1024, generator=torch.Generator().manual_seed(5)) * 0.2 if variant == "baseline-midpoint" else None
    out, trace = integrated_gradients(st["model"], st["slides"], st["cfg"].top_k_patches, 5, target=target, steps=IG_STEPS,
                                      baseline=base.to(dev) if base is not None else None, rule=rule, keep_gradients=True)
    assert int(out["status"].item()) == 0 and all("fts" not in rec and "grad_x_input" in rec for rec in trace)
    attr, gbar, f1, f0 = _reference_ig(st, target, *quadrature(rule, IG_STEPS), base)
    assert rel_err(out["target"].cpu(), f1.float()) < 1e-4 and rel_err(out["target_baseline"].cpu(), f0.float()) < 1e-4
    got = R.to_oracle_order(trace, st["otrace"], "integrated_gradients")
    got_g = R.to_oracle_order(trace, st["otrace"], "integrated_gradient")
    bs = torch.zeros(1024, dtype=torch.float64) if base is None else base.double()
    for l, orec in enumerate(st["otrace"]):
        num = orec["num_ims"]
        ig = trace[l]["integrated_gradients"]
        assert float(ig[torch.arange(ig.shape[1], device=dev)[None, :] >= trace[l]["num_ims"][:, None]].abs().sum()) == 0.0
        _check_level_attributions(got[l], attr[l], gbar[l].norm(dim=-1), (st["rows"][l].double() - bs).norm(dim=-1), num,
                                  f"{variant} level {l} integrated_gradients")
        e = rel_err(_valid_rows(got_g[l], num), _valid_rows(gbar[l], num))
        assert e < 2e-3, (l, e)
    ref_total = sum(a.sum(1) for a in attr)
    ref_gap = (ref_total - (f1 - f0)).abs()
    bound = ref_gap + 2e-3 * sum(a.abs().sum(1) for a in attr)
    print(f"{variant}: completeness gap {out['completeness_gap'].tolist()}  reference gap {ref_gap.tolist()}  bound {bound.tolist()}  "
          f"F(X) - F(base) {(f1 - f0).tolist()}")
    assert bool((out["completeness_gap"].cpu().double().abs() <= bound).all())
    total = sum(rec["integrated_gradients"].double().sum(1) for rec in trace).cpu()
    assert torch.allclose(out["completeness_gap"].cpu().double(), total - (out["target"].cpu().double() - out["target_baseline"].cpu().double()),
                          rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------
# 5. chunking and batch composition
# ------------------------------------------------------------------------------------------------
def test_integrated_gradients_chunking_and_batch_composition(dev, small):
    """chunk = 1 and chunk = 4 agree within 1e-5 relative per level, and a batch of three equals each slide alone within the same
    bar (the bar of test_gpu_saliency.test_slides_do_not_interact for batch composition)."""
    from paths_amd.saliency import integrated_gradients
    model, slides, keep = small["model"], small["slides"], small["cfg"].top_k_patches
    with H.spy_calls() as calls:
        o1, t1 = integrated_gradients(model, slides, keep, 5, steps=IG_STEPS, chunk=1)
    assert calls.count("paths_path_accumulate") == 5 * IG_STEPS and calls.count("paths_path_points") == 5 * (IG_STEPS + 1)
    assert calls.count("paths_saliency_rows") == 5 and calls.count("paths_topk") == 4
    with H.spy_calls() as calls:
        o4, t4 = integrated_gradients(model, slides, keep, 5, steps=IG_STEPS, chunk=4)
    assert calls.count("paths_path_accumulate") == 5 * IG_STEPS // 4
    o3, t3 = integrated_gradients(model, slides, keep, 5, steps=IG_STEPS, chunk=3)          # a short last chunk
    for l, (a, b, c) in enumerate(zip(t1, t4, t3)):
        assert rel_err(a["integrated_gradients"], b["integrated_gradients"]) < 1e-5, l
        assert rel_err(a["integrated_gradients"], c["integrated_gradients"]) < 1e-5, l
    assert rel_err(o1["target_baseline"], o4["target_baseline"]) < 1e-5
    for b, s in enumerate(slides):
        oa, ta = integrated_gradients(model, [s], keep, 5, steps=IG_STEPS)
        assert rel_err(oa["target_baseline"], o4["target_baseline"][b:b + 1]) < 1e-5
        for l, (ra, rb) in enumerate(zip(ta, t4)):
            n = int(ra["num_ims"][0])
            assert n == int(rb["num_ims"][b]) and torch.equal(ra["locs"][0, :n], rb["locs"][b, :n])
            e = rel_err(ra["integrated_gradients"][0, :n], rb["integrated_gradients"][b, :n])
            assert e < 1e-5, (b, l, e)


# ------------------------------------------------------------------------------------------------
# 6. SmoothGrad against the oracle
# ------------------------------------------------------------------------------------------------
def test_smooth_grad_vs_oracle(dev, small):
    from paths_amd.saliency import noise_key, smooth_grad
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    Sn = 4
    out, trace = smooth_grad(model, slides, keep, 5, samples=Sn, sigma=0.15, seed=11, keep_points=True, keep_gradients=True)
    pts = R.to_oracle_order(trace, st["otrace"], "points")
    assert all(p.shape == (Sn,) + x.shape for p, x in zip(pts, st["rows"]))
    refs = [R.frozen_path(st["params"], st["ocfg"], st["grids"], st["otrace"], [p[s] for p in pts], "risk")["grads"] for s in range(Sn)]
    got_gxi = R.to_oracle_order(trace, st["otrace"], "smooth_grad_x_input")
    got_sq = R.to_oracle_order(trace, st["otrace"], "smooth_grad_sq")
    got_g = R.to_oracle_order(trace, st["otrace"], "smooth_grad")
    for l, orec in enumerate(st["otrace"]):
        num, x = orec["num_ims"], st["rows"][l].double()
        gs = torch.stack([refs[s][l].double() for s in range(Sn)])
        ref_gxi = (gs * x[None]).sum(-1).mean(0)
        ref_sq = (gs * gs).sum(-1).mean(0)
        _check_level_attributions(got_gxi[l], ref_gxi, gs.norm(dim=-1).mean(0), x.norm(dim=-1), num, f"level {l} smooth_grad_x_input")
        e = rel_err(_valid_rows(got_sq[l].double().sqrt(), num), _valid_rows(ref_sq.sqrt(), num))
        print(f"level {l}: sqrt(smooth_grad_sq) rel err {e:.3g}")
        assert e < 2e-3, (l, e)
        assert rel_err(_valid_rows(got_g[l], num), _valid_rows(gs.mean(0), num)) < 2e-3
    # the exported points are the restated generator's under noise_key (level 2, every sample and slide)
    l = 2
    keys = [noise_key(11, l, s, b) for s in range(Sn) for b in range(3)]
    num = trace[l]["num_ims"].cpu().numpy()
    cells = torch.div(trace[l]["locs"].cpu(), 256, rounding_mode="floor")
    cells = cells * (torch.arange(cells.shape[1])[None, :] < trace[l]["num_ims"].cpu()[:, None])[..., None]      # (padding: any cell)
    x = np.stack([st["grids"][b].rows(l, cells[b, :, 0], cells[b, :, 1]).numpy() for b in range(3)])
    want, _, rms = R.path_points(x, None, [1.0] * Sn, [np.float32(0.15)] * Sn, keys, num)
    have = trace[l]["points"].reshape(Sn * 3, *x.shape[1:]).double().cpu().numpy()
    tol = 2 * U * np.abs(want) + 0.15 * np.tile(rms, (Sn, 1))[..., None] * (1e-5 + S.gamma(1024 + 2) * 5.89)
    assert (np.abs(have - want) <= tol).all()
    # same seed: the same bits; another seed: other noise; sigma = 0: the path pass's own gradient x input
    out2, trace2 = smooth_grad(model, slides, keep, 5, samples=Sn, sigma=0.15, seed=11)
    assert all(torch.equal(a["smooth_grad_x_input"], b["smooth_grad_x_input"]) and torch.equal(a["smooth_grad_sq"], b["smooth_grad_sq"])
               for a, b in zip(trace, trace2))
    assert all("points" not in rec and "smooth_grad" not in rec for rec in trace2)
    out3, trace3 = smooth_grad(model, slides, keep, 5, samples=Sn, sigma=0.15, seed=12)
    assert not any(torch.equal(a["smooth_grad_x_input"], b["smooth_grad_x_input"]) for a, b in zip(trace, trace3))
    with H.spy_calls() as calls:
        out0, trace0 = smooth_grad(model, slides, keep, 5, samples=2, sigma=0.0)
    assert calls.count("paths_path_points") == 5                           # default chunk max(1, 8 // 3) = 2: one frozen pass
    for l, rec in enumerate(trace0):
        assert rel_err(rec["smooth_grad_x_input"], rec["grad_x_input"]) < 1e-5, l
        assert rel_err(rec["smooth_grad_sq"].sqrt(), rec["grad_norm"]) < 1e-5, l


# ------------------------------------------------------------------------------------------------
# 7. zero-children slides, mode and gradients, grid dtypes and host slides
# ------------------------------------------------------------------------------------------------
def test_zero_children_slides_take_the_careful_path(dev):
    """The slides of test_gpu_saliency.test_input_gradients_on_zero_children_slides: both calls repeat the path pass on the careful
    path, run their points careful too, and meet the oracle along ITS recorded path (fallback rows carry no parent state)."""
    from oracle import paths_oracle as orc
    from paths_amd.saliency import integrated_gradients, quadrature, smooth_grad
    cfg, model, params, slides, ocfg = _setup(dev, None, wseed=9, dseed=57, top_k=2, base=(4, 4), n_slides=4, p_bg=0.93)
    grids = [orc.LazyGrids(s.synthetic_spec) for s in slides]
    otrace = []
    with torch.no_grad():
        orc.inference_end2end(params, ocfg, grids, None, otrace)
    assert any(any(rec["fallback"]) for rec in otrace)
    st = dict(params=params, ocfg=ocfg, grids=grids, otrace=otrace, rows=R.recorded_rows(grids, otrace))
    model.train()
    with H.spy_calls() as calls:
        out, trace = integrated_gradients(model, slides, cfg.top_k_patches, 5, steps=IG_STEPS)
    assert model.training and "paths_fallback_all_cells" in calls and calls.count("paths_saliency_rows") == 10
    attr, gbar, f1, f0 = _reference_ig(st, "risk", *quadrature("gausslegendre", IG_STEPS), None)
    assert rel_err(out["target"].cpu(), f1.float()) < 1e-4 and rel_err(out["target_baseline"].cpu(), f0.float()) < 1e-4
    got = R.to_oracle_order(trace, otrace, "integrated_gradients")
    for l, orec in enumerate(otrace):
        _check_level_attributions(got[l], attr[l], gbar[l].norm(dim=-1), st["rows"][l].double().norm(dim=-1), orec["num_ims"],
                                  f"zero-children level {l} integrated_gradients")
    out, trace = smooth_grad(model, slides, cfg.top_k_patches, 5, samples=2, sigma=0.15, keep_points=True)
    pts = R.to_oracle_order(trace, otrace, "points")
    refs = [R.frozen_path(params, ocfg, grids, otrace, [p[s] for p in pts], "risk")["grads"] for s in range(2)]
    got = R.to_oracle_order(trace, otrace, "smooth_grad_x_input")
    for l, orec in enumerate(otrace):
        gs, x = torch.stack([refs[s][l].double() for s in range(2)]), st["rows"][l].double()
        _check_level_attributions(got[l], (gs * x[None]).sum(-1).mean(0), gs.norm(dim=-1).mean(0), x.norm(dim=-1), orec["num_ims"],
                                  f"zero-children level {l} smooth_grad_x_input")


def test_mode_and_parameter_gradients_are_untouched(dev):
    from paths_amd.saliency import integrated_gradients, smooth_grad
    cfg, model, params, slides, ocfg = _setup(dev)
    calls = (lambda: integrated_gradients(model, slides, cfg.top_k_patches, 5, steps=2),
             lambda: smooth_grad(model, slides, cfg.top_k_patches, 5, samples=2))
    model.train()
    for call in calls:
        call()
        assert all(p.grad is None for p in model.parameters()) and model.training and all(m.training for m in model.modules())
    g = torch.Generator().manual_seed(1)
    preset = {}
    for i, (n, p) in enumerate(model.named_parameters()):
        if i % 3 == 0:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
            preset[n] = p.grad.clone()
    model.eval()
    for call in calls:
        with torch.no_grad():                                    # (the calls enable gradients for themselves)
            out, trace = call()
        assert not model.training and float(trace[0]["grad_norm"].sum()) > 0
        for n, p in model.named_parameters():
            assert (torch.equal(p.grad, preset[n]) if n in preset else p.grad is None), n
    assert all(p.requires_grad for p in model.parameters())
    with H.spy_calls() as spied:
        calls[0]()
    assert not [c for c in spied if c in ("paths_gemm_tn_x6", "paths_gemm_tn_f32", "paths_colsum_f32", "paths_flush_reductions")]


def test_fp16_grids_and_host_slides_give_the_fp32_resident_result(dev):
    """Features that fp16 represents exactly: the training path gathers fp32 copies, so fp16 grids and pinned host grids give the
    fp32 resident result of the same values (1e-5 relative)."""
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    from paths_amd.saliency import integrated_gradients, smooth_grad
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[16] * 4)
    host16 = [HostSlide.synthetic(14, sid, (6, 7), device=dev, dtype=torch.float16) for sid in range(3)]
    dev16 = [s.to_device() for s in host16]
    dev32 = [DeviceSlide([g.float() for g in s.grids], patch_size=s.patch_size) for s in dev16]
    run = lambda sl: (integrated_gradients(model, sl, cfg.top_k_patches, 5, steps=3)[1], smooth_grad(model, sl, cfg.top_k_patches, 5, samples=3)[1])
    ref = run(dev32)
    assert float(ref[0][0]["integrated_gradients"].abs().sum()) > 0
    for name, slides in (("fp16 resident", dev16), ("fp16 host", host16)):
        got = run(slides)
        for key, tr, rf in (("integrated_gradients", got[0], ref[0]), ("smooth_grad_x_input", got[1], ref[1]), ("smooth_grad_sq", got[1], ref[1])):
            for l, (a, b) in enumerate(zip(tr, rf)):
                assert torch.equal(a["num_ims"], b["num_ims"]) and rel_err(a[key], b[key]) < 1e-5, (name, key, l)
    del host16
    gc.collect()
    torch.cuda.synchronize()
    empty = getattr(torch._C, "_host_emptyCache", None)
    if empty is not None:
        empty()
