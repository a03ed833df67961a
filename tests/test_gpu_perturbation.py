"""Deletion / insertion curves along the frozen path on the GPU (paths_amd/saliency.py:perturbation_curves, csrc/perturb_rows.hip;
DESIGN 15): the two kernels against their numpy restatement (tests/perturb_ref.py; integers and bit patterns, no tolerance), the
curves against the oracle run along its own recorded path, the identities between the curves, a given trace, the launch lists and
the other slide kinds."""
import gc

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import path_ref as R
from tests import perturb_ref as P
from tests.test_cpu_perturbation import NUMS, SEG, TIES
from tests.test_gpu_backward import rel_err
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)
from tests.test_gpu_path_attributions import small  # noqa: F401  (fixture)
from tests.test_gpu_saliency import _setup

pytestmark = pytest.mark.gpu

STEPS = 4
NEW = ("paths_rank_joint", "paths_path_mask_points")


# ------------------------------------------------------------------------------------------------
# 1. paths_rank_joint
# ------------------------------------------------------------------------------------------------
def _run_rank(dev, scores, seg, num_ims, level_on, ascending):
    from paths_amd.saliency import rank_joint
    tab = torch.tensor(np.stack([np.cumsum(seg), [1] * len(seg) if level_on is None else level_on]), dtype=torch.int32, device=dev)
    args = (torch.from_numpy(scores).to(dev), tab[0], tab[1], torch.as_tensor(np.asarray(num_ims), dtype=torch.int64).to(dev))
    rank, count = rank_joint(*args, ascending=ascending)
    rank2, count2 = rank_joint(*args, ascending=ascending)
    assert torch.equal(rank, rank2) and torch.equal(count, count2)                          # bit-identical repeat
    assert rank.dtype == count.dtype == torch.int32
    return rank.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("case", ["distinct", "ties", "ascending", "level-1-off"])
def test_rank_joint_kernel_vs_numpy(dev, case):
    """B = 2, segments (37, 5, 130), num_ims [0, 37] / [5, 1] / [130, 64]: a slide with an empty level, single-row levels; NaN on
    every padded score (and on the level that is not chosen): they must not be read."""
    g = np.random.default_rng(11)
    n = sum(SEG)
    level_on = (1, 0, 1) if case == "level-1-off" else None
    s = g.standard_normal((2, n)).astype(np.float32) if case in ("distinct", "level-1-off") else TIES[g.integers(0, len(TIES), (2, n))]
    s[~P.valid_mask(SEG, NUMS, level_on)] = np.nan
    rank, count = _run_rank(dev, s, SEG, NUMS, level_on, case == "ascending")
    ref, ref_count = P.rank_joint(s, SEG, NUMS, level_on, case == "ascending")
    np.testing.assert_array_equal(count, ref_count)
    np.testing.assert_array_equal(rank, ref)
    assert ref_count.tolist() == ([135, 102] if level_on is None else [130, 101])


def test_rank_joint_streams_more_than_two_key_tiles(dev):
    """Joint length 2 tile + 3, every row valid, heavy ties across the tiles: the tile loop, its tail and its last partial tile."""
    from paths_amd.saliency import rank_joint_tile
    tile = rank_joint_tile()
    seg = (tile + 1, tile + 2)
    g = np.random.default_rng(5)
    s = g.integers(-40, 40, (2, sum(seg))).astype(np.float32)
    s[1, ::3] = g.standard_normal(len(s[1, ::3])).astype(np.float32)
    num = np.array([[seg[0]] * 2, [seg[1]] * 2])
    for ascending in (False, True):
        rank, count = _run_rank(dev, s, seg, num, None, ascending)
        ref, ref_count = P.rank_joint(s, seg, num, None, ascending)
        np.testing.assert_array_equal(count, ref_count)
        np.testing.assert_array_equal(rank, ref)
    assert count.tolist() == [2 * tile + 3] * 2


# ------------------------------------------------------------------------------------------------
# 2. paths_path_mask_points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_ims", ([0, 37], [19, 1]))
@pytest.mark.parametrize("D", [128, 384])
def test_path_mask_points_kernel_bitwise(dev, D, num_ims):
    from paths_amd.saliency import path_mask_points
    B, C, N = 2, 3, 37
    g = torch.Generator().manual_seed(D + num_ims[0])
    xs = torch.randn(B, N, D + 132, generator=g) * torch.exp2(torch.randint(-12, 4, (B, N, 1), generator=g).float())
    xs[:, ::5, 3] = -0.0
    valid = torch.arange(N)[None, :] < torch.as_tensor(num_ims)[:, None]
    xs[~valid] = float("nan")
    xd = xs.to(dev)[..., :D]                                              # a strided view
    x = xs[..., :D].contiguous().numpy()
    base = torch.randn(D, generator=g)
    # the level's slice of a joint rank [B, 100]: ranks are a permutation of the valid rows' 0 .. n_b - 1 shifted by 2, some rows -1
    joint = torch.full((B, 100), 12345, dtype=torch.int32)
    for b in range(B):
        joint[b, 40:40 + num_ims[b]] = (torch.randperm(num_ims[b], generator=g) + 2).int()
    joint[:, 40:40 + N:7] = -1
    nb = [n + 2 for n in num_ims]
    thr = torch.tensor([[0, nb[1]], [nb[0] // 2, 2], [nb[0], 3]], dtype=torch.int32)
    ins = torch.tensor([0, 1, 0], dtype=torch.int32)
    nd = torch.tensor(num_ims, device=dev)
    rk = joint.to(dev)[:, 40:40 + N]
    for bs in (base, None):
        out = path_mask_points(xd, None if bs is None else bs.to(dev), rk, thr.to(dev), ins.to(dev), nd).cpu().numpy()
        ref = P.mask_points(x, None if bs is None else bs.numpy(), joint[:, 40:40 + N].numpy(), thr.numpy(), ins.numpy(), num_ims)
        assert out.shape == ref.shape == (C * B, N, D)
        np.testing.assert_array_equal(out.view(np.uint32), ref.view(np.uint32))
        k = P.kept(joint[:, 40:40 + N].numpy(), thr.numpy(), ins.numpy(), num_ims)
        o = out.reshape(C, B, N, D).view(np.uint32)
        want = np.zeros(D, np.float32) if bs is None else bs.numpy()
        assert (o[k] == np.broadcast_to(x, (C, B, N, D)).view(np.uint32)[k]).all()              # kept rows: x bit for bit
        gone = ~k & valid.numpy()[None]
        assert (o[gone] == want.view(np.uint32)[None, :]).all()                             # removed rows: the baseline bit for bit
        assert not o[:, ~valid.numpy()].any()                                               # padded rows: +0
        if max(num_ims) > 1:
            assert k.any() and gone.any()


# ------------------------------------------------------------------------------------------------
# the function: the small setting, its recorded HIP trace and fixed distinct scores, shared
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_trace(dev, small):
    from paths_amd import utils as putils
    t = []
    with torch.no_grad():
        putils.recurse(small["model"], small["slides"], small["cfg"].top_k_patches, 5, trace=t, rollout=True)
    return t


def _fixed_scores(trace, dev, seed=2):
    """Distinct values over all levels and slides, in pseudo-random order."""
    Ns = [int(rec["locs"].shape[1]) for rec in trace]
    B = int(trace[0]["num_ims"].shape[0])
    v = torch.randperm(B * sum(Ns), generator=torch.Generator().manual_seed(seed)).float().sub(100.0).div(8.0).view(B, sum(Ns))
    return [t.contiguous().to(dev) for t in v.split(Ns, dim=1)]


def _oracle_curves(st, trace, out, target, base, levels):
    """Both curves of the oracle along its own path, its points built by perturb_ref from the HIP ranks mapped to the oracle's rows."""
    otrace, rows = st["otrace"], st["rows"]
    ranks = R.to_oracle_order(trace, otrace, "perturbation_rank")
    B = rows[0].shape[0]
    n = np.zeros(B, np.int64)
    for l, (rk, orec) in enumerate(zip(ranks, otrace)):
        valid = (torch.arange(rk.shape[1])[None, :] < orec["num_ims"][:, None]).numpy()
        r = rk.numpy()
        assert ((r[valid] >= 0) == (l in levels)).all()
        n += (valid & (r >= 0)).sum(1)
    np.testing.assert_array_equal(out["counts"].numpy(), P.counts(n, STEPS))
    for b in range(B):
        r = np.concatenate([rk.numpy()[b, :int(orec["num_ims"][b])] for rk, orec in zip(ranks, otrace)])
        assert sorted(r[r >= 0].tolist()) == list(range(int(n[b])))                          # jointly a permutation
    thr, ins = P.curve_members(n, STEPS)
    bs = None if base is None else base.numpy()
    pts = [torch.from_numpy(P.mask_points(x.numpy(), bs, rk.numpy(), thr, ins, orec["num_ims"].numpy())).view(len(ins), *x.shape)
           for x, rk, orec in zip(rows, ranks, otrace)]
    tg = torch.stack([R.frozen_path(st["params"], st["ocfg"], st["grids"], otrace, [p[c] for p in pts], target)["target"]
                      for c in range(len(ins))])
    return tg[:STEPS + 1].t(), tg[STEPS + 1:].t()                                           # deletion, insertion [B, steps + 1]


@pytest.mark.parametrize("variant", ["grad_x_input", "fixed-levels-2-3-baseline"])
def test_curves_vs_oracle_along_its_own_path(dev, small, hip_trace, variant):
    from paths_amd.saliency import perturbation_curves
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    if variant == "grad_x_input":
        scores, levels, base = "grad_x_input", None, None
    else:
        scores, levels = _fixed_scores(hip_trace, dev), [2, 3]
        base = torch.randn(1024, generator=torch.Generator().manual_seed(5)) * 0.2
    out, trace = perturbation_curves(model, slides, keep, 5, scores, steps=STEPS, mode="both", levels=levels,
                                     baseline=None if base is None else base.to(dev))
    assert int(out["status"].item()) == 0 and all("fts" not in rec for rec in trace)
    assert out["fractions"].dtype == torch.float64 and out["fractions"].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    if variant == "grad_x_input":                          # exact ties are not expected: if two valid values of a slide do tie, fail loudly
        for b in range(3):
            v = torch.cat([rec["grad_x_input"][b, :int(rec["num_ims"][b])] for rec in trace]).cpu().numpy()
            assert len(np.unique(v)) == len(v), f"slide {b}: two valid grad_x_input values tie exactly"
    dele, inse = _oracle_curves(st, trace, out, "risk", base, range(5) if levels is None else levels)
    for b in range(3):
        got = torch.cat([out["deletion"][b], out["insertion"][b]]).cpu()
        ref = torch.cat([dele[b], inse[b]])
        e = rel_err(got, ref)
        print(f"{variant} slide {b}: {2 * (STEPS + 1)} targets, rel err {e:.3g}; deletion {out['deletion'][b].tolist()}")
        assert e < 1e-4, (b, e)
    assert float((out["deletion"][:, 0] - out["deletion"][:, -1]).abs().min()) > 0           # (the curves move)
    for name, cv in (("deletion", out["deletion"]), ("insertion", out["insertion"])):
        d = cv.double().cpu()
        auc = ((d[:, :-1] + d[:, 1:]) * 0.5 * 0.25).sum(1)
        assert out[name + "_auc"].dtype == torch.float64 and torch.allclose(out[name + "_auc"].cpu(), auc, rtol=1e-12, atol=0)


def test_identities_between_the_curves(dev, small, hip_trace):
    from paths_amd.saliency import integrated_gradients, perturbation_curves
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    scores = _fixed_scores(hip_trace, dev)
    run = lambda **kw: perturbation_curves(model, slides, keep, 5, scores, steps=STEPS, **kw)
    out, trace = run()
    assert out["deletion"].shape == out["insertion"].shape == (3, STEPS + 1) and out["counts"].shape == (STEPS + 1, 3)
    assert torch.equal(out["deletion"][:, 0], out["target"]) and torch.equal(out["insertion"][:, STEPS], out["target"])
    assert torch.equal(out["deletion"][:, STEPS], out["target_baseline"]) and torch.equal(out["insertion"][:, 0], out["target_baseline"])
    ig, _ = integrated_gradients(model, slides, keep, 5, steps=2)
    assert torch.equal(out["target_baseline"], ig["target_baseline"]) and torch.equal(out["target"], ig["target"])
    od, td = run(mode="deletion")
    assert "insertion" not in od and "insertion_auc" not in od
    assert torch.equal(od["deletion"], out["deletion"]) and torch.equal(od["deletion_auc"], out["deletion_auc"])
    oi, _ = run(mode="insertion")
    assert "deletion" not in oi and torch.equal(oi["insertion"], out["insertion"])
    o2, t2 = run()
    assert torch.equal(o2["deletion"], out["deletion"]) and torch.equal(o2["insertion"], out["insertion"])
    assert all(torch.equal(a["perturbation_rank"], b["perturbation_rank"]) for a, b in zip(trace, t2))
    o1, o5 = run(chunk=1)[0], run(chunk=5)[0]
    for name in ("deletion", "insertion"):
        assert rel_err(o1[name], o5[name]) < 1e-5, name
    # the ranks: -1 on padded rows, jointly a permutation of 0 .. n_b - 1 on the valid ones; descending = False turns them round
    oa, ta = run(descending=False)
    for b in range(3):
        r = torch.cat([rec["perturbation_rank"][b, :int(rec["num_ims"][b])] for rec in trace]).cpu()
        ra = torch.cat([rec["perturbation_rank"][b, :int(rec["num_ims"][b])] for rec in ta]).cpu()
        n = int(out["counts"][STEPS, b])
        assert sorted(r.tolist()) == list(range(n)) and torch.equal(r + ra, torch.full_like(r, n - 1))
    for rec in trace:
        pad = torch.arange(rec["perturbation_rank"].shape[1], device=dev)[None, :] >= rec["num_ims"][:, None]
        assert bool((rec["perturbation_rank"][pad] == -1).all()) and rec["perturbation_rank"].dtype == torch.int32


def test_a_given_trace_is_the_path(dev, small, hip_trace):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    from paths_amd.saliency import input_gradients, perturbation_curves
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    t = [dict(rec) for rec in hip_trace]
    with H.spy_calls() as calls:
        out, tr = perturbation_curves(model, slides, keep, 5, "rollout", trace=t, steps=STEPS)
    assert "paths_topk" not in calls and "paths_topk_rows" not in calls and tr is t
    assert all("perturbation_rank" in rec for rec in t) and int(out["status"].item()) == 0
    assert float((out["deletion"][:, 0] - out["deletion"][:, -1]).abs().min()) > 0
    # a trace of input_gradients: the same path and rows as the call that makes that pass itself, so the same curves bit for bit
    own, _ = perturbation_curves(model, slides, keep, 5, "grad_norm", steps=STEPS)
    _, tg = input_gradients(model, slides, keep, 5)
    with H.spy_calls() as calls:
        giv, _ = perturbation_curves(model, slides, keep, 5, "grad_norm", trace=tg, steps=STEPS)
    assert "paths_topk" not in calls and "paths_saliency_rows" not in calls
    assert torch.equal(own["deletion"], giv["deletion"]) and torch.equal(own["insertion"], giv["insertion"])
    others = [DeviceSlide.synthetic(15, sid, (6, 7), p_bg=0.1, device=dev) for sid in range(3)]
    with pytest.raises(ValueError, match="trace|path"):
        perturbation_curves(model, others, keep, 5, "rollout", trace=[dict(rec) for rec in hip_trace], steps=STEPS)
    with pytest.raises(ValueError, match=r"\[B, N\].*got \(3, \d+, 2\)"):
        perturbation_curves(model, slides, keep, 5, "locs", trace=[dict(rec) for rec in hip_trace], steps=STEPS)
    with pytest.raises(ValueError, match="no such entry"):
        perturbation_curves(model, slides, keep, 5, "attention", trace=[dict(rec) for rec in hip_trace], steps=STEPS)
    bad = _fixed_scores(hip_trace, dev)
    bad[2][1, 0] = float("nan")                                       # (every slide has at least one patch at every level)
    assert int(hip_trace[2]["num_ims"][1]) > 0
    with pytest.raises(ValueError, match="NaN.*slide.*1"):
        perturbation_curves(model, slides, keep, 5, bad, steps=STEPS)
    ok = _fixed_scores(hip_trace, dev)
    for l, rec in enumerate(hip_trace):                               # NaN on padded rows and on levels not chosen is not looked at
        ok[l][torch.arange(ok[l].shape[1], device=dev)[None, :] >= rec["num_ims"][:, None]] = float("nan")
    ok[0][:] = float("nan")
    perturbation_curves(model, slides, keep, 5, ok, steps=1, levels=[1, 2, 3, 4])


def test_launch_hygiene(dev, small, hip_trace):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlideBatch
    from paths_amd.saliency import input_gradients, integrated_gradients, perturbation_curves
    cfg, model, _, slides, _ = _setup(dev)                            # (a model of its own: the training step changes it)
    keep = cfg.top_k_patches
    labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
    batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
    with H.spy_calls() as calls:
        with torch.no_grad():
            putils.recurse(model, slides, keep, 5)
        input_gradients(model, slides, keep, 5)
        integrated_gradients(model, slides, keep, 5, steps=2)
        model.train()
        putils.train_step(model, torch.optim.AdamW(model.parameters(), lr=1e-7), batch, 5, keep)
    assert len(calls) > 100 and "paths_topk" in calls and not [c for c in calls if c in NEW]
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    scores = _fixed_scores(hip_trace, dev)
    for mode, chunk, passes in (("both", None, 1 + 2 * 2), ("deletion", 1, 1 + 3), ("insertion", 5, 1 + 1)):
        with H.spy_calls() as calls:                                  # (default chunk max(1, 8 // 3) = 2; steps - 1 = 3 points between)
            perturbation_curves(model, slides, keep, 5, scores, steps=STEPS, mode=mode, chunk=chunk)
        assert calls.count("paths_rank_joint") == 1
        assert calls.count("paths_path_mask_points") == 5 * passes
        assert calls.count("paths_topk") == 4 and calls.count("paths_saliency_rows") == 5      # the path pass, once
        assert "paths_path_points" not in calls and "paths_path_accumulate" not in calls
    assert all(p.grad is None for p in model.parameters())
    was = model.training
    for training in (True, False):                                    # the model's mode is restored
        model.train(training)
        perturbation_curves(model, slides, keep, 5, scores, steps=1)
        assert model.training == training and all(m.training == training for m in model.modules())
    model.train(was)


def test_fp16_grids_and_host_slides_give_the_fp32_resident_curves(dev):
    """Features that fp16 represents exactly: the training path gathers fp32 copies, so fp16 grids and pinned host grids give the
    rows, and with fixed scores the curves, of the fp32 resident slides bit for bit."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    from paths_amd.saliency import perturbation_curves
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[16] * 4)
    host16 = [HostSlide.synthetic(14, sid, (6, 7), device=dev, dtype=torch.float16) for sid in range(3)]
    dev16 = [s.to_device() for s in host16]
    dev32 = [DeviceSlide([g.float() for g in s.grids], patch_size=s.patch_size) for s in dev16]
    t = []
    with torch.no_grad():
        putils.recurse(model, dev32, cfg.top_k_patches, 5, trace=t)
    scores = _fixed_scores(t, dev, seed=4)
    run = lambda sl: perturbation_curves(model, sl, cfg.top_k_patches, 5, scores, steps=STEPS)
    ref, rt = run(dev32)
    assert float((ref["deletion"][:, 0] - ref["deletion"][:, -1]).abs().min()) > 0
    for name, slides in (("fp16 resident", dev16), ("fp16 host", host16)):
        got, gt = run(slides)
        for key in ("deletion", "insertion", "target", "target_baseline", "deletion_auc", "insertion_auc"):
            assert torch.equal(got[key], ref[key]), (name, key)
        assert all(torch.equal(a["perturbation_rank"], b["perturbation_rank"]) for a, b in zip(gt, rt)), name
    del host16
    gc.collect()
    torch.cuda.synchronize()
    empty = getattr(torch._C, "_host_emptyCache", None)
    if empty is not None:
        empty()
