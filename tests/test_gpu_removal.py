"""Removal curves on the free path on the GPU (paths_amd/saliency.py:removal_curves, csrc/perturb_rows.hip): the two kernels
against their numpy restatement (tests/removal_ref.py; integers and bytes, no tolerance), a masked view against the slide with the
same rows zeroed (bitwise), the curves against the oracle run on zeroed grids, the identities, the fallback, the errors, the other
slide kinds and the launch lists."""
import gc

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import removal_ref as M
from tests.test_gpu_backward import rel_err
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)
from tests.test_gpu_path_attributions import small  # noqa: F401  (fixture)
from tests.test_gpu_perturbation import _fixed_scores, hip_trace  # noqa: F401  (fixture)
from tests.test_gpu_saliency import _setup

pytestmark = pytest.mark.gpu

STEPS = 4
PS = 256
NEW = ("paths_removal_masks", "paths_visited_overlap", "paths_level0_mask_rows")
# the oracle comparison's own setting (chosen on the CPU: see test_curves_vs_oracle_on_zeroed_grids)
ORACLE_WSEED, ORACLE_DSEED = 50, 14


# ------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------
def _garbage(g, shape):
    return g.integers(-(1 << 62), 1 << 62, shape, dtype=np.int64)


@pytest.mark.parametrize("num_ims", ([0, 37], [19, 1]))
@pytest.mark.parametrize("grid", [(5, 9), (67, 131)])
def test_removal_masks_and_overlap_kernels_exact(dev, grid, num_ims):
    """B = 2, C = 3, N = 40; a non-square grid (a swapped x / y shows) and one of 8,777 cells (three workgroups per member, a ragged
    16-byte tail); ranks with -1, garbage in the locations of padded rows, thresholds 0 / middle / all; a source that is not 16-byte
    aligned takes the byte path.  Bytes and integers against tests/removal_ref.py, bit-identical on repeat."""
    from paths_amd.saliency import removal_masks, visited_overlap
    X, Y = grid
    B, C, N = 2, 3, 40
    g = np.random.default_rng(X * 100 + num_ims[0])
    src = [(g.random((X, Y)) > 0.2).astype(np.uint8) for _ in range(B)]
    src[1][src[1] != 0] = 255                                             # any non-zero byte is tissue
    locs = _garbage(g, (B, N, 2))
    for b in range(B):
        cells = g.permutation(X * Y)[:num_ims[b]]
        locs[b, :num_ims[b], 0] = (cells // Y) * PS + g.integers(0, PS, num_ims[b])
        locs[b, :num_ims[b], 1] = (cells % Y) * PS + g.integers(0, PS, num_ims[b])
    joint = np.full((B, 100), 12345, np.int32)
    for b in range(B):
        joint[b, 40:40 + num_ims[b]] = g.permutation(num_ims[b]).astype(np.int32)
    joint[:, 40:40 + N:7] = -1
    rank = joint[:, 40:40 + N]
    thr = np.array([[0, 0], [num_ims[0] // 2, max(1, num_ims[1] // 2)], num_ims], np.int32)
    gxy = torch.tensor([[X] * B, [Y] * B], dtype=torch.int32, device=dev)
    nd = torch.tensor(num_ims, device=dev)
    ld, rd, td = torch.from_numpy(locs).to(dev), torch.from_numpy(joint).to(dev)[:, 40:40 + N], torch.from_numpy(thr).to(dev)
    pick = M.chosen(num_ims, rank, thr)
    ref, ref_left = M.removal_masks(src, locs, PS, pick)
    for shift in (0, 1):                                                  # (1: the sources start one byte off a 16-byte boundary)
        holder = [torch.zeros(X * Y + 16, dtype=torch.uint8, device=dev) for _ in range(B)]
        sd = [h[shift:shift + X * Y].view(X, Y) for h in holder]
        for t, s in zip(sd, src):
            t.copy_(torch.from_numpy(s))
        ptrs = torch.tensor([t.data_ptr() for t in sd], dtype=torch.int64, device=dev)
        assert all(t.data_ptr() % 16 == shift for t in sd)
        masks, left = removal_masks(ptrs, gxy[0], gxy[1], X * Y, ld, PS, nd, rd, td)
        masks2, left2 = removal_masks(ptrs, gxy[0], gxy[1], X * Y, ld, PS, nd, rd, td)
        assert masks.dtype == torch.uint8 and masks.shape == (C, B, (X * Y + 15) // 16 * 16) and left.dtype == torch.int32
        assert torch.equal(masks[..., :X * Y], masks2[..., :X * Y]) and torch.equal(left, left2)        # bit-identical repeat
        got = masks[..., :X * Y].cpu().numpy().reshape(C, B, X, Y)
        for c in range(C):
            for b in range(B):
                np.testing.assert_array_equal(got[c, b], ref[c][b], err_msg=f"member {c} slide {b} shift {shift}")
        np.testing.assert_array_equal(left.cpu().numpy(), ref_left)
        assert all(torch.equal(t.cpu(), torch.from_numpy(s)) for t, s in zip(sd, src))                  # the sources are only read
    if max(num_ims) > 1:
        assert (got[2] != got[0]).any() and (got[1] != got[0]).any()
    np.testing.assert_array_equal(got[0], np.stack(src))                                                # thr 0: a copy
    # the bitmap of the recorded cells: a NULL source, every valid row set
    bm, bleft = removal_masks(None, gxy[0], gxy[1], X * Y, ld, PS, nd, None, None, set_cells=True)
    rbm, rleft = M.removal_masks([np.zeros((X, Y), np.uint8)] * B, locs, PS, M.all_valid(num_ims, N), set_cells=True)
    np.testing.assert_array_equal(bm[0, :, :X * Y].cpu().numpy().reshape(B, X, Y), np.stack(rbm[0]))
    np.testing.assert_array_equal(bleft.cpu().numpy(), rleft)
    assert bleft[0].tolist() == list(num_ims)
    # set on a source: the same kernel with set != 0 and ranks
    sm, sleft = removal_masks(ptrs, gxy[0], gxy[1], X * Y, ld, PS, nd, rd, td, set_cells=True)
    rsm, rsleft = M.removal_masks(src, locs, PS, pick, set_cells=True)
    np.testing.assert_array_equal(sm[..., :X * Y].cpu().numpy().reshape(C, B, X, Y), np.array([[m for m in row] for row in rsm]))
    np.testing.assert_array_equal(sleft.cpu().numpy(), rsleft)
    # the overlap of C = 3 members' passes with the recorded cells: rows over more than one wave and more than one 256-row step
    Nm = 300
    num_m = np.array([0, min(Nm, X * Y), 19, 1, min(257, X * Y), 33])
    locs_m = _garbage(g, (C * B, Nm, 2))
    for v in range(C * B):
        cells = g.permutation(X * Y)[:num_m[v]]
        if num_ims[v % B]:                                  # half of the member's rows on recorded cells where there are any
            rec = (locs[v % B, :num_ims[v % B]] // PS) @ np.array([Y, 1])
            k = min(len(rec), num_m[v] // 2)
            cells = np.concatenate([rec[:k], np.setdiff1d(cells, rec[:k], assume_unique=False)[:num_m[v] - k]])
            num_m[v] = len(cells)
        locs_m[v, :num_m[v], 0], locs_m[v, :num_m[v], 1] = (cells // Y) * PS + 3, (cells % Y) * PS + 255
    args = (bm[0], gxy[0], gxy[1], torch.from_numpy(locs_m).to(dev), torch.from_numpy(num_m).to(dev), PS)
    ov = visited_overlap(*args)
    assert ov.dtype == torch.int32 and torch.equal(ov, visited_overlap(*args))
    want = M.visited_overlap(rbm[0], locs_m, num_m, PS)
    np.testing.assert_array_equal(ov.cpu().numpy(), want)
    if max(num_ims) > 1:
        assert want.max() > 0 and (want < num_m).any()
    # a pass against itself: num_ims
    own = visited_overlap(bm[0], gxy[0], gxy[1], ld, nd, PS)
    assert own.tolist() == list(num_ims)


# ------------------------------------------------------------------------------------------------
# the function: the small setting of the attribution tests
# ------------------------------------------------------------------------------------------------
def _removed_cells(out, slides, name, s, b, L=5):
    """Per level the cells [k, 2] member ``s`` (1 .. steps) of slide ``b`` turned to background: set in the source, clear in the member."""
    cells = []
    for l in range(L):
        X, Y = slides[b].shape(l)
        m = out["masks"][name][l][s - 1, b, :X * Y].view(X, Y)
        cells.append(torch.nonzero((slides[b].masks[l] != 0) & (m == 0)).cpu())
    return cells


def _member_views(out, slides, name, s0, c, L=5):
    views = []
    for ci in range(c):
        for b, sl in enumerate(slides):
            views.append(sl.with_masks([out["masks"][name][l][s0 + ci, b, :sl.shape(l)[0] * sl.shape(l)[1]].view(*sl.shape(l)) for l in range(L)]))
    return views


def _zeroed_twin(host, removed, dev, dtype=torch.float32):
    from paths_amd.data_utils.slide import DeviceSlide
    grids = []
    for g, cells in zip(host, removed):
        if len(cells):
            g = g.clone()
            g[cells[:, 0], cells[:, 1]] = 0
        grids.append(g)
    return DeviceSlide.from_host(grids, dev, dtype=dtype)


def _same_pass(a, ta, b, tb, what):
    """Two recursions' outputs and traces agree bit for bit on everything that is somebody's: logits, and per level num_ims and the
    valid rows' locs / importance, the kept indices below the last level."""
    assert torch.equal(a["logits"], b["logits"]), what
    assert len(ta) == len(tb)
    for l, (ra, rb) in enumerate(zip(ta, tb)):
        assert torch.equal(ra["num_ims"], rb["num_ims"]), (what, l)
        for v in range(ra["num_ims"].shape[0]):
            n = int(ra["num_ims"][v])
            assert torch.equal(ra["locs"][v, :n], rb["locs"][v, :n]), (what, l, v)
            assert torch.equal(ra["importance"][v, :n], rb["importance"][v, :n]), (what, l, v)
        if "keep_idx" in ra:
            assert torch.equal(ra["keep_count"], rb["keep_count"]), (what, l)
            for v in range(ra["num_ims"].shape[0]):
                k = int(ra["keep_count"][v])
                assert torch.equal(ra["keep_idx"][v, :k], rb["keep_idx"][v, :k]), (what, l, v)


def _check_twins(model, slides, keep, out, names, dev, chunk, host):
    """Every member of ``out`` as views and as zeroed DeviceSlides, in the batch composition of removal_curves: bitwise the same pass,
    and the curve's values.  Returns {(name, s): (output, trace)} of the members' passes."""
    from paths_amd import utils as putils
    from paths_amd.saliency import risk_score
    B, passes = len(slides), {}
    for name in names:
        for s0 in range(0, STEPS, chunk):
            c = min(chunk, STEPS - s0)
            views = _member_views(out, slides, name, s0, c)
            twins = [_zeroed_twin(host[b], _removed_cells(out, slides, name, s0 + ci + 1, b), dev) for ci in range(c) for b in range(B)]
            tv, tt = [], []
            with torch.no_grad():
                ov = putils.recurse(model, views, keep, 5, trace=tv)
                ot = putils.recurse(model, twins, keep, 5, trace=tt)
            _same_pass(ov, tv, ot, tt, f"{name} members {s0 + 1} .. {s0 + c}")
            assert int(ov["status"].item()) == int(ot["status"].item())
            assert torch.equal(risk_score(ov["logits"]).view(c, B).t(), out[name][:, s0 + 1:s0 + 1 + c]), (name, s0)
            for ci in range(c):
                passes[(name, s0 + ci + 1)] = (ov, tv, ci)
            del twins
    return passes


@pytest.fixture(scope="module")
def host_grids(dev, small):
    return [[g.cpu() for g in s.grids] for s in small["slides"]]


@pytest.fixture(scope="module")
def both(dev, small, hip_trace):
    """removal_curves of the small setting by fixed distinct scores over all levels, order "both": shared by the tests below."""
    from paths_amd.saliency import removal_curves
    scores = _fixed_scores(hip_trace, dev)
    out, trace = removal_curves(small["model"], small["slides"], small["cfg"].top_k_patches, 5, scores, steps=STEPS, order="both")
    return dict(out=out, trace=trace, scores=scores)


def test_masked_view_is_the_zeroed_slide_bitwise(dev, small, both, host_grids):
    """The test that pins the semantics: for every member of both orders, the removed cells read from the member masks, host grids
    with those rows zeroed uploaded as real DeviceSlides, run in the same batch composition: the same pass bit for bit."""
    st, out = small, both["out"]
    assert int(out["status"].item()) == 0
    removed = [sum(len(c) for c in _removed_cells(out, st["slides"], "morf", STEPS, b)) for b in range(3)]
    assert min(removed) > 50                                              # (half of about 270 visited patches, less those already background)
    _check_twins(st["model"], st["slides"], st["cfg"].top_k_patches, out, ("morf", "lerf"), dev, 2, host_grids)
    assert float((out["morf"][:, 0] - out["morf"][:, -1]).abs().min()) > 0     # (the curves move)


def test_identities(dev, small, both, hip_trace):
    from paths_amd import utils as putils
    from paths_amd.saliency import removal_curves, risk_score
    st, out, trace, scores = small, both["out"], both["trace"], both["scores"]
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    with torch.no_grad():
        free = putils.recurse(model, slides, keep, 5)
    assert out["morf"].shape == out["lerf"].shape == (3, STEPS + 1) and out["morf"].dtype == torch.float32
    assert torch.equal(out["target"], risk_score(free["logits"]))                              # point 0: recurse()'s target, bit for bit
    assert torch.equal(out["morf"][:, 0], out["target"]) and torch.equal(out["lerf"][:, 0], out["target"])
    assert out["fractions"].dtype == torch.float64 and out["fractions"].tolist() == [0.0, 0.125, 0.25, 0.375, 0.5]
    n = [sum(int(rec["num_ims"][b]) for rec in trace) for b in range(3)]
    np.testing.assert_array_equal(out["counts"].numpy(), M.counts(n, STEPS, 0.5))
    for name in ("morf", "lerf"):
        d = out[name].double().cpu()
        auc = ((d[:, :-1] + d[:, 1:]) * 0.5 * 0.125).sum(1)
        assert out[name + "_auc"].dtype == torch.float64 and torch.allclose(out[name + "_auc"].cpu(), auc, rtol=1e-12, atol=0)
        vis, ov = out["visited"][name], out["path_overlap"][name]
        assert vis.shape == ov.shape == (3, STEPS + 1, 5) and vis.dtype == ov.dtype == torch.int32
        nums = torch.stack([rec["num_ims"] for rec in trace], dim=1).int()
        assert torch.equal(vis[:, 0], nums) and torch.equal(ov[:, 0], nums)
        assert bool((ov <= vis).all()) and bool((ov[:, 1:] < vis[:, 1:]).any())              # (the path does move)
        for b in range(3):                                               # the ranks: jointly a permutation of the valid rows
            r = torch.cat([rec["removal_rank_" + name][b, :int(rec["num_ims"][b])] for rec in trace]).cpu()
            assert r.dtype == torch.int32 and sorted(r.tolist()) == list(range(n[b]))
    rm = torch.cat([torch.cat([rec["removal_rank_morf"][b, :int(rec["num_ims"][b])] for rec in trace]) for b in range(3)])
    rl = torch.cat([torch.cat([rec["removal_rank_lerf"][b, :int(rec["num_ims"][b])] for rec in trace]) for b in range(3)])
    assert torch.equal((rm + rl).cpu(), torch.cat([torch.full((k,), k - 1, dtype=torch.int32) for k in n]))   # distinct scores: lerf is morf reversed
    assert torch.equal(out["aopc_gap"], out["lerf_auc"] - out["morf_auc"])
    assert all("perturbation_rank" not in rec for rec in trace)
    run = lambda **kw: removal_curves(model, slides, keep, 5, scores, steps=STEPS, **kw)
    om, _ = run(order="morf")                                            # the morf half of "both", and a repeat, bit for bit
    assert "lerf" not in om and "lerf_auc" not in om and "aopc_gap" not in om and list(om["visited"]) == ["morf"]
    assert torch.equal(om["morf"], out["morf"]) and torch.equal(om["morf_auc"], out["morf_auc"])
    assert torch.equal(om["visited"]["morf"], out["visited"]["morf"]) and torch.equal(om["path_overlap"]["morf"], out["path_overlap"]["morf"])
    o2, t2 = run(order="both")
    for key in ("morf", "lerf", "target", "morf_auc", "lerf_auc", "aopc_gap"):
        assert torch.equal(o2[key], out[key]), key
    assert all(torch.equal(o2["visited"][k], out["visited"][k]) and torch.equal(o2["path_overlap"][k], out["path_overlap"][k]) for k in ("morf", "lerf"))
    # a given trace is the path: the same ranks, masks and curves as the call that makes the path pass itself
    with H.spy_calls() as calls:
        og, tg = run(order="morf", trace=[dict(rec) for rec in hip_trace])
    assert "paths_saliency_rows" not in calls and torch.equal(og["morf"], out["morf"])
    # the leaf level alone: nothing reacts - every member keeps the recorded path, and its last level drops by exactly counts
    ol, tl = run(order="both", levels=[4])
    n4 = [int(tl[4]["num_ims"][b]) for b in range(3)]
    np.testing.assert_array_equal(ol["counts"].numpy(), M.counts(n4, STEPS, 0.5))
    for name in ("morf", "lerf"):
        vis, ov = ol["visited"][name], ol["path_overlap"][name]
        assert torch.equal(vis, ov)
        assert torch.equal(vis[:, :, :4], vis[:, :1, :4].expand(-1, STEPS + 1, -1))
        assert torch.equal(vis[:, 0:1, 4] - vis[:, :, 4], ol["counts"].t().to(dev).int())


class _Zeroed:
    """A slide's grids for the oracle with some cells' rows zeroed: {level: set of (x, y)}."""

    def __init__(self, base, cells):
        self.base = base
        self.removed = [set(map(tuple, c.tolist())) for c in cells]

    def shape(self, level):
        return self.base.shape(level)

    def rows(self, level, x, y):
        r = self.base.rows(level, x, y).clone()
        if self.removed[level]:
            hit = torch.tensor([(int(a), int(b)) in self.removed[level] for a, b in zip(x, y)], dtype=torch.bool)
            r[hit] = 0
        return r


def _boundary_gap(otrace, b, keep):
    gap = float("inf")
    for rec in otrace[:-1]:
        n = int(rec["num_ims"][b])
        if n > keep:
            s = torch.sort(rec["importance"][b, :n], descending=True).values
            gap = min(gap, float(s[keep - 1] - s[keep]))
    return gap


@pytest.fixture(scope="module")
def oracle_setting(dev):
    """The small setting at the seeds of the oracle comparison, with the oracle's unperturbed trace and the host grids."""
    from oracle import paths_oracle as orc
    cfg, model, params, slides, ocfg = _setup(dev, None, wseed=ORACLE_WSEED, dseed=ORACLE_DSEED)
    grids = [orc.LazyGrids(s.synthetic_spec) for s in slides]
    otrace = []
    with torch.no_grad():
        orc.inference_end2end(params, ocfg, grids, None, otrace)
    return dict(cfg=cfg, model=model, params=params, slides=slides, ocfg=ocfg, grids=grids, otrace=otrace,
                host=[[g.cpu() for g in s.grids] for s in slides])


def test_curves_vs_oracle_on_zeroed_grids(dev, oracle_setting):
    """scores = "importance", all levels, max_fraction = 0.5, both orders: per member (order, step, slide) the oracle
    (orc.inference_end2end) runs on grids with the member's removed rows zeroed; the visited cell sets per level must be identical
    and a slide's targets within 1e-4 norm-wise over its points.  A member may be left out only if the oracle's own top-K boundary
    gap at some level is below 2e-6 (and is, here, only if its cells then differ); at most one member in eight may be left out.

    Seeds: wseed 50, dseed 14, chosen on the CPU with the oracle alone (ranking by its own importance): 2 of the 24 members have a
    boundary gap below 2e-6 there (morf step 4, slides 0 and 2: gap exactly 0).  Such gaps are common: the reference loads every
    level-0 cell, so removed level-0 cells are identical all-zero tokens with equal importance, and whenever the top-16 boundary of
    level 0 falls among them the gap is 0 and torch.topk and paths_topk pick different ones (the shared small setting, wseed 3,
    has 11 of 24; 244 seed pairs scanned gave 2 .. 12, this pair alone within the cap of 3).  Screened on the GPU: 2 of 24."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    from paths_amd.saliency import removal_curves, risk_score
    st = oracle_setting
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    out, trace = removal_curves(model, slides, keep, 5, "importance", steps=STEPS, order="both", max_fraction=0.5)
    passes = _check_twins(model, slides, keep, out, ("morf", "lerf"), dev, 2, st["host"])
    close, left_out, total = 0, [], 0
    ref = {name: torch.zeros(3, STEPS + 1) for name in ("morf", "lerf")}
    use = {name: torch.ones(3, STEPS + 1, dtype=torch.bool) for name in ("morf", "lerf")}
    base = risk_score(st["otrace"][-1]["logits"])
    for name in ("morf", "lerf"):
        ref[name][:, 0] = base
        for s in range(1, STEPS + 1):
            grids = [_Zeroed(st["grids"][b], _removed_cells(out, slides, name, s, b)) for b in range(3)]
            ot = []
            with torch.no_grad():
                orc.inference_end2end(st["params"], st["ocfg"], grids, None, ot)
            ref[name][:, s] = risk_score(ot[-1]["logits"])
            o, t, ci = passes[(name, s)]
            for b in range(3):
                total += 1
                v = ci * 3 + b
                gap = _boundary_gap(ot, b, 16)
                close += gap < 2e-6
                same = all(int(rec["num_ims"][v]) == int(orec["num_ims"][b]) and
                           sorted(map(tuple, torch.div(rec["locs"][v, :int(rec["num_ims"][v])], PS, rounding_mode="floor").tolist())) ==
                           sorted(map(tuple, torch.div(orec["locs"][b, :int(orec["num_ims"][b])], PS, rounding_mode="floor").tolist()))
                           for rec, orec in zip(t, ot))
                if not same:
                    assert gap < 2e-6, f"{name} step {s} slide {b}: the visited cells differ and the oracle's boundary gap is {gap:.3g}"
                    left_out.append((name, s, b))
                    use[name][b, s] = False
    print(f"{total} members, {close} with an oracle boundary gap below 2e-6, left out {left_out}")
    assert close <= total // 8 and len(left_out) <= total // 8, (close, left_out)
    for b in range(3):
        m = torch.cat([use["morf"][b], use["lerf"][b]])
        got = torch.cat([out["morf"][b], out["lerf"][b]]).cpu()[m]
        want = torch.cat([ref["morf"][b], ref["lerf"][b]])[m]
        e = rel_err(got, want)
        print(f"slide {b}: {int(m.sum())} targets, rel err {e:.3g}; morf {out['morf'][b].tolist()} lerf {out['lerf'][b].tolist()}")
        assert e < 1e-4, (b, e)


def test_a_member_without_tissue_children_takes_the_careful_path(dev, small, hip_trace, host_grids):
    """levels = [1], max_fraction = 1: the last member loses every level-1 child of the level-0 patches it keeps; its pass repeats on
    the careful path (all remaining tissue cells of level 1, no parent state), status bit 0 shows, and the zeroed twin still agrees."""
    from paths_amd.saliency import removal_curves
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    with H.spy_calls() as calls:
        out, trace = removal_curves(model, slides, keep, 5, "importance", steps=STEPS, order="morf", levels=[1], max_fraction=1.0)
    assert "paths_fallback_all_cells" in calls and int(out["status"].item()) & 1
    n1 = trace[1]["num_ims"].cpu()
    assert out["counts"][STEPS].tolist() == n1.tolist()
    vis, ov = out["visited"]["morf"], out["path_overlap"]["morf"]
    assert ov[:, STEPS, 1].tolist() == [0, 0, 0] and bool((vis[:, STEPS, 1] > 0).all())     # other cells than the recorded ones
    for b in range(3):                                                    # ... all of the level's remaining tissue
        X, Y = slides[b].shape(1)
        assert int(vis[b, STEPS, 1]) == int(out["masks"]["morf"][1][STEPS - 1, b, :X * Y].count_nonzero())
    with H.spy_calls() as calls:
        _check_twins(model, slides, keep, out, ("morf",), dev, 2, host_grids)
    assert "paths_fallback_all_cells" in calls


def test_errors_come_before_any_member_pass(dev, small):
    from paths_amd.saliency import removal_curves
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    with H.spy_calls() as calls:
        with pytest.raises(ValueError, match=r"order 'morf', step 4 .* slide 0 without level-0 tissue"):
            removal_curves(model, slides, keep, 5, "importance", steps=STEPS, levels=[0], max_fraction=1.0)
    assert calls.count("paths_topk") == 4 and "paths_topk_rows" not in calls              # the path pass, nothing after it
    after = calls[calls.index("paths_rank_joint"):]
    assert set(after) == {"paths_rank_joint", "paths_removal_masks"}, sorted(set(after))
    assert after.count("paths_rank_joint") == 2 and after.count("paths_removal_masks") == 2 * 5
    assert all(p.grad is None for p in model.parameters()) and not model.training


def test_other_slide_kinds(dev):
    """fp16 resident and pinned host grids give the fp32 resident curves of the same values bit for bit; lstm = false runs with a
    given trace and raises without one."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    from paths_amd.saliency import removal_curves
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[16] * 4)
    host16 = [HostSlide.synthetic(14, sid, (6, 7), device=dev, dtype=torch.float16) for sid in range(3)]
    dev16 = [s.to_device() for s in host16]
    dev32 = [DeviceSlide([g.float() for g in s.grids], patch_size=s.patch_size) for s in dev16]
    t = []
    with torch.no_grad():
        putils.recurse(model, dev32, cfg.top_k_patches, 5, trace=t)
    scores = _fixed_scores(t, dev, seed=4)
    run = lambda sl: removal_curves(model, sl, cfg.top_k_patches, 5, scores, steps=STEPS)
    ref, rt = run(dev32)
    assert float((ref["morf"][:, 0] - ref["morf"][:, -1]).abs().min()) > 0
    for name, slides in (("fp16 resident", dev16), ("fp16 host", host16)):
        got, gt = run(slides)
        for key in ("morf", "lerf", "target", "morf_auc", "lerf_auc"):
            assert torch.equal(got[key], ref[key]), (name, key)
        for k in ("morf", "lerf"):
            assert torch.equal(got["visited"][k], ref["visited"][k]) and torch.equal(got["path_overlap"][k], ref["path_overlap"][k]), (name, k)
        assert all(torch.equal(a["removal_rank_morf"], b["removal_rank_morf"]) for a, b in zip(gt, rt)), name
    del host16
    gc.collect()
    torch.cuda.synchronize()
    empty = getattr(torch._C, "_host_emptyCache", None)
    if empty is not None:
        empty()
    cfg, model, _, slides, _ = _setup(dev, {"model_config": {"lstm": False}})
    with pytest.raises(NotImplementedError, match="lstm=false"):
        removal_curves(model, slides, cfg.top_k_patches, 5, "importance", steps=2)
    t = []
    with torch.no_grad():
        free = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=t)
    out, _ = removal_curves(model, slides, cfg.top_k_patches, 5, "importance", trace=t, steps=2, order="morf")
    assert out["morf"].shape == (3, 3) and bool(torch.isfinite(out["morf"]).all()) and float((out["morf"][:, 0] - out["morf"][:, -1]).abs().min()) > 0


def test_launch_hygiene(dev, small, hip_trace):
    from paths_amd import utils as putils
    from paths_amd.saliency import perturbation_curves, removal_curves
    st = small
    model, slides, keep = st["model"], st["slides"], st["cfg"].top_k_patches
    scores = _fixed_scores(hip_trace, dev)
    with H.spy_calls() as calls:
        with torch.no_grad():
            putils.recurse(model, slides, keep, 5)
        perturbation_curves(model, slides, keep, 5, scores, steps=2)
    assert len(calls) > 100 and not [c for c in calls if c in NEW]
    before = [[m.clone() for m in s.masks] for s in slides]
    was = model.training
    for training in (True, False):
        model.train(training)
        with H.spy_calls() as calls:                                      # (default chunk max(1, 8 // 3) = 2: 1 + 2 * 2 free passes)
            removal_curves(model, slides, keep, 5, scores, steps=STEPS)
        assert model.training == training and all(m.training == training for m in model.modules())
    model.train(was)
    assert calls.count("paths_rank_joint") == 2 and calls.count("paths_removal_masks") == 2 * 5 + 5
    assert calls.count("paths_visited_overlap") == 5 * 5 and calls.count("paths_level0_mask_rows") == 4
    assert calls.count("paths_saliency_rows") == 5                                                   # the path pass, once
    assert calls.count("paths_topk") + calls.count("paths_topk_rows") == 4 + 5 * 4                   # ... and five free passes
    assert "paths_path_mask_points" not in calls and "paths_fallback_all_cells" not in calls
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.equal(a, b) for s, saved in zip(slides, before) for a, b in zip(s.masks, saved))   # the sources' own masks: unchanged bytes
