"""The NumPy contract of the selection chain (tests/select_ref.py) is the reference's (no GPU needed): top-K against torch.topk, an
element-loop sort and the pinned special values; expansion, fallback and gathers against the oracle's one-slide step, the fallback
branch included; the level-0 batch against the oracle's initial item; plain loops for what the oracle does not state; and the map
from every entry point of select.hip to its direct test."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from oracle import paths_oracle as orc
from tests import helpers as H
from tests import select_ref as S
from tests.test_cpu_on_demand import PATCH, SHAPES, D, _case, _oracle

FILL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# top-K
# ------------------------------------------------------------------------------------------------
def _topk_one(scores, keep, n=None, ldk=None):
    """One slide through the replica: (keep_idx row with its fill, count)."""
    n = len(scores) if n is None else n
    ldk = (len(scores) + 4) if ldk is None else ldk
    ki, kc = np.full((1, ldk), FILL, np.int32), np.full((1,), FILL, np.int32)
    S.topk(np.asarray(scores, np.float32)[None], len(scores), [n], keep, ki, kc)
    return ki[0], int(kc[0])


def _distinct_scores(rng, n):
    """n distinct finite-or-infinite float32 values: normal, negative, subnormal, +-inf, one ulp apart (no zero, no NaN)."""
    special = np.array([np.inf, -np.inf, 2.0 ** -149, -2.0 ** -149, 2.0 ** -130, 1.0, np.nextafter(np.float32(1), np.float32(2)), 3e38, -3e38],
                       np.float32)
    head = rng.permutation(special)[:min(n, len(special))]
    rest = np.setdiff1d(np.unique(rng.standard_normal(2 * n + 16).astype(np.float32)), np.append(special, np.float32(0)))
    return rng.permutation(np.concatenate([head, rng.permutation(rest)[:n - len(head)]])).astype(np.float32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 200])
def test_topk_equals_torch_topk_on_distinct_scores(n):
    rng = np.random.default_rng(n)
    sc = _distinct_scores(rng, n)
    assert len(np.unique(sc)) == n
    for keep in (1, n - 1, n, n + 1, -1):
        if keep == 0:
            continue                                     # (n = 1: keep = n - 1 is not a legal argument)
        ki, count = _topk_one(sc, keep)
        want_count = n if keep < 0 else min(n, keep)
        assert count == want_count and (ki[count:] == FILL).all()
        if keep < 0:
            np.testing.assert_array_equal(ki[:count], np.arange(n))
        else:
            np.testing.assert_array_equal(ki[:count], orc.topk_indices(torch.from_numpy(sc), want_count).numpy())


def test_topk_reads_only_the_valid_prefix_and_honours_ld():
    rng = np.random.default_rng(5)
    sc = rng.standard_normal((3, 12)).astype(np.float32)
    sc[:, 9:] = np.nan
    sc[1, 4:] = 3e38
    num = [9, 4, 0]
    ki, kc = np.full((3, 11), FILL, np.int32), np.full((3,), FILL, np.int32)
    rows = np.full((3, 11), FILL, np.int64)
    S.topk(sc, 12, num, 5, ki, kc, rows, row_base_addr=1000, row_ld=12, slide_rows=20, zero_row_addr=77)
    assert kc.tolist() == [5, 4, 0]
    for b in range(3):
        c = kc[b]
        np.testing.assert_array_equal(ki[b, :c], orc.topk_indices(torch.from_numpy(sc[b, :num[b]]), c).numpy())
        assert (ki[b, c:] == FILL).all() and (rows[b, c:] == 77).all()
        np.testing.assert_array_equal(rows[b, :c], 1000 + ((b * 20 + ki[b, :c].astype(np.int64)) * 12) * 4)


def test_topk_ties_go_to_the_lower_index():
    """Against an element loop: insertion sort by (score descending, index ascending) on rows with runs of exact ties."""
    rng = np.random.default_rng(11)
    for n, keep in ((50, 20), (130, 64), (130, 129), (9, 9)):
        sc = rng.integers(-3, 4, n).astype(np.float32) * 0.5          # seven distinct values (no zero of the other sign): long runs
        sc[sc == 0] = 0.25
        order = []
        for i in range(n):
            at = 0
            while at < len(order) and (sc[order[at]] > sc[i] or (sc[order[at]] == sc[i] and order[at] < i)):
                at += 1
            order.insert(at, i)
        ki, count = _topk_one(sc, keep)
        assert count == keep
        np.testing.assert_array_equal(ki[:count], order[:keep])


def test_topk_special_values_are_ordered_by_bit_pattern():
    """The pinned cases: +0.0 before -0.0 whatever their indices; a NaN with a clear sign bit before +inf; a NaN with the sign bit
    set after -inf.  torch.topk ranks EVERY NaN first, so the last case is where the kernel's order and the reference's differ."""
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)[0]
    pnan, nnan = f(0x7FC00000), f(0xFFC00000)
    ki, _ = _topk_one([-0.0, 0.0, -0.0, 0.0], 4)
    assert ki[:4].tolist() == [1, 3, 0, 2]
    ki, _ = _topk_one([0.0, -0.0], 2)
    assert ki[:2].tolist() == [0, 1]
    sc = np.array([1.0, -np.inf, nnan, np.inf, pnan, -1.0, 0.0], np.float32)
    ki, count = _topk_one(sc, -1)
    assert count == 7 and ki[:7].tolist() == list(range(7))
    ki, _ = _topk_one(sc, 7)
    assert ki[:7].tolist() == [4, 3, 0, 6, 5, 1, 2]
    ref = orc.topk_indices(torch.from_numpy(sc), 7).tolist()
    assert set(ref[:2]) == {2, 4} and ref[2:] == [3, 0, 6, 5, 1], "torch.topk: both NaNs first"
    # the keys themselves: strictly increasing along descending bit-pattern order, the index breaks ties
    vals = np.array([pnan, np.inf, 3e38, 1.0, 2.0 ** -149, 0.0, -0.0, -2.0 ** -149, -1.0, -np.inf, nnan], np.float32)
    keys = S.topk_key(vals, np.zeros(len(vals), np.int64))
    assert (np.diff(keys.astype(object)) > 0).all()
    two = S.topk_key(np.array([2.5, 2.5], np.float32), [3, 4])
    assert int(two[0]) < int(two[1]) and int(two[0]) & 0xFFFFFFFF == 3 and int(two[0]) >> 32 == 0xFFFFFFFF ^ 0xC0200000


def test_topk_argument_check():
    assert S.check_topk_args(1, 8192, 512, 512) == 0 and S.check_topk_args(1, 8193, 512, 512) == -1
    assert S.check_topk_args(1, 100, 0, 100) == -1 and S.check_topk_args(1, 100, -1, 99) == -1 and S.check_topk_args(1, 100, 50, 49) == -1
    assert S.check_topk_args(1, 100, 50, 8193) == -1 and S.check_topk_args(0, 100, 50, 50) == -1 and S.check_topk_args(1, 9, 64, 9) == 0


# ------------------------------------------------------------------------------------------------
# expansion, fallback and gathers against the oracle's one-slide step
# ------------------------------------------------------------------------------------------------
def _oracle_with_ctx(c, ctx):
    n = c["n"]
    z = torch.zeros
    item, keep_inds = orc.iter_slide(c["grids"], 0, n, torch.from_numpy(c["locs"]), z(0, 4), z(n, 0, 4), z(4), torch.from_numpy(ctx),
                                     torch.from_numpy(c["imp"]), c["keep"], PATCH)
    return item, keep_inds.numpy()


def _chain(cases, ctxs):
    """top-K -> expansion -> fallback -> gather of the replica, all slides in one call each (capacities sized for the fallback)."""
    B = len(cases)
    n_cur = max(c["n"] for c in cases)
    ldk = n_cur
    imp = np.full((B, n_cur + 2), np.nan, np.float32)
    locs = np.zeros((B, n_cur, 2), np.int64)
    state = np.zeros((B, n_cur, 4), np.float32)
    for b, c in enumerate(cases):
        imp[b, :c["n"]], locs[b, :c["n"]], state[b, :c["n"]] = c["imp"], c["locs"], ctxs[b]
    num_ims = np.array([c["n"] for c in cases], np.int64)
    keeps = {c["keep"] for c in cases}
    keep_idx, keep_count = np.full((B, ldk), 0, np.int32), np.full((B,), FILL, np.int32)
    for keep in keeps:                                  # (one launch has one keep: slides of another are overwritten in their turn)
        ki, kc = np.full((B, ldk), 0, np.int32), np.full((B,), FILL, np.int32)
        S.topk(imp, n_cur + 2, num_ims, keep, ki, kc)
        for b, c in enumerate(cases):
            if c["keep"] == keep:
                keep_idx[b], keep_count[b] = ki[b], kc[b]
    grids = [c["grids"].grids[1].numpy() for c in cases]
    nx = np.array([g.shape[0] for g in grids], np.int32)
    ny = np.array([g.shape[1] for g in grids], np.int32)
    flat = [g.reshape(-1, D) for g in grids]
    masks = [S.tissue_mask(f).reshape(g.shape[:2]) for f, g in zip(flat, grids)]
    n_next = max(4 * ldk, int((nx * ny).max()))
    out = dict(num_out=np.full((B,), FILL, np.int64), locs_out=np.full((B, n_next, 2), FILL, np.int64), parent_out=np.full((B, n_next), FILL, np.int64),
               src_row=np.full((B, n_next), FILL, np.int32), src_cell=np.full((B, n_next), FILL, np.int32),
               hp_row=np.full((B, n_next), FILL, np.int32))
    status = S.expand_children(keep_idx, keep_count, locs, PATCH, nx, ny, masks, n_next, **out)
    fell = out["num_out"] == 0
    assert bool(status & 1) == bool(fell.any()) and not status & 2
    assert S.fallback_all_cells(nx, ny, masks, PATCH, n_next, **out) == 0
    fts = np.full((B, n_next, D), np.nan, np.float32)
    ctx = np.full((B, n_next, 4), np.nan, np.float32)
    S.gather_rows(flat, [0] * B, out["src_cell"], out["src_row"], out["num_out"], state_cur=state, n_cur=n_cur, ld_state_cur=4, Dp=4,
                  fts_out=fts, state_out=ctx, zero_pad=1)
    return out, fell, keep_idx, keep_count, fts, ctx, masks, ldk


def _some_tissue_but_none_among_the_children(rng):
    """A next grid whose only background rows are the children of the two kept patches: the oracle falls back to its TISSUE cells."""
    c = _case(rng, 3, 3, (1, 0), 5, 2, p_bg=0.0)
    kept = c["locs"][np.argsort(-c["imp"])[:2]] // PATCH
    g = c["grids"].grids[1]
    for x, y in kept:
        g[2 * x:2 * x + 2, 2 * y:2 * y + 2] = 0
    return c


@pytest.mark.parametrize("seed", range(6))
def test_chain_equals_the_oracle_step(seed):
    """The cases of the on-demand contract test (odd next grids, keep = -1, a keep above the level) and the oracle's FALLBACK branch,
    which that test skips: a next grid without any tissue (every cell is taken) and one with tissue only outside the kept patches'
    children (its tissue cells are taken)."""
    rng = np.random.default_rng(200 + seed)
    cases = [_case(rng, *shape, odd, n, keep, p_bg=rng.choice([0.1, 0.5])) for shape, odd, n, keep in SHAPES]
    dead = _case(rng, 3, 3, (1, 0), 5, 2, p_bg=2.0)
    part = _some_tissue_but_none_among_the_children(rng)
    cases.insert(seed % len(cases), dead)
    cases.insert((3 * seed + 1) % len(cases), part)
    ctxs = [rng.standard_normal((c["n"], 4)).astype(np.float32) for c in cases]
    oracle = [_oracle_with_ctx(c, x) for c, x in zip(cases, ctxs)]
    out, fell, keep_idx, keep_count, fts, ctx, masks, ldk = _chain(cases, ctxs)
    for b, (c, (item, keep_inds)) in enumerate(zip(cases, oracle)):
        k = int(out["num_out"][b])
        np.testing.assert_array_equal(keep_idx[b, :keep_count[b]], keep_inds, err_msg="top-K")
        assert bool(fell[b]) == item["fallback"] and (item["fallback"] or (c is not dead and c is not part))
        assert k == item["locs"].shape[0] > 0
        np.testing.assert_array_equal(out["locs_out"][b, :k], item["locs"].numpy())
        np.testing.assert_array_equal(out["parent_out"][b, :k], item["parent_inds"].numpy())
        np.testing.assert_array_equal(fts[b, :k], item["fts"].numpy())
        np.testing.assert_array_equal(ctx[b, :k], item["ctx_patch"][:, 0].numpy())
        assert (fts[b, k:] == 0).all() and (ctx[b, k:] == 0).all(), "zero_pad"
        Y = masks[b].shape[1]
        np.testing.assert_array_equal(out["src_cell"][b, :k], (item["locs"][:, 0].numpy() // PATCH) * Y + item["locs"][:, 1].numpy() // PATCH)
        if item["fallback"]:
            # parent_inds are CELL indices, the context is fresh, and the rows are the grid's tissue cells (all cells if it has none)
            want = np.nonzero(masks[b].reshape(-1))[0] if masks[b].any() else np.arange(masks[b].size)
            np.testing.assert_array_equal(out["parent_out"][b, :k], want)
            assert (out["src_row"][b, :k] == -1).all() and (out["hp_row"][b, :k] == -1).all() and (ctx[b, :k] == 0).all()
            assert (c is dead) <= (k == masks[b].size) and (c is part) <= (0 < k < masks[b].size)
        else:
            np.testing.assert_array_equal(out["src_row"][b, :k], keep_inds[item["parent_inds"].numpy()])
            np.testing.assert_array_equal(out["hp_row"][b, :k], b * ldk + item["parent_inds"].numpy())
            assert (out["src_row"][b, k:] == -1).all() and (out["src_cell"][b, k:] == -1).all() and (out["locs_out"][b, k:] == 0).all()


def test_expansion_reports_exceeded_capacity_and_clamps_keep_count():
    rng = np.random.default_rng(3)
    c = _case(rng, 4, 4, (0, 0), 16, -1, p_bg=0.0)
    keep_idx = np.tile(np.arange(16, dtype=np.int32), (3, 1))
    locs = np.tile(c["locs"][None], (3, 1, 1))
    masks = [np.ones((8, 8), np.uint8)] * 3
    mk = lambda n: dict(num_out=np.full((3,), FILL, np.int64), locs_out=np.full((3, n, 2), FILL, np.int64), parent_out=np.full((3, n), FILL, np.int64),
                        src_row=np.full((3, n), FILL, np.int32), src_cell=np.full((3, n), FILL, np.int32), child_pos=np.full((3, 64), FILL, np.int32))
    out = mk(10)
    assert S.expand_children(keep_idx, np.array([16, 2, -3], np.int32), locs, PATCH, [8] * 3, [8] * 3, masks, 10, **out) == 3
    assert out["num_out"].tolist() == [64, 8, 0]
    assert all((v[0] == FILL).all() for k, v in out.items() if k != "num_out"), "over capacity: num_out only"
    assert (out["src_row"][1, :8] >= 0).all() and (out["src_row"][1, 8:] == -1).all() and (out["src_row"][2] == -1).all()
    assert (out["child_pos"][1, :8] >= 0).all() and (out["child_pos"][1, 8:] == FILL).all() and (out["child_pos"][2] == FILL).all()
    big, clamped = mk(64), mk(64)
    S.expand_children(keep_idx, np.array([21, 16, 16], np.int32), locs, PATCH, [8] * 3, [8] * 3, masks, 64, **big)
    S.expand_children(keep_idx, np.array([16, 16, 16], np.int32), locs, PATCH, [8] * 3, [8] * 3, masks, 64, **clamped)
    assert all(np.array_equal(big[k], clamped[k]) for k in big), "keep_count above ldk behaves as ldk"
    assert S.check_expand_args(1, 4, 8, PATCH, 16) == 0
    for bad in ((0, 4, 8, PATCH, 16), (1, 0, 8, PATCH, 16), (1, 4, 0, PATCH, 16), (1, 4, 8, 0, 16), (1, 4, 8, PATCH, 0), (1, 4, 8, PATCH, 1 << 29)):
        assert S.check_expand_args(*bad) == -1
    assert S.check_fallback_args(1, 8, PATCH) == 0 and S.check_fallback_args(0, 8, PATCH) == S.check_fallback_args(1, 0, PATCH) == \
        S.check_fallback_args(1, 8, 0) == -1


def test_level0_batch_equals_the_oracle_initial_items():
    rng = np.random.default_rng(9)
    cfg = H.oracle_config(patch_embed_dim=D, lstm=False)
    shapes = [(3, 5), (2, 2)]
    grids = [rng.standard_normal((X, Y, D)).astype(np.float32) for X, Y in shapes]
    want = orc.collate([orc.initial_item(orc.DenseGrids([torch.from_numpy(g)]), cfg) for g in grids])
    n0 = 15
    fts, locs, parent = np.full((2, n0, D), np.nan, np.float32), np.full((2, n0, 2), FILL, np.int64), np.full((2, n0), FILL, np.int64)
    num, ptrs = np.full((2,), FILL, np.int64), np.full((2, n0), FILL, np.int64)
    S.level0_batch([g.reshape(-1, D) for g in grids], [4096, 8192], [3, 2], [5, 2], cfg.patch_size, locs, parent, num, fts=fts, zero_pad=1,
                   row_ptrs=ptrs, zero_row_addr=64)
    np.testing.assert_array_equal(fts, want["fts"].numpy())
    np.testing.assert_array_equal(locs, want["locs"].numpy())
    np.testing.assert_array_equal(parent, want["parent_inds"].numpy())
    np.testing.assert_array_equal(num, want["num_ims"].numpy())
    assert ptrs[0].tolist() == [4096 + j * D * 4 for j in range(15)] and ptrs[1].tolist() == [8192 + j * D * 4 for j in range(4)] + [64] * 11
    keep = np.full((2, n0, D), np.nan, np.float32)
    S.level0_batch([g.reshape(-1, D) for g in grids], [0, 0], [3, 2], [5, 2], cfg.patch_size, locs, parent, num, fts=keep, zero_pad=0)
    assert np.isnan(keep[1, 4:]).all() and np.array_equal(keep[1, :4], fts[1, :4]), "without zero_pad the padding copies are untouched"


# ------------------------------------------------------------------------------------------------
# element loops for what the oracle does not state
# ------------------------------------------------------------------------------------------------
def test_fallback_against_an_element_loop():
    """Touched slides only; tissue cells row-major or every cell; the tail keeps the fill; over capacity writes num_out only."""
    rng = np.random.default_rng(21)
    shapes = [(7, 5), (3, 4), (2, 2), (6, 6), (1, 1)]
    masks = [(rng.random(s) < 0.4).astype(np.uint8) for s in shapes]
    masks[3][:] = 0
    masks[4][:] = 1
    nx, ny = [s[0] for s in shapes], [s[1] for s in shapes]
    for n_next, hp in ((36, True), (35, True), (36, False)):
        mk = lambda: dict(num_out=np.array([0, 0, 3, 0, 0], np.int64), locs_out=np.full((5, n_next, 2), FILL, np.int64),
                          parent_out=np.full((5, n_next), FILL, np.int64), src_row=np.full((5, n_next), FILL, np.int32),
                          src_cell=np.full((5, n_next), FILL, np.int32), **({"hp_row": np.full((5, n_next), FILL, np.int32)} if hp else {}))
        got, want = mk(), mk()
        status = S.fallback_all_cells(nx, ny, masks, PATCH, n_next, **got)
        want_status = 0
        for b in range(5):
            if b == 2:
                continue
            cells = [(x, y) for x in range(nx[b]) for y in range(ny[b]) if masks[b][x, y]]
            if not cells:
                cells = [(x, y) for x in range(nx[b]) for y in range(ny[b])]
            want["num_out"][b] = len(cells)
            if len(cells) > n_next:
                want_status |= 2
                continue
            for pos, (x, y) in enumerate(cells):
                want["locs_out"][b, pos] = (x * PATCH, y * PATCH)
                want["parent_out"][b, pos] = want["src_cell"][b, pos] = x * ny[b] + y
                want["src_row"][b, pos] = -1
                if hp:
                    want["hp_row"][b, pos] = -1
        assert status == want_status == (2 if n_next == 35 else 0)
        for k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert got["num_out"].tolist()[2:] == [3, 36, 1] and (got["locs_out"][2] == FILL).all()
        assert (got["src_row"][4, 1:] == FILL).all(), "rows beyond n_out are not rewritten"


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("zero_pad", [0, 1])
def test_gather_padding_rules_against_an_element_loop(dtype, zero_pad):
    rng = np.random.default_rng(4)
    B, n_next, n_cur, Dp, ld, off = 3, 5, 4, 4, 12, 8
    grids = [rng.standard_normal((c, D)).astype(dtype) for c in (6, 3, 2)]
    addrs = [1 << 20, 1 << 21, 1 << 22]
    num_out = [0, 3, 5]
    src_cell = np.stack([rng.integers(0, len(g), n_next) for g in grids]).astype(np.int32)
    src_row = rng.integers(-1, n_cur, (B, n_next)).astype(np.int32)
    src_row[2, 1] = -1
    state = rng.standard_normal((B, n_cur, ld)).astype(np.float32)
    fts, st, ptrs = np.full((B, n_next, D), np.nan, np.float32), np.full((B, n_next, Dp), np.nan, np.float32), np.full((B, n_next), FILL, np.int64)
    S.gather_rows(grids, addrs, src_cell, src_row, num_out, state_cur=state, n_cur=n_cur, ld_state_cur=ld, state_off=off, Dp=Dp, fts_out=fts,
                  state_out=st, zero_pad=zero_pad, row_ptrs=ptrs, zero_row_addr=99)
    for b in range(B):
        for j in range(n_next):
            if j < num_out[b]:
                assert ptrs[b, j] == addrs[b] + int(src_cell[b, j]) * D * np.dtype(dtype).itemsize
                for e in range(D):
                    assert fts[b, j, e] == np.float32(grids[b][src_cell[b, j], e])
                for e in range(Dp):
                    assert st[b, j, e] == (state[b, src_row[b, j], off + e] if src_row[b, j] >= 0 else 0.0)
            else:
                assert ptrs[b, j] == 99
                assert ((fts[b, j] == 0).all() and (st[b, j] == 0).all()) if zero_pad else (np.isnan(fts[b, j]).all() and np.isnan(st[b, j]).all())
    only = np.full((B, n_next), FILL, np.int64)
    S.gather_rows(grids, addrs, src_cell, src_row, num_out, row_ptrs=only, zero_row_addr=99)
    np.testing.assert_array_equal(only, ptrs)


@pytest.mark.parametrize("Dm", [4, 8, 64, 1024])
def test_tissue_mask_on_the_special_rows(Dm):
    rows, verdict = S.tissue_special_rows(Dm)
    loop = []
    for r in rows:
        s = np.float32(0)
        with np.errstate(invalid="ignore"):
            for v in r:
                s = np.float32(s + v)
        loop.append(0 if s == 0 else 1)
    assert loop == verdict.tolist() == S.tissue_mask(rows).tolist()
    assert S.tissue_mask(rows[:, ::-1]).tolist() == verdict.tolist(), "no verdict depends on the order of the sum"
    half = rows.astype(np.float16)
    assert S.tissue_mask(half).tolist() == [0, 0, 1, 0, 0, 0, 1, 1], "2^-149 is not an fp16 value; every other row is"
    assert np.isnan(np.array([S.absmax_bits(rows)], np.uint32).view(np.float32)[0])
    assert S.absmax_bits(rows[:6]) == int(np.array([1.5], np.float32).view(np.uint32)[0]) and S.absmax_bits(rows[:2]) == 0
    assert S.absmax_bits(rows[7:]) == 0x7F800000


def test_scale_add_rows_replica():
    x, h = np.arange(24, dtype=np.float32).reshape(6, 4), np.ones((6, 4), np.float32)
    alpha = np.array([2, 3, 4, 5, 6, 7], np.float32)
    z = S.scale_add_rows(x, alpha, h, [2, 0], 3, 1)
    for r in range(6):
        for e in range(4):
            assert z[r, e] == float(alpha[r]) * float(x[r, e]) + (1.0 if r in (0, 1) else 0.0)
    assert np.array_equal(S.scale_add_rows(x, None, None, [2, 0], 3, 0), x.astype(np.float64))


# ------------------------------------------------------------------------------------------------
# coverage: every entry point of select.hip has a direct test
# ------------------------------------------------------------------------------------------------
HERE = "tests/test_gpu_select.py"
ROWS = "tests/test_gpu_row_backward.py"
OND = "tests/test_gpu_on_demand.py"
PACKED = "tests/test_gpu_packed_slides.py"
SELECT_DIRECT_TESTS = {
    "paths_topk": HERE + "::test_topk_equals_the_numpy_contract",
    "paths_topk_rows": HERE + "::test_topk_equals_the_numpy_contract",
    "paths_expand_children": HERE + "::test_expand_kernel_equals_the_numpy_contract",
    "paths_fallback_all_cells": HERE + "::test_fallback_kernel_equals_the_numpy_contract",
    "paths_gather_rows": HERE + "::test_gather_kernel_equals_the_numpy_contract",
    "paths_gather_rows_h16": HERE + "::test_gather_kernel_equals_the_numpy_contract",
    "paths_level0_batch": HERE + "::test_level0_kernel_equals_the_numpy_contract",
    "paths_level0_batch_h16": HERE + "::test_level0_kernel_equals_the_numpy_contract",
    "paths_gather_rows_packed": PACKED + "::test_packed_gather_equals_its_dense_twin",
    "paths_gather_rows_packed_h16": PACKED + "::test_packed_gather_equals_its_dense_twin",
    "paths_level0_batch_packed": PACKED + "::test_packed_level0_equals_its_dense_twin",
    "paths_level0_batch_packed_h16": PACKED + "::test_packed_level0_equals_its_dense_twin",
    "paths_tissue_mask": HERE + "::test_tissue_kernels_on_the_special_rows",
    "paths_scale_add_rows": HERE + "::test_scale_add_rows_vs_fp64",
    "paths_tissue_mask_absmax": OND + "::test_row_predicate_over_a_candidate_buffer",
    "paths_tissue_mask_absmax_h16": OND + "::test_row_predicate_over_a_candidate_buffer",
    "paths_candidate_children": OND + "::test_candidate_kernel_equals_the_numpy_contract",
    "paths_admit_children": OND + "::test_admit_kernel_equals_the_numpy_contract",
    "paths_gather_kept_rows": ROWS + "::test_gradients_between_levels_are_bitwise_fp32_block_sums",
    "paths_gather_rows_bwd": ROWS + "::test_gradients_between_levels_are_bitwise_fp32_block_sums",
    "paths_sibling_sum": ROWS + "::test_gradients_between_levels_are_bitwise_fp32_block_sums",
    "paths_scatter_kept_rows": ROWS + "::test_gradients_between_levels_are_bitwise_fp32_block_sums",
    "paths_synth_grid": "tests/test_gpu_parity.py::test_synth_grid_bit_exact_and_mask",
    "paths_synth_grid_h16": "tests/test_gpu_half_grids.py::test_fp16_synthetic_grids_match_the_host_replica",
}


def test_every_entry_point_of_select_hip_has_a_direct_test():
    """A new selection kernel needs a direct test before it ships."""
    with open(os.path.join(ROOT, "paths_amd", "csrc", "select.hip")) as f:
        src = f.read()
    block = src[src.index('extern "C" {'):]
    names = re.findall(r"^int (paths_\w+)\(", block, flags=re.M)
    assert len(names) >= 20 and len(set(names)) == len(names)
    missing = sorted(set(names) - set(SELECT_DIRECT_TESTS))
    assert not missing, f"entry points of select.hip without a direct test: {missing}"
    assert not set(SELECT_DIRECT_TESTS) - set(names), "the map names an entry point select.hip does not define"


def test_select_direct_test_map_names_real_tests():
    for name, tid in SELECT_DIRECT_TESTS.items():
        path, test = tid.split("::")
        assert os.path.isfile(os.path.join(ROOT, path)), tid
        mod = importlib.import_module(path[:-3].replace("/", "."))
        assert callable(getattr(mod, test, None)), tid
