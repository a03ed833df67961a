"""CPU side of the removal curves on the free path (paths_amd/saliency.py:removal_curves): the properties of the numpy
restatement of the two kernels (tests/removal_ref.py), the count formula, the argument checks of removal_curves and with_masks, and
the host-side argument validation of the entry points."""
import types

import numpy as np
import pytest
import torch

from tests import perturb_ref as P
from tests import removal_ref as M

PS = 256
SHAPES = ((5, 9), (10, 18), (20, 36))                       # three levels of a non-square pyramid
SEG = (45, 40, 64)                                          # the levels' row capacities
NUMS = np.array([[45, 45], [0, 37], [64, 19]])              # [L, B]


def _setting(seed):
    """Per level: source masks (about a fifth background), locations of distinct cells (garbage on padded rows), and one joint
    rank by distinct scores."""
    g = np.random.default_rng(seed)
    src, locs = [], []
    for (X, Y), n, num in zip(SHAPES, SEG, NUMS):
        src.append([(g.random((X, Y)) > 0.2).astype(np.uint8) for _ in range(2)])
        lc = np.full((2, n, 2), -(1 << 40), np.int64)
        for b in range(2):
            cells = g.permutation(X * Y)[:num[b]]
            lc[b, :num[b], 0], lc[b, :num[b], 1] = (cells // Y) * PS + g.integers(0, PS, num[b]), (cells % Y) * PS
        locs.append(lc)
    scores = g.standard_normal((2, sum(SEG))).astype(np.float32)
    scores[~P.valid_mask(SEG, NUMS)] = np.nan
    return src, locs, scores


def _split(rank):
    off = np.cumsum((0,) + SEG)
    return [rank[:, a:b] for a, b in zip(off[:-1], off[1:])]


def test_counts_formula():
    from paths_amd.saliency import removal_counts
    n = [0, 1, 19, 130, 34816]
    for steps in (1, 4, 8):
        for frac in (0.5, 1.0, 0.3, 1e-3):
            c = M.counts(n, steps, frac)
            np.testing.assert_array_equal(removal_counts(n, steps, frac), c)
            m = np.floor(frac * np.asarray(n)).astype(np.int64)
            assert (c[0] == 0).all() and (c[steps] == m).all() and (np.diff(c, axis=0) >= 0).all()
            assert all(abs(int(c[s, j]) - s * int(m[j]) / steps) <= 0.5 for s in range(steps + 1) for j in range(len(n)))
    np.testing.assert_array_equal(M.counts(n, 4, 1.0), P.counts(n, 4))


@pytest.mark.parametrize("ascending", [False, True])
def test_members_are_nested_clear_their_counts_and_left_is_the_popcount(ascending):
    src, locs, scores = _setting(3)
    rank, n = P.rank_joint(scores, SEG, NUMS, None, ascending)
    steps = 4
    thr = M.counts(n, steps, 0.5)
    cleared = np.zeros((steps + 1, 2), np.int64)
    for l, rk in enumerate(_split(rank)):
        pick = M.chosen(NUMS[l], rk, thr)
        masks, left = M.removal_masks(src[l], locs[l], PS, pick)
        for s in range(steps + 1):
            for b in range(2):
                m = masks[s][b]
                assert m.dtype == np.uint8 and m.shape == SHAPES[l] and left[s, b] == np.count_nonzero(m)
                assert not (m & ~src[l][b]).any()                                        # nothing is ever set
                if s:
                    assert not (m & ~masks[s - 1][b]).any()                              # nested in s
                gone = np.zeros(SHAPES[l], bool)
                r = np.nonzero(pick[s, b])[0]
                gone[locs[l][b, r, 0] // PS, locs[l][b, r, 1] // PS] = True
                assert gone.sum() == len(r)                                              # (two valid rows never share a cell)
                assert ((m != 0) == ((src[l][b] != 0) & ~gone)).all()
                cleared[s, b] += len(r)
        assert (np.array([[np.count_nonzero(x) for x in row] for row in masks[:1]]) == [[np.count_nonzero(x) for x in src[l]]]).all()
    np.testing.assert_array_equal(cleared, thr)                                          # over all levels: exactly counts[s, b] cells


def test_overlap_of_a_pass_with_itself_is_num_ims():
    src, locs, _ = _setting(5)
    for l, (X, Y) in enumerate(SHAPES):
        zero = [np.zeros((X, Y), np.uint8)] * 2
        bm, left = M.removal_masks(zero, locs[l], PS, M.all_valid(NUMS[l], SEG[l]), set_cells=True)
        assert left[0].tolist() == NUMS[l].tolist()
        ov = M.visited_overlap(bm[0], np.concatenate([locs[l]] * 3), np.tile(NUMS[l], 3), PS)
        assert ov.dtype == np.int32 and ov.tolist() == NUMS[l].tolist() * 3
        # a member that keeps only its first rows overlaps by that many; against the other slide's bitmap the count is the cells shared
        ov = M.visited_overlap(bm[0], locs[l], np.minimum(NUMS[l], 7), PS)
        assert ov.tolist() == np.minimum(NUMS[l], 7).tolist()


def test_morf_on_v_is_lerf_on_minus_v():
    src, locs, scores = _setting(9)
    r1, n = P.rank_joint(scores, SEG, NUMS, None, False)
    r2, _ = P.rank_joint(-scores, SEG, NUMS, None, True)
    thr = M.counts(n, 4, 0.7)
    differs = False
    for l, (a, b) in enumerate(zip(_split(r1), _split(r2))):
        m1, l1 = M.removal_masks(src[l], locs[l], PS, M.chosen(NUMS[l], a, thr))
        m2, l2 = M.removal_masks(src[l], locs[l], PS, M.chosen(NUMS[l], b, thr))
        assert all((x == y).all() for ra, rb in zip(m1, m2) for x, y in zip(ra, rb)) and (l1 == l2).all()
        r3 = _split(P.rank_joint(scores, SEG, NUMS, None, True)[0])[l]
        differs = differs or (M.chosen(NUMS[l], a, thr) != M.chosen(NUMS[l], r3, thr)).any()
    assert differs                                                                        # (lerf on v itself is another curve)


def test_argument_errors_come_before_the_device():
    from paths_amd import saliency
    from paths_amd.data_utils import slide as S
    model = types.SimpleNamespace(use_lstm=True)
    fn = saliency.removal_curves
    with pytest.raises(NotImplementedError, match="lstm=false"):
        fn(types.SimpleNamespace(use_lstm=False), [], [2], 2, "importance")
    od = [S.OnDemandSlide([(2, 2)], lambda l, c: torch.zeros(len(c), 8), 8, "cpu")]
    with pytest.raises(NotImplementedError, match="on-demand"):
        fn(model, od, [2], 2, "importance")
    with pytest.raises(ValueError, match="unknown target"):
        fn(model, [], [2], 2, "importance", target="hazard")
    for steps in (0, -3, 2.0):
        with pytest.raises(ValueError, match="steps"):
            fn(model, [], [2], 2, "importance", steps=steps)
    for order in ("deletion", "insertion", None):
        with pytest.raises(ValueError, match="order"):
            fn(model, [], [2], 2, "importance", order=order)
    for frac in (0, 0.0, -0.5, 1.5, "half", True, float("nan")):
        with pytest.raises(ValueError, match="max_fraction"):
            fn(model, [], [2], 2, "importance", max_fraction=frac)
    for levels in ([2], [-1], [0, 5]):
        with pytest.raises(ValueError, match="levels"):
            fn(model, [], [2], 2, "importance", levels=levels)
    for chunk in (0, 1.5):
        with pytest.raises(ValueError, match="chunk"):
            fn(model, [], [2], 2, "importance", chunk=chunk)
    for bad in ([torch.zeros(1, 4)], torch.zeros(2, 1, 4), 3):
        with pytest.raises(ValueError, match="scores"):
            fn(model, [], [2], 2, bad)
    for bad in ([{}], [{}, {}]):
        with pytest.raises(ValueError, match="trace"):
            fn(model, [], [2], 2, "importance", trace=bad)
    # a given trace needs no gradient: lstm = false gets past the variant check (and stops at the trace's own)
    with pytest.raises(ValueError, match="trace"):
        fn(types.SimpleNamespace(use_lstm=False), [], [2], 2, "importance", trace=[{}])


def _host_side_slide(cls):
    """A slide object with the read surface with_masks needs, built without a device: two levels, 2 x 3 and 4 x 6."""
    masks = [torch.ones(2, 3, dtype=torch.uint8), torch.ones(4, 6, dtype=torch.uint8)]
    return cls._new(torch.float32, torch.device("cpu"), masks, grids=[torch.zeros(2, 3, 8), torch.zeros(4, 6, 8)], absmax=1.5, slide_id="x")


@pytest.mark.parametrize("kind", ["DeviceSlide", "HostSlide"])
def test_with_masks_checks_and_shares(kind):
    from paths_amd.data_utils import slide as S
    s = _host_side_slide(getattr(S, kind))
    good = [torch.zeros(2, 3, dtype=torch.uint8), torch.ones(4, 6, dtype=torch.uint8)]
    v = s.with_masks(good)
    assert type(v) is type(s) and v.masked_view and not s.masked_view and v.host_resident == s.host_resident
    assert all(a is b for a, b in zip(v.grids, s.grids)) and v.grids is s.grids          # shared, not copied
    assert all(a is b for a, b in zip(v.masks, good)) and s.masks[0].all()               # the source keeps its own masks
    assert v.dtype == s.dtype and v.patch_size == s.patch_size and v.feature_absmax() == s.feature_absmax() == 1.5
    assert v.num_levels == 2 and v.shape(1) == (4, 6) and v.dim == 8
    assert v.with_masks(s.masks).masked_view                                             # a view of a view
    for bad, what in (([good[0]], "one mask per level"), ([good[0], good[1].float()], "uint8"), ([good[0], torch.ones(6, 4, dtype=torch.uint8)], "uint8"),
                      ([good[0], torch.ones(4, 12, dtype=torch.uint8)[:, ::2]], "contiguous"), ([good[0], np.ones((4, 6), np.uint8)], "uint8"),
                      ([good[0], torch.ones(4, 6, dtype=torch.uint8, device="meta")], "lives on")):
        with pytest.raises(ValueError, match=what):
            s.with_masks(bad)


def test_on_demand_slides_have_no_masked_views():
    from paths_amd.data_utils import slide as S
    od = S.OnDemandSlide([(2, 2)], lambda l, c: torch.zeros(len(c), 8), 8, "cpu")
    with pytest.raises(NotImplementedError, match="with_masks"):
        od.with_masks([torch.ones(2, 2, dtype=torch.uint8)])


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    assert lib.paths_abi_version() == 3
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)
    rm = lambda src, gx, gy, mc, locs, ps, ni, rk, ldr, thr, N, B, C, st, masks, ldm, left: lib.paths_removal_masks(
        src, gx, gy, mc, locs, ps, ni, rk, ldr, thr, N, B, C, st, masks, ldm, left, None)
    ok = dict(src=A, gx=A, gy=A, mc=45, locs=A, ps=256, ni=A, rk=A, ldr=40, thr=A, N=40, B=2, C=3, st=0, masks=A, ldm=48, left=A)
    for change, word in ((dict(masks=None), b"null"), (dict(left=None), b"null"), (dict(locs=None), b"null"), (dict(rk=None), b"come together"),
                         (dict(thr=None), b"come together"), (dict(N=0), b"positive"), (dict(ps=0), b"positive"), (dict(B=0), b"B (0)"),
                         (dict(C=70000), b"C (70000)"), (dict(mc=0), b"max_cells"), (dict(ldm=45), b"multiple of 16"), (dict(ldm=32), b"multiple of 16"),
                         (dict(ldr=39), b"rank stride"), (dict(masks=A + 8), b"aligned"), (dict(rk=A + 2), b"aligned"), (dict(locs=A + 4), b"aligned")):
        assert rm(**{**ok, **change}) == -1 and word in lib.paths_last_error(), (change, lib.paths_last_error())
    vo = lambda bm, ldb, gx, gy, locs, nm, ps, Nm, B, C, ov: lib.paths_visited_overlap(bm, ldb, gx, gy, locs, nm, ps, Nm, B, C, ov, None)
    ok = dict(bm=A, ldb=48, gx=A, gy=A, locs=A, nm=A, ps=256, Nm=40, B=2, C=3, ov=A)
    for change, word in ((dict(bm=None), b"null"), (dict(ov=None), b"null"), (dict(Nm=0), b"positive"), (dict(ldb=0), b"positive"),
                         (dict(B=0), b"B (0)"), (dict(C=0), b"C (0)"), (dict(ov=A + 2), b"aligned"), (dict(nm=A + 4), b"aligned")):
        assert vo(**{**ok, **change}) == -1 and word in lib.paths_last_error(), (change, lib.paths_last_error())
    l0 = lambda mp, gx, gy, B, D, n0, fts, rows, zero: lib.paths_level0_mask_rows(mp, gx, gy, B, D, n0, fts, rows, zero, None)
    assert l0(None, A, A, 2, 128, 45, A, None, None) == -1 and b"null" in lib.paths_last_error()
    assert l0(A, A, A, 2, 126, 45, A, None, None) == -1 and b"bad shape" in lib.paths_last_error()
    assert l0(A, A, A, 2, 128, 45, None, None, None) == -1 and b"copy" in lib.paths_last_error()
    assert l0(A, A, A, 2, 128, 45, None, A, None) == -1 and b"zero row" in lib.paths_last_error()
    with pytest.raises(_lib.PathsHipError, match=r"paths_visited_overlap failed \(-1\)"):
        _lib.call("paths_visited_overlap", None, 0, None, None, None, None, 0, 0, 0, 0, None, None)


def test_removed_map_paints_the_members_cells():
    from paths_amd import heatmap as hm
    lv = [{"locs": np.array([[0, 0], [256, 512]]), "removal_rank_morf": np.array([1, 0], np.int32)},
          {"locs": np.array([[0, 256], [512, 0], [768, 1280]]), "removal_rank_morf": np.array([2, -1, 3], np.int32)}]
    maps = hm.removed_map(lv, (2, 3), 3)
    assert [m.dtype for m in maps] == [np.uint8] * 2 and [m.shape for m in maps] == [(4, 6)] * 2
    want0 = np.zeros((4, 6), np.uint8)
    want0[0:2, 0:2] = 1
    want0[2:4, 4:6] = 1
    want1 = np.zeros((4, 6), np.uint8)
    want1[0, 1] = 1                                                       # rank 2 < 3; rank -1 (not ranked) and rank 3 stay
    assert (maps[0] == want0).all() and (maps[1] == want1).all()
    assert not any(m.any() for m in hm.removed_map(lv, (2, 3), 0))
    with pytest.raises(KeyError, match="removal_rank_lerf"):
        hm.removed_map(lv, (2, 3), 1, order="lerf")
    with pytest.raises(ValueError, match="order"):
        hm.removed_map(lv, (2, 3), 1, order="both")
