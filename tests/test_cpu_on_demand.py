"""On-demand slides, host side (no GPU needed): the NumPy statement of the two selection kernels' contracts composed around a tissue
lookup against the oracle's one-slide step, and OnDemandSlide's argument checks and request bookkeeping."""
import types

import numpy as np
import pytest
import torch

from oracle import paths_oracle as orc
from paths_amd.data_utils import slide as S
from tests import on_demand_ref as R

PATCH, D = 256, 8


def _case(rng, X, Y, odd, npatches, keep, p_bg):
    """One slide at a level of X x Y cells: ``npatches`` distinct cells with random importances, a next grid of (2X - odd[0]) x
    (2Y - odd[1]) cells whose rows are background with probability ``p_bg``."""
    cells = rng.permutation(X * Y)[:npatches]
    locs = np.stack([cells // Y, cells % Y], axis=1).astype(np.int64) * PATCH
    imp = rng.permutation(npatches).astype(np.float32) / npatches             # distinct: top-K has one answer
    nX, nY = 2 * X - odd[0], 2 * Y - odd[1]
    nxt = rng.standard_normal((nX, nY, D)).astype(np.float32)
    nxt[rng.random((nX, nY)) < p_bg] = 0
    return dict(locs=locs, imp=imp, keep=keep, grids=orc.DenseGrids([torch.zeros(X, Y, D), torch.from_numpy(nxt)]), n=npatches)


def _oracle(c):
    n = c["n"]
    z = torch.zeros
    item, keep_inds = orc.iter_slide(c["grids"], 0, n, torch.from_numpy(c["locs"]), z(0, 4), z(n, 0, 4), z(4), z(n, 4),
                                     torch.from_numpy(c["imp"]), c["keep"], PATCH)
    return item, keep_inds.numpy()


def _composed(cases, keeps):
    """candidates -> mask from the DenseGrids lookup of exactly the candidate cells -> admit, all slides in one call each."""
    B = len(cases)
    ldk = max(1, max(len(k) for k in keeps))
    n_cur = max(c["n"] for c in cases)
    keep_idx = np.zeros((B, ldk), np.int32)
    keep_count = np.array([len(k) for k in keeps], np.int32)
    locs = np.zeros((B, n_cur, 2), np.int64)
    for b, (c, k) in enumerate(zip(cases, keeps)):
        keep_idx[b, :len(k)] = k
        locs[b, :c["n"]] = c["locs"]
    nx = np.array([c["grids"].shape(1)[0] for c in cases], np.int32)
    ny = np.array([c["grids"].shape(1)[1] for c in cases], np.int32)
    cc, cells, slot = R.candidate_children(keep_idx, keep_count, locs, PATCH, nx, ny, np.full((B,), -7, np.int32),
                                           np.full((B, 4 * ldk, 2), -7, np.int64), np.full((B, 4 * ldk), -7, np.int32))
    mask = np.zeros((B, 4 * ldk), np.uint8)
    asked = []
    for b, c in enumerate(cases):
        q = torch.from_numpy(cells[b, :cc[b]])
        asked.append(q.numpy())
        assert ((q >= 0).all() and (q[:, 0] < int(nx[b])).all() and (q[:, 1] < int(ny[b])).all()), "only cells inside the grid are asked for"
        assert len(np.unique(q.numpy(), axis=0)) == len(q), "no cell twice"
        if len(q):
            mask[b, :cc[b]] = (c["grids"].rows(1, q[:, 0], q[:, 1]).sum(dim=1) != 0).numpy()
    n_next = 4 * ldk
    out = dict(num_out=np.full((B,), -7, np.int64), locs_out=np.full((B, n_next, 2), -7, np.int64), parent_out=np.full((B, n_next), -7, np.int64),
               src_row=np.full((B, n_next), -7, np.int32), src_cell=np.full((B, n_next), -7, np.int32),
               hp_row=np.full((B, n_next), -7, np.int32), child_pos=np.full((B, 4 * ldk), -7, np.int32))
    status = R.admit_children(cc, cells, slot, mask, keep_idx, keep_count, PATCH, n_next, **out)
    return out, status, (cc, cells, slot, keep_idx, keep_count, ldk)


SHAPES = [((3, 4), (1, 1), 12, 5), ((3, 4), (1, 0), 7, -1), ((5, 2), (0, 1), 10, 64), ((4, 4), (0, 0), 16, 3), ((1, 1), (1, 1), 1, 1),
          ((6, 5), (1, 1), 23, 23)]


@pytest.mark.parametrize("seed", range(6))
def test_composed_contract_equals_the_oracle_step(seed):
    """Odd next grids (2x+1 / 2y+1 out of bounds), keep = -1, a keep larger than the level, and one slide whose candidates are all
    background (count 0, status bit 0): locations, (child -> parent) pairs, order and counts are the oracle's."""
    rng = np.random.default_rng(100 + seed)
    cases = [_case(rng, *shape, odd, n, keep, p_bg=rng.choice([0.1, 0.5])) for shape, odd, n, keep in SHAPES]
    dead = _case(rng, 3, 3, (1, 0), 5, 2, p_bg=2.0)                            # every row of the next grid is background
    cases.insert(seed % len(cases), dead)
    oracle = [_oracle(c) for c in cases]
    out, status, (cc, cells, slot, keep_idx, keep_count, ldk) = _composed(cases, [k for _, k in oracle])
    assert status == 1, "exactly the all-background slide sets bit 0; the capacity 4 ldk is never exceeded"
    for b, (c, (item, keep_inds)) in enumerate(zip(cases, oracle)):
        assert item["fallback"] or c is not dead
        if item["fallback"]:                   # (the dead slide for certain; a tiny random grid may be all background too)
            assert out["num_out"][b] == 0 and cc[b] > 0
            assert (out["src_row"][b] == -1).all() and (out["locs_out"][b] == 0).all()
            continue
        k = int(out["num_out"][b])
        assert k == item["locs"].shape[0] > 0
        np.testing.assert_array_equal(out["locs_out"][b, :k], item["locs"].numpy())
        np.testing.assert_array_equal(out["parent_out"][b, :k], item["parent_inds"].numpy())
        np.testing.assert_array_equal(out["src_row"][b, :k], keep_inds[item["parent_inds"].numpy()])
        np.testing.assert_array_equal(out["hp_row"][b, :k], b * ldk + item["parent_inds"].numpy())
        # the rows the gathers would fetch are the oracle's
        q = torch.from_numpy(cells[b, out["src_cell"][b, :k]])
        assert torch.equal(c["grids"].rows(1, q[:, 0], q[:, 1]), item["fts"])
        # padding, and child_pos as the inverse map of the surviving candidates
        assert (out["locs_out"][b, k:] == 0).all() and (out["parent_out"][b, k:] == 0).all()
        assert (out["src_row"][b, k:] == -1).all() and (out["src_cell"][b, k:] == -1).all() and (out["hp_row"][b, k:] == -1).all()
        count = int(keep_count[b])
        cp = out["child_pos"][b]
        assert (cp[4 * count:] == -7).all() and sorted(cp[:4 * count][cp[:4 * count] >= 0]) == list(range(k))
        for pos in range(k):
            x, y = out["locs_out"][b, pos] // PATCH
            assert cp[((x & 1) * 2 + (y & 1)) * count + out["parent_out"][b, pos]] == pos
        assert (cells[b, cc[b]:] == -1).all() and (slot[b, cc[b]:] == -1).all()
        assert cc[b] <= 4 * count


def test_admit_reports_exceeded_capacity_and_writes_nothing_else():
    rng = np.random.default_rng(3)
    c = _case(rng, 4, 4, (0, 0), 16, -1, p_bg=0.0)
    _, keep = _oracle(c)
    keep_idx, keep_count = keep[None].astype(np.int32), np.array([16], np.int32)
    cc, cells, slot = R.candidate_children(keep_idx, keep_count, c["locs"][None], PATCH, [8], [8], np.zeros(1, np.int32),
                                           np.zeros((1, 64, 2), np.int64), np.zeros((1, 64), np.int32))
    assert cc[0] == 64
    out = dict(num_out=np.full((1,), -7, np.int64), locs_out=np.full((1, 10, 2), -7, np.int64), parent_out=np.full((1, 10), -7, np.int64),
               src_row=np.full((1, 10), -7, np.int32), src_cell=np.full((1, 10), -7, np.int32))
    assert R.admit_children(cc, cells, slot, np.ones((1, 64), np.uint8), keep_idx, keep_count, PATCH, 10, **out) == 2
    assert out["num_out"][0] == 64 and all((v == -7).all() for k, v in out.items() if k != "num_out")
    assert R.check_admit_args(1, 0, PATCH, 16) == -1 and R.check_candidate_args(0, 4, PATCH, 16) == -1
    assert R.check_candidate_args(1, 4, 0, 16) == -1 and R.check_admit_args(1, 4, PATCH, 1 << 29) == -1 and R.check_admit_args(1, 4, PATCH, 16) == 0


# ------------------------------------------------------------------------------------------------
# OnDemandSlide: arguments and bookkeeping (CPU tensors stand in for the device)
# ------------------------------------------------------------------------------------------------
def _grid_encode(grids, log=None):
    def encode(level, cells):
        if log is not None:
            log.append((level, cells.clone()))
        return grids[level][cells[:, 0], cells[:, 1]]
    return encode


def test_on_demand_slide_checks_its_arguments():
    enc = lambda level, cells: torch.zeros(len(cells), 8)
    with pytest.raises(NotImplementedError):
        S.OnDemandSlide([(2, 2)], enc, 8, "cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        S.OnDemandSlide([(2, 2)], enc, 8, "cpu", dtype=torch.float64)
    with pytest.raises(ValueError):
        S.OnDemandSlide([], enc, 8, "cpu")
    with pytest.raises(ValueError):
        S.OnDemandSlide([(2, 0)], enc, 8, "cpu")
    with pytest.raises(ValueError):
        S.OnDemandSlide([(2, 2)], None, 8, "cpu")
    with pytest.raises(ValueError):
        S.OnDemandSlide([(2, 2)], enc, 6, "cpu")
    s = S.OnDemandSlide([(2, 3), (4, 6)], enc, 8, "cpu", slide_id="s0", subtype=1)
    assert s.on_demand and not s.host_resident and s.num_levels == 2 and s.shape(1) == (4, 6) and s.dim == 8
    assert s.dtype == torch.float32 and s.patch_size == 256 and s.requested == [None, None]


def test_encode_results_are_checked():
    cells = torch.tensor([[0, 0], [1, 2]])
    bad = {"shape": lambda l, c: torch.zeros(len(c) + 1, 8), "width": lambda l, c: torch.zeros(len(c), 4),
           "dtype": lambda l, c: torch.zeros(len(c), 8, dtype=torch.float16), "type": lambda l, c: np.zeros((len(c), 8), np.float32)}
    for what, enc in bad.items():
        s = S.OnDemandSlide([(2, 3)], enc, 8, "cpu", slide_id="bad-" + what)
        with pytest.raises(ValueError, match="bad-" + what):
            s.request(0, cells)
    s = S.OnDemandSlide([(2, 3)], lambda l, c: torch.zeros(len(c), 8, device="meta"), 8, "cpu")
    with pytest.raises(ValueError, match="lives on"):
        s.request(0, cells)


def test_requested_bookkeeping_and_once_per_level():
    grids = [torch.arange(2 * 3 * 8, dtype=torch.float32).reshape(2, 3, 8), torch.ones(4, 6, 8)]
    log = []
    s = S.OnDemandSlide([(2, 3), (4, 6)], _grid_encode(grids, log), 8, "cpu")
    c0 = torch.cartesian_prod(torch.arange(2), torch.arange(3))
    rows = s.request(0, c0)
    assert torch.equal(rows, grids[0].reshape(6, 8)) and torch.equal(s.requested[0], c0) and s.requested[1] is None
    with pytest.raises(RuntimeError, match="already requested"):
        s.request(0, c0)
    assert s.request(1, torch.zeros((0, 2), dtype=torch.int64)) is None, "an empty request never reaches the encoder (n >= 1)"
    assert len(log) == 1 and s.requested[1].shape == (0, 2)
    s.begin_pass()
    assert s.requested == [None, None]
    assert torch.equal(s.request(1, torch.tensor([[3, 5]])), torch.ones(1, 8)) and len(log) == 2 and log[1][0] == 1


def test_from_slide_indexes_the_grids():
    grids = [torch.randn(2, 3, 8), torch.randn(4, 6, 8)]
    res = types.SimpleNamespace(host_resident=False, grids=grids, num_levels=2, dim=8, dtype=torch.float32, patch_size=128,
                                slide_id="r", subtype=None, shape=lambda l: tuple(grids[l].shape[:2]))
    s = S.OnDemandSlide.from_slide(res)
    assert s.shapes == [(2, 3), (4, 6)] and s.dim == 8 and s.patch_size == 128 and s.slide_id == "r" and s.device.type == "cpu"
    cells = torch.tensor([[3, 5], [0, 0], [2, 1]])
    assert torch.equal(s.request(1, cells), grids[1][cells[:, 0], cells[:, 1]])


def test_batches_refuse_a_mix_and_a_cpu_device():
    """The kind checks come first: stand-ins are enough, no table is built."""
    od = S.OnDemandSlide([(2, 2)], lambda l, c: torch.zeros(len(c), 8), 8, "cpu")
    res = types.SimpleNamespace(host_resident=False)
    with pytest.raises(ValueError, match="on-demand"):
        S.DeviceSlideBatch([res, od])
    with pytest.raises(ValueError, match="on-demand"):
        S.slide_batch([od, res])
    with pytest.raises(ValueError, match="on-demand"):
        S.OnDemandSlideBatch([od, res])
    from paths_amd._lib import PathsHipError
    with pytest.raises(PathsHipError, match="GPU only"):
        S.slide_batch([od])
    assert S.DeviceSlideBatch.on_demand is False and S.OnDemandSlideBatch.on_demand is True


def test_stored_entry_points_refuse_on_demand_slides_before_the_device():
    from paths_amd import saliency, utils as putils
    od = [S.OnDemandSlide([(2, 2)], lambda l, c: torch.zeros(len(c), 8), 8, "cpu")]
    model = types.SimpleNamespace(use_lstm=True)
    for fn in (lambda: putils.GraphedRecursion(model, od, [2], 2), lambda: putils.recurse_train(model, od, [2], 2),
               lambda: saliency.input_gradients(model, od, [2], 2)):
        with pytest.raises(NotImplementedError, match="on-demand"):
            fn()


@pytest.mark.parametrize("want_hp_row", [True, False])
def test_child_buffers_are_the_six_tables_of_the_expansion(want_hp_row):
    """The resident and the split expansion hand their entry points the same tuple: shapes and dtypes of the C signature."""
    from paths_amd import utils as putils
    B, cap = 3, 5
    bufs = putils._child_buffers(B, cap, want_hp_row, "cpu")
    assert len(bufs) == 6
    i32, i64 = torch.int32, torch.int64
    want = [((B,), i64), ((B, cap, 2), i64), ((B, cap), i64), ((B, cap), i32), ((B, cap), i32), ((B, cap), i32)]
    for t, (shape, dtype) in zip(bufs[:5], want):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    if want_hp_row:
        assert tuple(bufs[5].shape) == want[5][0] and bufs[5].dtype == want[5][1] and bufs[5].is_contiguous()
    else:
        assert bufs[5] is None
