"""The row cache of on-demand slides without a GPU: the NumPy contracts of paths_cache_probe / paths_cache_fill (tests/cache_ref.py) on
hand-made cases, the header and the binding, what CachedOnDemandSlide and its batch refuse, and the export of a hand-filled cache."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cache_ref as R

FILL = -7
NONE = R.SRC_NONE


def _cells(*xy):
    return np.asarray(xy, np.int64).reshape(-1, 2)


def _probe(cells, index, n_max):
    B = len(cells)
    out = (np.full((B, n_max), FILL, np.int32), np.full((B,), FILL, np.int32), np.full((B, n_max, 2), FILL, np.int64), np.full((B,), FILL, np.int32))
    return R.probe(cells, [len(c) for c in cells], index, *out)


def _index(shape, **rows):
    ix = np.full(shape, -1, np.int32)
    for k, r in rows.items():                      # c12=0: cell (1, 2) holds row 0
        ix[int(k[1]), int(k[2])] = r
    return ix


# ------------------------------------------------------------------------------------------------
# 1. the contracts on hand-made cases
# ------------------------------------------------------------------------------------------------
def test_probe_all_hit_all_miss_and_interleaved():
    ix = _index((2, 3), c00=2, c01=0, c12=1)
    src, mc, cells, st = _probe([_cells((0, 1), (1, 2), (0, 0))], [ix], 4)
    assert src.tolist() == [[0, 1, 2, FILL]] and mc.tolist() == [0] and st.tolist() == [0] and (cells == FILL).all(), "all hit"
    src, mc, cells, st = _probe([_cells((1, 1), (0, 2), (1, 0))], [ix], 3)
    assert src.tolist() == [[-1, -2, -3]] and mc.tolist() == [3] and cells[0].tolist() == [[1, 1], [0, 2], [1, 0]], "all miss, order kept"
    src, mc, cells, st = _probe([_cells((1, 0), (0, 0), (0, 2), (1, 2), (1, 1))], [ix], 6)
    assert src.tolist() == [[-1, 2, -2, 1, -3, FILL]] and mc.tolist() == [3]
    assert cells[0, :3].tolist() == [[1, 0], [0, 2], [1, 1]] and (cells[0, 3:] == FILL).all(), "misses compacted in request order"


def test_probe_a_cell_outside_the_grid_and_an_empty_slide():
    ix = [_index((2, 3), c00=0), _index((1, 1)), _index((2, 2))]
    cells = [_cells((0, 0), (2, 0), (0, 3), (-1, 0), (1, 1)), _cells(), _cells((1, 1))]
    src, mc, mcells, st = _probe(cells, ix, 5)
    assert src[0].tolist() == [0, NONE, NONE, NONE, -1] and mc.tolist() == [1, 0, 1] and st.tolist() == [1, 0, 0], "outside: no miss, status"
    assert (src[1] == FILL).all() and (mcells[1] == FILL).all(), "n = 0: only the count and the status are written"
    assert mcells[0, 0].tolist() == [1, 1] and mcells[2, 0].tolist() == [1, 1]


def _fill_case(capacity, count=1, D=4, dtype=np.float32):
    """One slide, grid (2, 3), the store holds cell (0, 0) as row 0; the request interleaves it with three misses."""
    ix = [_index((2, 3), c00=0)]
    cells = [_cells((1, 0), (0, 0), (0, 2), (1, 1))]
    src, mc, mcells, _ = _probe(cells, ix, 6)
    store = [np.full((max(capacity, 1), D), FILL, dtype)]
    store[0][0] = 10
    enc = [np.arange(3 * D, dtype=dtype).reshape(3, D) + 100]
    out = np.full((1, 6, D), FILL, dtype)
    new = R.fill(cells, [4], src, mc, enc, store, [count], [capacity], ix, out)
    return ix[0], store[0], enc[0], out[0], new


def test_fill_stores_every_miss_when_there_is_room():
    ix, store, enc, out, new = _fill_case(capacity=5)
    assert new == [4] and ix.tolist() == [[0, -1, 2], [1, 3, -1]]
    assert (out[0] == enc[0]).all() and (out[1] == 10).all() and (out[2] == enc[1]).all() and (out[3] == enc[2]).all()
    assert (out[4:] == 0).all(), "rows behind n are zeroed"
    assert (store[1:4] == enc).all() and (store[4] == FILL).all() and (store[0] == 10).all()


def test_fill_capacity_cuts_in_the_middle_and_at_zero():
    ix, store, enc, out, new = _fill_case(capacity=2)
    assert new == [2] and ix.tolist() == [[0, -1, -1], [1, -1, -1]], "the first miss is stored, the others pass through"
    assert (out[0] == enc[0]).all() and (out[2] == enc[1]).all() and (out[3] == enc[2]).all() and (store[1] == enc[0]).all()
    ix, store, enc, out, new = _fill_case(capacity=1)
    assert new == [1] and ix.tolist() == [[0, -1, -1], [-1, -1, -1]] and (out[3] == enc[2]).all() and (out[1] == 10).all()


def test_fill_reads_an_outside_cell_as_zeros_and_skips_an_empty_slide():
    ix = [_index((2, 2), c11=0), _index((1, 1))]
    cells = [_cells((5, 5), (1, 1), (0, 1)), _cells()]
    src, mc, _, st = _probe(cells, ix, 3)
    assert st.tolist() == [1, 0] and mc.tolist() == [1, 0]
    store = [np.full((2, 4), 3, np.float16), np.zeros((0, 4), np.float16)]
    out = np.full((2, 3, 4), FILL, np.float16)
    new = R.fill(cells, [3, 0], src, mc, [np.full((1, 4), 9, np.float16), None], store, [1, 0], [2, 0], ix, out)
    assert new == [2, 0] and (out[0, 0] == 0).all() and (out[0, 1] == 3).all() and (out[0, 2] == 9).all() and (out[1] == 0).all()
    assert ix[0].tolist() == [[-1, 1], [-1, 0]] and (ix[1] == -1).all()


def test_refused_shapes():
    assert R.check_args(1, 1, 4) == 0 and R.check_args(3, 4097, 1024) == 0
    for bad in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (1, 1, 6), (-1, 1, 4), (1, 1, -4)):
        assert R.check_args(*bad) == -1


# ------------------------------------------------------------------------------------------------
# 2. header, binding, build list
# ------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_built():
    import ctypes as C
    import __graft_entry__ as g
    from paths_amd import _lib
    vp, i = C.c_void_p, C.c_int
    assert _lib.DECLARATIONS["paths_cache_probe"] == (i, [vp] * 5 + [i, i, i] + [vp] * 5)
    fill = (i, [vp] * 11 + [i, i, i] + [vp, vp])
    assert _lib.DECLARATIONS["paths_cache_fill"] == fill == _lib.DECLARATIONS["paths_cache_fill_h16"]
    assert "row_cache.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "row_cache.hip"))
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define PATHS_CACHE_PROBE_CHUNK (\d+)", text).group(1)) % 64 == 0
    assert "#define PATHS_CACHE_SRC_NONE (-2147483647 - 1)" in text and R.SRC_NONE == -2147483647 - 1
    assert _lib.ABI_VERSION == 3, "the entries are additive"


# ------------------------------------------------------------------------------------------------
# 3. what the class and the batch refuse
# ------------------------------------------------------------------------------------------------
def _slide(cls=None, **kw):
    from paths_amd.data_utils.slide import CachedOnDemandSlide
    return (cls or CachedOnDemandSlide)([(2, 3), (4, 6)], lambda level, cells: None, 4, "cpu", **kw)


def test_constructor_checks_and_defaults():
    from paths_amd.data_utils.slide import CachedOnDemandSlide, OnDemandSlide
    s = _slide()
    assert isinstance(s, OnDemandSlide) and s.on_demand and s.caching and not OnDemandSlide.caching
    assert s.max_rows == [None, None] and s.count == [0, 0] and s.encoded == [None, None] and s.requested == [None, None]
    assert s.row_limit(0) == 6 and s.row_limit(1) == 24 and s.capacity(1) == 0
    assert _slide(max_rows=5).max_rows == [5, 5] and _slide(max_rows=5).row_limit(1) == 5 and _slide(max_rows=[0, 9]).max_rows == [0, 9]
    assert sorted(s.stats) == ["hits", "misses", "requests", "stored"] and all(v == [0, 0] for v in s.stats.values())
    for bad in (-1, [1], [1, 2, 3], 2.5, [1, "x"], True):
        with pytest.raises(ValueError, match="max_rows"):
            _slide(max_rows=bad)
    with pytest.raises(ValueError, match="multiple of 4"):
        CachedOnDemandSlide([(2, 2)], lambda l, c: None, 6, "cpu")
    with pytest.raises(ValueError, match="callable"):
        CachedOnDemandSlide([(2, 2)], None, 4, "cpu")
    with pytest.raises(NotImplementedError, match="on-demand|OnDemandSlide"):
        s.with_masks([])


def test_a_mixed_batch_is_refused():
    from paths_amd.data_utils.slide import DeviceSlideBatch, OnDemandSlide, OnDemandSlideBatch, any_on_demand, slide_batch, uncached_children
    plain = _slide(OnDemandSlide)
    cached = _slide()
    assert any_on_demand([cached])
    for make in (OnDemandSlideBatch, slide_batch):
        with pytest.raises(ValueError, match="all caching .* or all plain"):
            make([cached, plain])
    with pytest.raises(ValueError, match="on-demand"):
        DeviceSlideBatch([cached])
    with pytest.raises(ValueError, match="CachedOnDemandSlide"):
        uncached_children([plain], [{}], [])


def test_stored_slide_entry_points_refuse_a_caching_slide():
    from paths_amd import utils as putils
    with pytest.raises(NotImplementedError, match="on-demand"):
        putils._stored_batch([_slide()], "input_gradients")


# ------------------------------------------------------------------------------------------------
# 4. export of a hand-filled cache
# ------------------------------------------------------------------------------------------------
def test_export_patches_round_trips_through_check_patches():
    from paths_amd.data_utils.slide import check_patches, stored_cells
    s = _slide()
    # level 0: rows 0..2 are cells (1, 2), (0, 0), (0, 1) in insertion order, in a store with room to spare; level 1: never reached
    s.index[0] = torch.tensor([[1, 2, -1], [-1, -1, 0]], dtype=torch.int32)
    s.store[0] = torch.arange(20, dtype=torch.float32).reshape(5, 4)
    s.store[0][1] = 0                                  # stored background: a row like any other
    s.count[0] = 3
    coords, feats, shapes = s.export_patches()
    assert shapes == [(2, 3), (4, 6)] and coords[0].tolist() == [[1, 2], [0, 0], [0, 1]] and coords[0].dtype == torch.int64
    assert torch.equal(feats[0], s.store[0][:3]) and tuple(coords[1].shape) == (0, 2) and tuple(feats[1].shape) == (0, 4)
    lin = check_patches(coords, feats, shapes, torch.float32)
    assert lin[0].tolist() == [5, 0, 1] and lin[1].numel() == 0
    with pytest.raises(RuntimeError, match="names 3 cells for 2"):
        stored_cells(s.index[0], 2)
    s.clear()
    assert s.count == [0, 0] and s.index == [None, None] and s.store == [None, None]
    assert all(c.shape[0] == 0 for c in s.export_patches()[0])
