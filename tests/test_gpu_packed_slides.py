"""Packed (tissue-only) slides on the GPU: the pack kernels against their NumPy contract (tests/pack_ref.py), the packed gather and
level-0 entry points against their dense twins, and every way of running the recursion on packed slides against the dense slides of the
same values, bit for bit.  Small grids; D = 256 for the kernels, the model's 1024 for the recursions."""
import gc

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import pack_ref as R
from tests.test_gpu_half_grids import assert_same_recursion
from tests.test_gpu_parity import LOGIT_TOL, build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
NP = {F32: np.float32, F16: np.float16}
PACKED_NAMES = {"paths_gather_rows_packed", "paths_gather_rows_packed_h16", "paths_level0_batch_packed", "paths_level0_batch_packed_h16"}
KEYS = ("logits", "ctx_slide", "importance")


def free_pinned():
    gc.collect()
    torch.cuda.synchronize()
    empty = getattr(torch._C, "_host_emptyCache", None)
    if empty is not None:
        empty()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------
# 1. the pack kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (48, 80)])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_pack_kernels_equal_the_numpy_contract(dev, dtype, shape):
    """A scan block of paths_pack_index is 1024 cells: 48 x 80 = 3,840 cells are three full blocks and a partial one of 768.  The levels
    are the contract's case grids: mixed (with a zero-sum row and a row of -0.0 only), all background, no background, single cells."""
    from paths_amd.data_utils.slide import DeviceSlide
    cases = R.case_grids(NP[dtype], shape, 256, seed=shape[0])
    grids = [torch.from_numpy(g) for g in cases.values()]
    dense = DeviceSlide([g.to(dev) for g in grids])
    packed = dense.pack()
    built = DeviceSlide.from_host([g.float() for g in grids], dev, dtype=dtype, packed=True)
    torch.cuda.synchronize()
    assert packed.packed and not dense.packed and packed.num_levels == len(grids) and packed.dim == 256 and packed.dtype == dtype
    assert dense.rows is None and dense.index is None and packed.grids is None
    for l, (name, g) in enumerate(cases.items()):
        rows, index, n = R.pack(g)
        assert packed.shape(l) == dense.shape(l) == g.shape[:2]
        assert packed.index[l].dtype == torch.int32 and packed.index[l].is_cuda
        np.testing.assert_array_equal(packed.index[l].cpu().numpy(), index, err_msg=name)
        assert tuple(packed.rows[l].shape) == (n, 256), name
        assert same_bits(packed.rows[l].cpu(), torch.from_numpy(rows)), name
        assert torch.equal(packed.masks[l], dense.masks[l]), name
        np.testing.assert_array_equal(packed.masks[l].cpu().numpy(), R.tissue_mask(g), err_msg=name)
        assert torch.equal(built.index[l], packed.index[l]) and same_bits(built.rows[l], packed.rows[l]), name
        assert torch.equal(built.masks[l], packed.masks[l]), name
        assert same_bits(packed.to_dense().grids[l], dense.grids[l]), name
    assert packed.feature_absmax() == dense.feature_absmax() == built.feature_absmax() and dense.feature_absmax() > 0
    if shape != (1, 1):
        m = cases["mixed"]
        kept, mask = R.kept_flags(m).astype(bool), R.tissue_mask(m).reshape(-1).astype(bool)
        assert (kept & ~mask).sum() == 2 and not (mask & ~kept).any(), "the zero-sum row and the -0.0 row are kept behind a 0 mask"
    cells = [g.shape[0] * g.shape[1] for g in grids]
    n_rows = [int(r.shape[0]) for r in packed.rows]
    assert packed.resident_bytes() == sum(n * 256 * packed.rows[0].element_size() + 4 * c + c for n, c in zip(n_rows, cells))


def test_pack_index_is_repeatable_and_checks_its_arguments(dev):
    from paths_amd import _lib
    rng = np.random.default_rng(5)
    cells = 3 * 1024 + 5
    flags = torch.from_numpy((rng.random(cells) < 0.4).astype(np.uint8)).to(dev)
    parts = int(_lib.load().paths_pack_index_partials(cells))
    assert parts == 4
    outs = []
    for _ in range(2):
        index = torch.full((cells + 8,), -7, dtype=torch.int32, device=dev)
        count = torch.full((1,), -7, dtype=torch.int32, device=dev)
        partials = torch.full((parts + 2,), -7, dtype=torch.int32, device=dev)
        _lib.call("paths_pack_index", flags.data_ptr(), cells, index.data_ptr(), count.data_ptr(), partials.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        assert (index[cells:] == -7).all() and (partials[parts:] == -7).all(), "nothing is written past the tables"
        outs.append((index[:cells].cpu(), int(count)))
    f = flags.cpu().numpy().astype(bool)
    want = np.where(f, np.cumsum(f) - f, -1).astype(np.int32)
    np.testing.assert_array_equal(outs[0][0].numpy(), want)
    assert outs[0][1] == outs[1][1] == int(f.sum()) and torch.equal(outs[0][0], outs[1][0])
    st = _lib.stream()
    for args in ((None, cells, index.data_ptr(), count.data_ptr(), partials.data_ptr(), st),
                 (flags.data_ptr(), 0, index.data_ptr(), count.data_ptr(), partials.data_ptr(), st),
                 (flags.data_ptr(), cells, index.data_ptr(), count.data_ptr(), None, st)):
        with pytest.raises(_lib.PathsHipError, match=r"paths_pack_index failed \(-1\)"):
            _lib.call("paths_pack_index", *args)
    g = torch.zeros((4, 6), dtype=torch.float32, device=dev)
    with pytest.raises(_lib.PathsHipError, match="multiple of 4"):
        _lib.call("paths_pack_flags", g.data_ptr(), 4, 6, flags.data_ptr(), st)
    with pytest.raises(_lib.PathsHipError, match=r"failed \(-1\)"):
        _lib.call("paths_pack_rows", g.data_ptr(), 4, 4, index.data_ptr(), 0, g.data_ptr(), st)


def _patch_lists(dev, dtype, seed=3, D=256):
    """Three levels as coords + features: rows in a scrambled order, a level without tissue, a full level."""
    rng = np.random.default_rng(seed)
    shapes = [(3, 5), (6, 10), (2, 2)]
    coords, feats = [], []
    for (X, Y), frac in zip(shapes, (0.6, 0.0, 1.0)):
        cells = rng.permutation(X * Y)[:int(round(frac * X * Y))]
        coords.append(torch.from_numpy(np.stack([cells // Y, cells % Y], axis=1).astype(np.int64)).reshape(-1, 2))
        feats.append(torch.from_numpy(rng.standard_normal((len(cells), D)).astype(np.float32)).to(dtype))
    return coords, feats, shapes


@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_from_patches_equals_the_scattered_dense_slide(dev, dtype, kind):
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    cls = DeviceSlide if kind == "device" else HostSlide
    coords, feats, shapes = _patch_lists(dev, dtype)
    s = cls.from_patches(coords, [f.float() for f in feats], shapes, dev, dtype=dtype, patch_size=128, slide_id="p")
    grids = []
    for c, f, (X, Y) in zip(coords, feats, shapes):
        g = torch.zeros((X, Y, 256), dtype=dtype)
        g[c[:, 0], c[:, 1]] = f
        grids.append(g)
    dense = DeviceSlide([g.to(dev) for g in grids], patch_size=128)
    assert s.packed and s.patch_size == 128 and s.slide_id == "p" and s.dtype == dtype and s.num_levels == 3 and s.dim == 256
    for l in range(3):
        assert s.shape(l) == shapes[l] and s.index[l].is_cuda and s.rows[l].is_cuda == (kind == "device")
        assert same_bits(s.rows[l].cpu(), feats[l]), "rows are kept in the given order"
        c = coords[l]
        assert s.index[l].cpu()[c[:, 0], c[:, 1]].tolist() == list(range(c.shape[0])) and int((s.index[l] >= 0).sum()) == c.shape[0]
        assert torch.equal(s.masks[l], dense.masks[l])
        assert same_bits(s.to_dense().grids[l].cpu(), grids[l])
    assert s.rows[1].shape[0] == 0 and s.feature_absmax() == dense.feature_absmax()
    if kind == "host":
        assert all(r.is_pinned() for r in s.rows if r.numel()) and s.host_bytes() == sum(r.numel() * r.element_size() for r in s.rows)
        assert s.resident_bytes() == sum(5 * X * Y for X, Y in shapes), "device bytes of a packed HostSlide: index + masks"
        t = s.to_device()
        assert t.packed and not t.host_resident and all(same_bits(a.cpu(), b) for a, b in zip(t.rows, s.rows))
        assert t.feature_absmax() == s.feature_absmax()
    del s
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 2. the packed gather / level-0 entry points against their dense twins
# ------------------------------------------------------------------------------------------------
def _packed_tables(dev, dtype, shapes, D, seed):
    """Dense grids with background cells (and one level without any row) + their packed form and the three pointer tables."""
    from paths_amd.data_utils.slide import _pack_device_grid
    rng = np.random.default_rng(seed)
    grids = []
    for k, (X, Y) in enumerate(shapes):
        g = torch.from_numpy(rng.standard_normal((X * Y, D)).astype(np.float32)).to(dtype)
        g[torch.from_numpy(rng.random(X * Y) < (1.0 if k == 1 else 0.4))] = 0         # slide 1: an empty level (n_l = 0)
        grids.append(g.view(X, Y, D).to(dev))
    packed = [_pack_device_grid(g) for g in grids]
    assert packed[1][0].shape[0] == 0 and all(p[0].shape[0] > 0 for k, p in enumerate(packed) if k != 1)
    tab = lambda vals: torch.tensor(vals, dtype=torch.int64, device=dev)
    return grids, packed, tab([g.data_ptr() for g in grids]), tab([r.data_ptr() if r.numel() else 0 for r, _ in packed]), \
        tab([ix.data_ptr() for _, ix in packed])


def _expected_ptrs(packed, cells, valid, D, zero_row):
    """row_ptrs of a packed launch: rows.data_ptr() + index * D * itemsize, zero_row for index < 0 and for padding."""
    want = torch.full(cells.shape, zero_row.data_ptr(), dtype=torch.int64)
    for b, (rows, index) in enumerate(packed):
        r = index.reshape(-1).cpu()[cells[b].long().clamp(min=0)].long()
        ok = valid[b] & (r >= 0)
        want[b, ok] = rows.data_ptr() + r[ok] * D * rows.element_size()
    return want


@pytest.mark.parametrize("dest", ["copy", "ptrs", "both"])
@pytest.mark.parametrize("zero_pad", [0, 1])
@pytest.mark.parametrize("n_next", [10, 7])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_packed_gather_equals_its_dense_twin(dev, dtype, n_next, zero_pad, dest):
    """n_next = 10 and 7 are no multiples of the 4 rows of a workgroup; num_out covers n_next, a middle value and 0; slide 1's level has
    no row at all."""
    from paths_amd import _lib
    D, Dp, n_cur, B = 256, 64, 5, 3
    sfx = "_h16" if dtype == F16 else ""
    shapes = [(3, 4), (2, 5), (4, 4)]
    grids, packed, d_grid, d_rows, d_index = _packed_tables(dev, dtype, shapes, D, n_next)
    rng = np.random.default_rng(n_next)
    src_cell = torch.from_numpy(np.stack([rng.integers(0, X * Y, n_next) for X, Y in shapes]).astype(np.int32))
    src_row = torch.from_numpy(rng.integers(-1, n_cur, (B, n_next)).astype(np.int32)).to(dev)
    num_out = torch.tensor([n_next, n_next // 2, 0], dtype=torch.int64)
    state = torch.from_numpy(rng.standard_normal((B, n_cur, Dp)).astype(np.float32)).to(dev)
    zero_row = torch.zeros((D,), device=dev)
    d_cell, d_num = src_cell.to(dev), num_out.to(dev)

    def run(name, ptrs, extra):
        fts = torch.full((B, n_next, D), float("nan"), device=dev) if dest != "ptrs" else None
        rp = torch.full((B, n_next), -5, dtype=torch.int64, device=dev) if dest != "copy" else None
        so = torch.full((B, n_next, Dp), float("nan"), device=dev)
        p = _lib.ptr
        _lib.call(name, p(ptrs), p(d_cell), D, p(state), n_cur, Dp, p(src_row), Dp, p(d_num), B, n_next, p(fts), p(so), zero_pad, p(rp),
                  p(zero_row) if rp is not None else None, *extra, _lib.stream())
        torch.cuda.synchronize()
        return fts, rp, so

    fa, ra, sa = run("paths_gather_rows_packed" + sfx, d_rows, (d_index.data_ptr(),))
    fb, rb, sb = run("paths_gather_rows" + sfx, d_grid, ())
    assert torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    if fa is not None:
        assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)), "fts_out bit-equal (padding rows included)"
        assert not torch.isnan(fa[0]).any() and float(fa[0].abs().sum()) > 0
    if ra is not None:
        valid = torch.arange(n_next)[None, :] < num_out[:, None]
        assert torch.equal(ra.cpu(), _expected_ptrs(packed, src_cell, valid, D, zero_row))
        assert (ra[1].cpu() == zero_row.data_ptr()).all(), "a level without rows: every entry is the zero row"
        assert int((ra[0].cpu() == zero_row.data_ptr()).sum()) > 0, "some gathered cells are background"


@pytest.mark.parametrize("dest", ["copy", "ptrs", "both"])
@pytest.mark.parametrize("zero_pad", [0, 1])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_packed_level0_equals_its_dense_twin(dev, dtype, zero_pad, dest):
    from paths_amd import _lib
    D, n0 = 256, 18
    sfx = "_h16" if dtype == F16 else ""
    shapes = [(3, 5), (1, 1), (4, 4)]
    grids, packed, d_grid, d_rows, d_index = _packed_tables(dev, dtype, shapes, D, 11)
    B = len(shapes)
    gx = torch.tensor([s[0] for s in shapes], dtype=torch.int32, device=dev)
    gy = torch.tensor([s[1] for s in shapes], dtype=torch.int32, device=dev)
    zero_row = torch.zeros((D,), device=dev)

    def run(name, ptrs, extra):
        fts = torch.full((B, n0, D), float("nan"), device=dev) if dest != "ptrs" else None
        rp = torch.full((B, n0), -5, dtype=torch.int64, device=dev) if dest != "copy" else None
        locs = torch.full((B, n0, 2), -5, dtype=torch.int64, device=dev)
        parent = torch.full((B, n0), -5, dtype=torch.int64, device=dev)
        num = torch.full((B,), -5, dtype=torch.int64, device=dev)
        p = _lib.ptr
        _lib.call(name, p(ptrs), p(gx), p(gy), B, D, 256, n0, p(fts), p(locs), p(parent), p(num), zero_pad, p(rp),
                  p(zero_row) if rp is not None else None, *extra, _lib.stream())
        torch.cuda.synchronize()
        return fts, rp, locs, parent, num

    a = run("paths_level0_batch_packed" + sfx, d_rows, (d_index.data_ptr(),))
    b = run("paths_level0_batch" + sfx, d_grid, ())
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)
    assert a[4].tolist() == [15, 1, 16]
    if a[0] is not None:
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    if a[1] is not None:
        cells = torch.arange(n0, dtype=torch.int32)[None, :].repeat(B, 1)
        valid = cells < torch.tensor([X * Y for X, Y in shapes])[:, None]
        assert torch.equal(a[1].cpu(), _expected_ptrs(packed, cells * valid, valid, D, zero_row))
        assert int((a[1][0, :15].cpu() == zero_row.data_ptr()).sum()) > 0, "level 0 holds background cells"


def test_packed_entry_points_check_their_arguments(dev):
    from paths_amd import _lib
    t = torch.zeros((8,), dtype=torch.int64, device=dev)
    f = torch.zeros((64,), device=dev)
    p, st = t.data_ptr(), _lib.stream()
    with pytest.raises(_lib.PathsHipError, match=r"failed \(-1\).*null"):
        _lib.call("paths_gather_rows_packed", p, p, 8, None, 1, 8, None, 8, p, 1, 2, f.data_ptr(), None, 0, None, None, None, st)
    with pytest.raises(_lib.PathsHipError, match=r"failed \(-1\).*null"):
        _lib.call("paths_level0_batch_packed_h16", p, p, p, 1, 8, 256, 2, f.data_ptr(), p, p, p, 0, None, None, None, st)
    with pytest.raises(_lib.PathsHipError, match=r"failed \(-1\).*zero row"):
        _lib.call("paths_gather_rows_packed_h16", p, p, 8, None, 1, 8, None, 8, p, 1, 2, None, None, 0, p, None, p, st)


# ------------------------------------------------------------------------------------------------
# 3. recursion twins
# ------------------------------------------------------------------------------------------------
def _slides(dev, kind, dtype, seed=99, ids=range(3), base=(9, 11), p_bg=0.6, **kw):
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    cls = DeviceSlide if kind == "device" else HostSlide
    dense = [cls.synthetic(seed, sid, base, p_bg=p_bg, device=dev, dtype=dtype, **kw) for sid in ids]
    return dense, [s.pack() for s in dense]


@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_packed_recursion_is_bitwise_its_dense_twin(dev, dtype, kind):
    from paths_amd.data_utils.slide import DeviceSlideBatch
    cfg, model, _ = build_model(dev, 77, None, top_k_patches=[24] * 4)
    dense, packed = _slides(dev, kind, dtype)
    db = DeviceSlideBatch(dense)
    flat_before = db.flat_tables().clone()
    pb = DeviceSlideBatch(packed)
    assert pb.packed and not db.packed and db.index_ptrs is None and pb.host_resident == (kind == "host")
    assert pb.grid_ptrs[4].cpu().tolist() == [s.rows[4].data_ptr() for s in packed]
    assert pb.index_ptrs[4].cpu().tolist() == [s.index[4].data_ptr() for s in packed]
    # a dense batch's tables are byte for byte what they were: grid pointers, mask pointers, gx, gy per level
    B = len(dense)
    want = torch.cat([t[l].view(torch.uint8) for l in range(5) for t in (db.grid_ptrs, db.mask_ptrs, db.gx, db.gy)])
    assert torch.equal(db.flat_tables(), want) and torch.equal(flat_before, want) and want.numel() == 5 * 24 * B
    assert pb.flat_tables().numel() == 5 * 32 * B and torch.equal(pb.clone_tables().index_ptrs[3], pb.index_ptrs[3])
    with pytest.raises(ValueError, match="packed"):
        DeviceSlideBatch([dense[0], packed[1]])
    sfx = "_h16" if dtype == F16 else ""
    for kw in ({}, dict(attention=True, rollout=True)):
        H.twin_runs(model, cfg.top_k_patches, pb, db, **kw)       # (the first pass also builds the cached weight images)
        ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, pb, db, **kw)
        assert ca.count("paths_level0_batch_packed" + sfx) == 1 and ca.count("paths_gather_rows_packed" + sfx) == 4
        assert not (set(cb) & PACKED_NAMES), "a dense run launches no packed entry point"
        assert cb.count("paths_level0_batch" + sfx) == 1 and cb.count("paths_gather_rows" + sfx) == 4
        assert [c.replace("_packed", "") for c in ca] == cb, "the same launch list but for the two address-forming kernels"
        assert int(oa["status"].item()) == 0
        assert_same_recursion(ta, tb, oa, ob)
        for l, (x, y) in enumerate(zip(ta, tb)):
            for key in ("attention", "attention_self", "rollout", "rollout_self") if kw else ():
                assert torch.equal(x[key], y[key]), f"level {l}: {key}"
    assert int(ta[4]["num_ims"].min()) > 0
    del dense, packed, db, pb
    free_pinned()


@pytest.mark.parametrize("kind", ["device", "host"])
def test_packed_recursion_with_gathered_copies(dev, kind, monkeypatch):
    """utils.ROWS_IN_PLACE off: the gathers write fp32 copies (a dropped row is written as zeros) instead of an address table."""
    from paths_amd import utils as putils
    monkeypatch.setattr(putils, "ROWS_IN_PLACE", False)
    cfg, model, _ = build_model(dev, 77, None, top_k_patches=[24] * 4)
    dense, packed = _slides(dev, kind, F16)
    ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, packed, dense)
    assert "paths_stage_rows" not in ca and ca.count("paths_gather_rows_packed_h16") == 4 and not (set(cb) & PACKED_NAMES)
    assert_same_recursion(ta, tb, oa, ob)
    del dense, packed
    free_pinned()


def test_packed_recursion_vs_oracle(dev):
    """The setting of test_gpu_parity.test_recursion_vs_oracle_random_seeds on packed slides, with its bars."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    cfg, model, params = build_model(dev, 77, None, top_k_patches=[24] * 4)
    ocfg = H.oracle_config(top_k_patches=[24] * 4)
    slides = [DeviceSlide.synthetic(99, sid, (9, 11), p_bg=0.15, device=dev, packed=True) for sid in range(3)]
    assert all(s.packed for s in slides)
    trace, otrace = [], []
    with torch.no_grad():
        out = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=trace)
        hz, _ = orc.inference_end2end(params, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], None, otrace)
    for l in range(5):
        np.testing.assert_array_equal(trace[l]["num_ims"].cpu().numpy(), otrace[l]["num_ims"].numpy())
    np.testing.assert_allclose(torch.sigmoid(out["logits"]).cpu().numpy(), hz.numpy(), atol=LOGIT_TOL, rtol=0)


# ------------------------------------------------------------------------------------------------
# 4. zero-children fallback, masked views, on-demand replay
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["device", "host"])
def test_packed_zero_children_fallback_bitwise(dev, kind):
    from paths_amd import utils as putils
    cfg, model, _ = build_model(dev, 9, None, top_k_patches=[2] * 4)
    dense, packed = _slides(dev, kind, F32, seed=57, ids=range(4), base=(4, 4), p_bg=0.93)
    with torch.no_grad():
        fast = putils._recurse(model, packed, cfg.top_k_patches, 5, None, careful=False)
    assert int(fast["status"].item()) & 1, "test slides should trigger the fallback (pick another seed otherwise)"
    ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, packed, dense)
    assert "paths_fallback_all_cells" in ca and "paths_fallback_all_cells" in cb and not (set(cb) & PACKED_NAMES)
    assert_same_recursion(ta, tb, oa, ob)
    del dense, packed
    free_pinned()


def test_packed_masked_view_bitwise(dev):
    """with_masks on a packed slide: cleared cells at level 0 (read as zero rows) and deeper (dropped by the child filter)."""
    cfg, model, _ = build_model(dev, 77, None, top_k_patches=[24] * 4)
    dense, packed = _slides(dev, "device", F32, p_bg=0.3)
    gen = torch.Generator().manual_seed(8)
    views = [[], []]
    for d, p in zip(dense, packed):
        masks = [(m.cpu() * (torch.rand(m.shape, generator=gen) < 0.8)).to(torch.uint8).to(dev) for m in d.masks]
        assert any(int(m.sum()) < int(o.sum()) for m, o in zip(masks, d.masks)) and int(masks[0].sum()) < masks[0].numel()
        views[0].append(d.with_masks(masks))
        views[1].append(p.with_masks(masks))
    assert all(v.packed and v.masked_view and v.rows is p.rows for v, p in zip(views[1], packed))
    ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, views[1], views[0])
    assert "paths_level0_mask_rows" in ca and "paths_level0_mask_rows" in cb
    assert_same_recursion(ta, tb, oa, ob)
    # the view of the packed slide packs / unpacks to a view
    assert views[0][0].pack().masked_view and torch.equal(views[0][0].pack().masks[2], views[0][0].masks[2])


@pytest.mark.parametrize("kind", ["device", "host"])
def test_on_demand_replay_of_a_packed_slide(dev, kind):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import OnDemandSlide
    cfg, model, _ = build_model(dev, 77, None, top_k_patches=[24] * 4)
    dense, packed = _slides(dev, kind, F32)
    ta, tb = [], []
    with torch.no_grad():
        oa = putils.recurse(model, [OnDemandSlide.from_slide(s) for s in packed], cfg.top_k_patches, 5, trace=ta)
        ob = putils.recurse(model, packed, cfg.top_k_patches, 5, trace=tb)
    torch.cuda.synchronize()
    assert_same_recursion(ta, tb, oa, ob)
    del dense, packed
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 5. tape, pipeline, graph
# ------------------------------------------------------------------------------------------------
def test_packed_tape_rebind_pipeline_and_graph(dev):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch, HostSlide
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[24] * 4)
    keep = cfg.top_k_patches
    mk = lambda seed, packed=True: DeviceSlideBatch([DeviceSlide.synthetic(seed, sid, (9, 11), p_bg=0.6, device=dev, packed=packed)
                                                     for sid in range(3)])
    ba, bb, dense = mk(99), mk(7), mk(99, packed=False)

    def eager(batch):
        with torch.no_grad():
            o = putils.recurse(model, batch, keep, 5)
        return {k: o[k].clone() for k in KEYS}

    ra, rb, rd = eager(ba), eager(bb), eager(dense)
    assert not torch.equal(ra["logits"], rb["logits"]) and all(torch.equal(ra[k], rd[k]) for k in KEYS)
    with torch.no_grad():
        tape = putils.TapedRecursion(model, ba, keep, 5)
        out = tape.replay()
        names = [name for _, _, name in tape.tape]
        assert names.count("paths_level0_batch_packed") == 1 and names.count("paths_gather_rows_packed") == 4
        assert all(torch.equal(out[k], ra[k]) for k in KEYS)
        tape0 = tape.tape
        for batch, ref in ((bb, rb), (ba, ra), (bb, rb)):
            out = tape.rebind(batch).run()
            assert tape.tape is tape0, "bound, not recorded again"
            assert all(torch.equal(out[k], ref[k]) for k in KEYS)
        with pytest.raises(ValueError, match="packed"):
            tape.rebind(dense)
        dt = putils.TapedRecursion(model, dense, keep, 5)
        out = dt.replay()
        assert all(torch.equal(out[k], rd[k]) for k in KEYS) and not ({name for _, _, name in dt.tape} & PACKED_NAMES)
        with pytest.raises(ValueError, match="packed"):
            dt.rebind(ba)
        dt.close()
        tape.close()
        pipe = putils.PipelinedRecursion(model, [ba, bb], keep, 5)
        pipe.submit(0)
        pipe.submit(1)
        o0 = {k: v.clone() for k, v in pipe.result(0).items()}
        o1 = pipe.result(1)
        assert all(torch.equal(o0[k], ra[k]) for k in KEYS) and all(torch.equal(o1[k], rb[k]) for k in KEYS)
        pipe.close()
        graph = putils.GraphedRecursion(model, ba, keep, 5)
        out = graph.run()
        assert all(torch.equal(out[k], ra[k]) for k in KEYS)
        host = DeviceSlideBatch([HostSlide.synthetic(99, 0, (9, 11), p_bg=0.6, device=dev, packed=True)])
        with pytest.raises(NotImplementedError, match="host-resident"):
            putils.GraphedRecursion(model, host, keep, 5)
    torch.cuda.synchronize()
    del graph, host
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 6. training and attribution
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["device", "host"])
def test_packed_training_steps_are_bitwise_the_dense_twin(dev, kind):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlideBatch
    from paths_amd.optim import HipAdamW
    dense, packed = _slides(dev, kind, F32, seed=14, base=(16, 16), p_bg=0.6)
    labels = np.asarray([s.synthetic_spec.label(4) for s in dense], np.int64)

    def run(slides):
        cfg, model, _ = build_model(dev, 3, None, top_k_patches=[64] * 4)
        batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
        model.train()
        opt = HipAdamW(model.parameters(), lr=1e-4)
        losses, grads = [], []
        with H.spy_calls() as calls:
            for _ in range(3):
                losses.append(float(putils.train_step(model, opt, batch, 5, cfg.top_k_patches)))
                grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        return losses, grads, {n: p.detach().clone() for n, p in model.named_parameters()}, calls

    la, ga, pa, ca = run(packed)
    lb, gb, pb, cb = run(dense)
    assert ca.count("paths_level0_batch_packed") == 3 and ca.count("paths_gather_rows_packed") == 12 and not (set(cb) & PACKED_NAMES)
    assert np.isfinite(la).all() and la == lb
    for a, b in zip(ga, gb):
        assert a.keys() == b.keys() and all(torch.equal(a[n], b[n]) for n in a)
    assert all(torch.equal(pa[n], pb[n]) for n in pa)
    del dense, packed
    free_pinned()


def test_packed_input_gradients_and_removal_curves(dev):
    from paths_amd import utils as putils
    from paths_amd.saliency import input_gradients, removal_curves
    from tests.test_gpu_perturbation import _fixed_scores
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[16] * 4)
    dense, packed = _slides(dev, "device", F32, seed=14, base=(6, 7), p_bg=0.4)
    oa, ta = input_gradients(model, packed, cfg.top_k_patches, 5, keep_gradients=True)
    ob, tb = input_gradients(model, dense, cfg.top_k_patches, 5, keep_gradients=True)
    assert torch.equal(oa["logits"], ob["logits"]) and torch.equal(oa["target"], ob["target"])
    assert float(ta[0]["grad_norm"].sum()) > 0
    for l, (a, b) in enumerate(zip(ta, tb)):
        assert a.keys() == b.keys()
        for key in a:
            assert torch.equal(a[key], b[key]), f"level {l}: {key}"
    t = []
    with torch.no_grad():
        putils.recurse(model, dense, cfg.top_k_patches, 5, trace=t)
    scores = _fixed_scores(t, dev, seed=4)
    run = lambda sl: removal_curves(model, sl, cfg.top_k_patches, 5, scores, steps=4)
    got, _ = run(packed)
    ref, _ = run(dense)
    assert float((ref["morf"][:, 0] - ref["morf"][:, -1]).abs().min()) > 0
    for key in ("morf", "lerf", "target", "morf_auc", "lerf_auc"):
        assert torch.equal(got[key], ref[key]), key


# ------------------------------------------------------------------------------------------------
# 7. footprint
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_packed_footprint(dev, dtype):
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    spec = dict(dim=256, num_levels=4, p_bg=0.6, device=dev, dtype=dtype)
    dense = DeviceSlide.synthetic(5, 1, (6, 5), **spec)
    packed = DeviceSlide.synthetic(5, 1, (6, 5), packed=True, **spec)
    twin = dense.pack()
    es = 2 if dtype == F16 else 4
    cells = [30 << (2 * l) for l in range(4)]
    n = [int(r.shape[0]) for r in packed.rows]
    assert n[0] == 30 and all(0 < n[l] < cells[l] for l in range(1, 4)), "level 0 has no background, deeper levels about 60 %"
    assert packed.resident_bytes() == sum(k * 256 * es + 4 * c + c for k, c in zip(n, cells))
    assert dense.resident_bytes() == sum(c * 256 * es + c for c in cells) and packed.resident_bytes() < 0.55 * dense.resident_bytes()
    for l in range(4):
        assert same_bits(packed.rows[l], twin.rows[l]) and torch.equal(packed.index[l], twin.index[l]) and torch.equal(packed.masks[l], twin.masks[l])
        assert n[l] == int(dense.masks[l].sum()), "synthetic tissue rows never cancel: kept rows = tissue cells"
    assert packed.feature_absmax() == dense.feature_absmax() and packed.synthetic_spec == dense.synthetic_spec
    h = HostSlide.synthetic(5, 1, (6, 5), packed=True, bounce_bytes=40_000, **spec)         # (the mask pass runs in many chunks)
    assert h.packed and h.resident_bytes() == sum(5 * c for c in cells) and h.host_bytes() == sum(k * 256 * es for k in n)
    assert all(r.is_pinned() and not r.is_cuda for r in h.rows) and all(ix.is_cuda for ix in h.index)
    hp = HostSlide.synthetic(5, 1, (6, 5), **spec).pack()
    for l in range(4):
        assert same_bits(h.rows[l], packed.rows[l].cpu()) and torch.equal(h.index[l], packed.index[l]) and torch.equal(h.masks[l], dense.masks[l])
        assert same_bits(hp.rows[l], h.rows[l]) and torch.equal(hp.masks[l], h.masks[l])
        assert same_bits(h.to_dense().grids[l], dense.grids[l].cpu())
    assert h.feature_absmax() == hp.feature_absmax() == dense.feature_absmax()
    del h, hp
    free_pinned()
