"""The selection chain's kernels (paths_amd/csrc/select.hip) against their NumPy contract (tests/select_ref.py), one entry point at a
time: every output buffer is pre-filled with a sentinel, one launch, and every buffer is compared bit for bit (float buffers as int32
views), padding and what the kernel must leave alone included.  Inputs stay inside the kernels' documented limits."""
import numpy as np
import pytest
import torch

from tests import select_ref as S
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16 = torch.float16
FILL = -7                     # what the kernels leave untouched keeps this value
NAN_FILL = 0x7FC00007         # ... and this bit pattern (a NaN) in float buffers
TORCH_OF = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}


def _ifill(dev, shape, dtype):
    return torch.full(shape, FILL, dtype=dtype, device=dev)


def _ffill(dev, shape):
    return torch.full(shape, NAN_FILL, dtype=torch.int32, device=dev).view(torch.float32)


def _np_ffill(shape):
    return np.full(shape, NAN_FILL, np.int32).view(np.float32)


def _host(t):
    """A device buffer as the integers the comparison is made on."""
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy()


def _same(got: dict, want: dict):
    assert set(got) == set(want)
    for k, t in got.items():
        w = want[k]
        np.testing.assert_array_equal(_host(t), w.view(np.int32) if w.dtype == np.float32 else w, err_msg=k)


def _like(dev, arrays: dict):
    """Device twins of the replica's (pre-filled) host buffers."""
    return {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.float32 else v).to(dev) for k, v in arrays.items()}


# ------------------------------------------------------------------------------------------------
# paths_topk / paths_topk_rows
# ------------------------------------------------------------------------------------------------
TOPK_N = (1, 9, 65, 200, 2050)                     # 2050: the key count pads to 2056, 33 workgroups per slide
TOPK_KEEP = ("one", "64", "n_max", "n_max+5", "all")


def _topk_scores(rng, ld, num_ims, keep, rot):
    """Slide b holds row kind (b + rot) % 4: standard normal values; a run of (up to) 100 exact ties straddling the count boundary;
    alternating -0.0 / +0.0; +-inf, both NaN signs, subnormals and two values one ulp apart among normal values.  The columns at and
    beyond num_ims[b] hold +NaN and 3e38: a kernel that reads them ranks them first."""
    sc = np.empty((len(num_ims), ld), np.float32)
    for b, n in enumerate(num_ims):
        count = n if keep < 0 else min(n, keep)
        v = rng.standard_normal(ld).astype(np.float32)
        kind = (b + rot) % 4
        if kind == 1 and n > 0:
            m = min(100, n)
            run = rng.permutation(n)[:m]
            others = np.sort(np.delete(v[:n], run))[::-1]
            g = max(0, min(count - m // 2, len(others)))               # values above the run: the boundary falls inside it
            hi = others[g - 1] if g > 0 else (others[0] + 1 if len(others) else 1.0)
            lo = others[g] if g < len(others) else hi - 1
            v[run] = np.float32((float(hi) + float(lo)) / 2)
        elif kind == 2:
            v[0::2], v[1::2] = -0.0, 0.0
        elif kind == 3 and n > 0:
            special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000001, 0x80000001, 0x00000200, 0x3F800000, 0x3F800001],
                               np.uint32)
            at = rng.permutation(n)[:min(n, len(special))]
            v.view(np.uint32)[at] = rng.permutation(special)[:len(at)]
        v[n:] = np.where(np.arange(ld - n) % 2 == 0, np.float32(np.nan), np.float32(3e38))
        sc[b] = v
    return sc


@pytest.mark.parametrize("keep_kind", TOPK_KEEP)
@pytest.mark.parametrize("n_max", TOPK_N)
def test_topk_equals_the_numpy_contract(dev, n_max, keep_kind):
    """B = 5 slides of n_max, n_max - 1, about half, 1 and 0 patches in rows of stride n_max + 3; ldk = max(needed, 70) is longer
    than count (and, for small n_max, than n_max: the launch then covers the row table, not the scores)."""
    from paths_amd import _lib
    keep = {"one": 1, "64": 64, "n_max": n_max, "n_max+5": n_max + 5, "all": -1}[keep_kind]
    rng = np.random.default_rng(1000 * n_max + TOPK_KEEP.index(keep_kind))
    B, ld = 5, n_max + 3
    num_ims = [n_max, n_max - 1, n_max // 2, min(1, n_max), 0]
    ldk = max(n_max if keep < 0 else min(keep, n_max), 70)
    assert S.check_topk_args(B, n_max, keep, ldk) == 0 and max(num_ims) <= n_max
    sc = _topk_scores(rng, ld, num_ims, keep, TOPK_KEEP.index(keep_kind))
    slide_rows, row_ld = n_max + 2, 12
    table = torch.zeros((B, slide_rows, row_ld), device=dev)
    zero_row = torch.zeros((row_ld,), device=dev)
    d_sc, d_num = torch.from_numpy(sc).to(dev), torch.tensor(num_ims, dtype=torch.int64, device=dev)

    want = dict(keep_idx=np.full((B, ldk), FILL, np.int32), keep_count=np.full((B,), FILL, np.int32))
    S.topk(sc, ld, num_ims, keep, **want)
    got = _like(dev, dict(keep_idx=np.full((B, ldk), FILL, np.int32), keep_count=np.full((B,), FILL, np.int32)))
    _lib.call("paths_topk", d_sc.data_ptr(), ld, d_num.data_ptr(), B, n_max, keep, got["keep_idx"].data_ptr(), ldk, got["keep_count"].data_ptr(),
              _lib.stream())
    torch.cuda.synchronize()
    _same(got, want)
    for b, n in enumerate(num_ims):
        c = n if keep < 0 else min(n, keep)
        assert want["keep_count"][b] == c and (want["keep_idx"][b, c:] == FILL).all()

    want = dict(keep_idx=np.full((B, ldk), FILL, np.int32), keep_count=np.full((B,), FILL, np.int32), kept_rows=np.full((B, ldk), FILL, np.int64))
    S.topk(sc, ld, num_ims, keep, want["keep_idx"], want["keep_count"], want["kept_rows"], table.data_ptr(), row_ld, slide_rows, zero_row.data_ptr())
    got = _like(dev, dict(keep_idx=np.full((B, ldk), FILL, np.int32), keep_count=np.full((B,), FILL, np.int32),
                          kept_rows=np.full((B, ldk), FILL, np.int64)))
    _lib.call("paths_topk_rows", d_sc.data_ptr(), ld, d_num.data_ptr(), B, n_max, keep, got["keep_idx"].data_ptr(), ldk,
              got["keep_count"].data_ptr(), table.data_ptr(), row_ld, slide_rows, got["kept_rows"].data_ptr(), zero_row.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    _same(got, want)
    assert (want["kept_rows"][4] == zero_row.data_ptr()).all() and (want["kept_rows"] != FILL).all()


# ------------------------------------------------------------------------------------------------
# paths_expand_children
# ------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 8, 512, 513, 600)     # kept patches per slide: none; one thread's worth; all cached; 512: exactly the four cached candidates
                                      # per thread; 513: five per thread and threads 411 .. 511 start past the end; 600: as the on-demand test
EXP_LDK = max(COUNTS)
EXP_KEEP_COUNT = (EXP_LDK + 5, -3) + COUNTS      # slides 0 and 1: keep_count outside [0, ldk] behaves as ldk and 0 (not last in the batch)
EXP_X, EXP_Y = 5, 7                   # next grid: 2x + 1 = 5 and 2y + 1 = 7 fall outside


def _expand_inputs(patch_size, mask_kind, seed=0):
    rng = np.random.default_rng(seed)
    B, ldk, n_cur = len(EXP_KEEP_COUNT), EXP_LDK, 700
    cells = np.stack([rng.integers(0, 3, (B, n_cur)), rng.integers(0, 4, (B, n_cur))], axis=2).astype(np.int64)     # a 3 x 4 parent level
    locs = cells * patch_size
    keep_idx = rng.integers(0, n_cur, (B, ldk)).astype(np.int32)
    keep_count = np.asarray(EXP_KEEP_COUNT, np.int32)
    nx, ny = np.full((B,), EXP_X, np.int32), np.full((B,), EXP_Y, np.int32)
    x, y = np.meshgrid(np.arange(EXP_X), np.arange(EXP_Y), indexing="ij")
    masks = {"ones": np.ones((B, EXP_X, EXP_Y)), "zeros": np.zeros((B, EXP_X, EXP_Y)), "checker": np.tile((x + y) % 2, (B, 1, 1)),
             "random": rng.random((B, EXP_X, EXP_Y)) < 0.5}[mask_kind].astype(np.uint8)
    return B, ldk, n_cur, locs, keep_idx, keep_count, nx, ny, masks


def _expand_buffers(B, ldk, n_next, tables):
    out = dict(num_out=np.full((B,), FILL, np.int64), locs_out=np.full((B, n_next, 2), FILL, np.int64), parent_out=np.full((B, n_next), FILL, np.int64),
               src_row=np.full((B, n_next), FILL, np.int32), src_cell=np.full((B, n_next), FILL, np.int32))
    if tables:
        out.update(hp_row=np.full((B, n_next), FILL, np.int32), child_pos=np.full((B, 4 * ldk), FILL, np.int32))
    return out


def _expand_device_inputs(dev, locs, keep_idx, keep_count, nx, ny, masks):
    t = lambda a: torch.from_numpy(a).to(dev)
    d = dict(keep_idx=t(keep_idx), keep_count=t(keep_count), locs=t(locs), nx=t(nx), ny=t(ny), masks=t(masks))
    cells = masks.shape[1] * masks.shape[2]
    d["mask_ptrs"] = torch.tensor([d["masks"].data_ptr() + b * cells for b in range(len(nx))], dtype=torch.int64, device=dev)
    return d


def _launch_expand(d, ldk, n_cur, patch_size, B, n_next, got, status):
    from paths_amd import _lib
    p = lambda k: got[k].data_ptr() if k in got else None
    _lib.call("paths_expand_children", d["keep_idx"].data_ptr(), ldk, d["keep_count"].data_ptr(), d["locs"].data_ptr(), n_cur, patch_size,
              d["nx"].data_ptr(), d["ny"].data_ptr(), d["mask_ptrs"].data_ptr(), B, n_next, p("num_out"), p("locs_out"), p("parent_out"),
              p("src_row"), p("src_cell"), status.data_ptr(), p("child_pos"), p("hp_row"), _lib.stream())
    torch.cuda.synchronize()


def _expand_expected(patch_size, mask_kind, n_next_kind, tables):
    """The replica's outputs for one case (from buffers holding the fill), and that the case reaches what it is there for."""
    B, ldk, n_cur, locs, keep_idx, keep_count, nx, ny, masks = _expand_inputs(patch_size, mask_kind)
    if patch_size == 1 << 30:
        assert locs.max() >= 1 << 31
    assert keep_idx.max() < n_cur and keep_count[0] > ldk and keep_count[1] < 0 and S.check_expand_args(B, n_cur, 5, patch_size, ldk) == 0
    full = _expand_buffers(B, ldk, 4 * ldk, tables)
    S.expand_children(keep_idx, keep_count, locs, patch_size, nx, ny, masks, 4 * ldk, **full)
    n_next = {"full": 4 * ldk, "exact": max(1, int(full["num_out"].max())), "five": 5}[n_next_kind]
    want = _expand_buffers(B, ldk, n_next, tables)
    want_status = S.expand_children(keep_idx, keep_count, locs, patch_size, nx, ny, masks, n_next, **want)
    num = want["num_out"]
    np.testing.assert_array_equal(num, full["num_out"])
    clamped = _expand_buffers(B, ldk, n_next, tables)
    S.expand_children(keep_idx, np.clip(keep_count, 0, ldk), locs, patch_size, nx, ny, masks, n_next, **clamped)
    assert all(np.array_equal(want[k], clamped[k]) for k in want), "keep_count = ldk + 5 and -3 behave as ldk and 0"
    assert want_status & 1 and num[1] == num[2] == 0, "the slides without kept patches produce nothing"
    if mask_kind == "zeros":
        assert (num == 0).all() and want_status == 1
        assert (want["locs_out"] == 0).all() and (want["parent_out"] == 0).all() and (want["src_row"] == -1).all() and (want["src_cell"] == -1).all()
        assert not tables or ((want["hp_row"] == -1).all() and (want["child_pos"][0] == -1).all() and (want["child_pos"][2] == FILL).all())
    elif n_next_kind == "five":
        over = num > 5
        assert want_status & 2 and over[[0, 5, 6, 7]].all() and not over[[1, 2, 3]].any()
        assert all((v[over] == FILL).all() for k, v in want.items() if k != "num_out"), "over capacity: num_out only"
        assert (want["src_row"][3, :num[3]] >= 0).all() and (want["src_row"][3, num[3]:] == -1).all(), "a slide that fits is written in full"
    else:
        assert not want_status & 2 and num.max() <= n_next and (n_next_kind != "exact" or num.max() == n_next)
        assert mask_kind != "ones" or 4 * 512 * 0.5 < num[6] < 4 * 513, "some children of the 513 kept patches fall outside the 5 x 7 grid"
    return n_next, want, want_status


@pytest.mark.parametrize("tables", [True, False], ids=["tables", "no_tables"])
@pytest.mark.parametrize("n_next_kind", ["full", "exact", "five"])
@pytest.mark.parametrize("mask_kind", ["ones", "zeros", "checker", "random"])
@pytest.mark.parametrize("patch_size", [256, 1 << 30])
def test_expand_kernel_equals_the_numpy_contract(dev, patch_size, mask_kind, n_next_kind, tables):
    """patch_size 2^30 puts the pixel coordinates of every cell with x = 2 at 2^31: the 64-bit division path.  n_next: 4 ldk; exactly
    the largest num_out of the batch (at least 1, the smallest capacity the entry point accepts); 5, which the slides with 8 and more
    kept patches exceed (they write num_out only)."""
    B, ldk, n_cur, locs, keep_idx, keep_count, nx, ny, masks = _expand_inputs(patch_size, mask_kind)
    n_next, want, want_status = _expand_expected(patch_size, mask_kind, n_next_kind, tables)
    got = _like(dev, _expand_buffers(B, ldk, n_next, tables))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    _launch_expand(_expand_device_inputs(dev, locs, keep_idx, keep_count, nx, ny, masks), ldk, n_cur, patch_size, B, n_next, got, status)
    _same(got, want)
    assert int(status.item()) == want_status


@pytest.mark.parametrize("patch_size", [256, 1 << 30])
def test_expand_kernel_equals_its_split_form(dev, patch_size):
    """paths_candidate_children -> the candidates' mask bytes (looked up on the device) -> paths_admit_children on the same inputs:
    every output but src_cell is the resident kernel's; src_cell names the same cell in either form."""
    from paths_amd import _lib
    B, ldk, n_cur, locs, keep_idx, keep_count, nx, ny, masks = _expand_inputs(patch_size, "random")
    d = _expand_device_inputs(dev, locs, keep_idx, keep_count, nx, ny, masks)
    n_next = 4 * ldk
    res = _like(dev, _expand_buffers(B, ldk, n_next, True))
    st_res = torch.zeros((1,), dtype=torch.int32, device=dev)
    _launch_expand(d, ldk, n_cur, patch_size, B, n_next, res, st_res)
    cc = _ifill(dev, (B,), torch.int32)
    cells = _ifill(dev, (B, 4 * ldk, 2), torch.int64)
    slot = _ifill(dev, (B, 4 * ldk), torch.int32)
    _lib.call("paths_candidate_children", d["keep_idx"].data_ptr(), ldk, d["keep_count"].data_ptr(), d["locs"].data_ptr(), n_cur, patch_size,
              d["nx"].data_ptr(), d["ny"].data_ptr(), B, cc.data_ptr(), cells.data_ptr(), slot.data_ptr(), _lib.stream())
    valid = (cells[:, :, 0] >= 0)
    bidx = torch.arange(B, device=dev)[:, None].expand(B, 4 * ldk)
    cmask = (d["masks"][bidx, cells[:, :, 0].clamp(min=0), cells[:, :, 1].clamp(min=0)] * valid).to(torch.uint8).contiguous()
    spl = _like(dev, _expand_buffers(B, ldk, n_next, True))
    st_spl = torch.zeros((1,), dtype=torch.int32, device=dev)
    p = lambda k: spl[k].data_ptr()
    _lib.call("paths_admit_children", cc.data_ptr(), cells.data_ptr(), slot.data_ptr(), cmask.data_ptr(), d["keep_idx"].data_ptr(), ldk,
              d["keep_count"].data_ptr(), patch_size, B, n_next, p("num_out"), p("locs_out"), p("parent_out"), p("src_row"), p("src_cell"),
              st_spl.data_ptr(), p("child_pos"), p("hp_row"), _lib.stream())
    torch.cuda.synchronize()
    assert int(st_res.item()) == int(st_spl.item()) == 1
    for k in res:
        if k != "src_cell":
            np.testing.assert_array_equal(_host(res[k]), _host(spl[k]), err_msg=k)
    num, h_cells = _host(res["num_out"]), _host(cells)
    a, s = _host(res["src_cell"]), _host(spl["src_cell"])
    assert num.max() > 600
    for b in range(B):
        k = int(num[b])
        np.testing.assert_array_equal(h_cells[b, s[b, :k]], np.stack([a[b, :k] // EXP_Y, a[b, :k] % EXP_Y], axis=1))
        assert (a[b, k:] == -1).all() and (s[b, k:] == -1).all()


# ------------------------------------------------------------------------------------------------
# paths_fallback_all_cells
# ------------------------------------------------------------------------------------------------
FB_SHAPES = ((37, 29), (5, 7), (4, 4), (33, 32), (1, 1))      # 1073 cells: two per thread, ragged end; fewer cells than threads; the slide
FB_NUM_OUT = (0, 0, 3, 0, 0)                                  # that is not touched; 1056 cells without tissue: every cell; one cell


@pytest.mark.parametrize("variant", ["fits", "one_short", "no_hp_row"])
def test_fallback_kernel_equals_the_numpy_contract(dev, variant):
    from paths_amd import _lib
    rng = np.random.default_rng(17)
    masks = [(rng.random(s) < p).astype(np.uint8) for s, p in zip(FB_SHAPES, (0.3, 0.5, 2.0, -1.0, 2.0))]
    assert masks[0].sum() < 1056 and 0 < masks[1].sum() < 35 and masks[3].sum() == 0 and masks[4].sum() == 1
    B = len(FB_SHAPES)
    n_next = 1055 if variant == "one_short" else 1056
    nx, ny = np.array([s[0] for s in FB_SHAPES], np.int32), np.array([s[1] for s in FB_SHAPES], np.int32)
    assert S.check_fallback_args(B, n_next, 256) == 0

    def buffers():
        out = _expand_buffers(B, 1, n_next, variant != "no_hp_row")
        out.pop("child_pos", None)
        out["num_out"][:] = FB_NUM_OUT
        return out

    want = buffers()
    want_status = S.fallback_all_cells(nx, ny, masks, 256, n_next, **want)
    got = _like(dev, buffers())
    d_masks = [torch.from_numpy(m).to(dev) for m in masks]
    ptrs = torch.tensor([m.data_ptr() for m in d_masks], dtype=torch.int64, device=dev)
    d_nx, d_ny = torch.from_numpy(nx).to(dev), torch.from_numpy(ny).to(dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    p = lambda k: got[k].data_ptr() if k in got else None
    _lib.call("paths_fallback_all_cells", d_nx.data_ptr(), d_ny.data_ptr(), ptrs.data_ptr(), 256, B, n_next, p("num_out"), p("locs_out"),
              p("parent_out"), p("src_row"), p("src_cell"), status.data_ptr(), p("hp_row"), _lib.stream())
    torch.cuda.synchronize()
    _same(got, want)
    assert int(status.item()) == want_status == (2 if variant == "one_short" else 0)
    assert want["num_out"].tolist() == [int(masks[0].sum()), int(masks[1].sum()), 3, 1056, 1]
    assert all((v[2] == FILL).all() for k, v in want.items() if k != "num_out"), "a slide with children is not touched"
    k0 = int(want["num_out"][0])
    assert (want["src_cell"][0, :k0] == np.nonzero(masks[0].reshape(-1))[0]).all() and (want["src_cell"][0, k0:] == FILL).all()
    if variant == "one_short":
        assert all((v[3] == FILL).all() for k, v in want.items() if k != "num_out"), "over capacity: num_out only"
    else:
        assert (want["parent_out"][3] == np.arange(1056)).all() and (want["src_row"][3] == -1).all()


# ------------------------------------------------------------------------------------------------
# paths_gather_rows / paths_gather_rows_h16
# ------------------------------------------------------------------------------------------------
def _grid_values(rng, cells, D, dtype):
    """Normal values with -0.0, +-inf, subnormals of the grid's type and (fp16) its largest finite value."""
    g = torch.from_numpy(rng.standard_normal((cells, D)).astype(np.float32))
    sub = 2.0 ** -24 if dtype == F16 else 2.0 ** -149
    flat = g.view(-1)
    for at, v in zip(rng.permutation(cells * D)[:6], (-0.0, float("inf"), float("-inf"), sub, -3 * sub, 65504.0)):
        flat[at] = v
    return g.to(dtype)


@pytest.mark.parametrize("dest", ["copy", "ptrs", "both"])
@pytest.mark.parametrize("zero_pad", [0, 1])
@pytest.mark.parametrize("dims", [(8, 8, 8, 0), (1024, 1280, 1280, 0), (1024, 256, 1280, 1024), (8, 0, 0, 0)],
                         ids=["D8", "D1024_state1280", "D1024_window256", "D8_no_state"])
@pytest.mark.parametrize("n_next", [10, 7, 1])
@pytest.mark.parametrize("dtype", [torch.float32, F16], ids=["f32", "f16"])
def test_gather_kernel_equals_the_numpy_contract(dev, dtype, n_next, dims, zero_pad, dest):
    """dims = (D, Dp, row stride of the state, first state column): the third case is the column window of the default path (the
    memory-cell quarter of an h | c state).  num_out covers 0, a middle value and n_next; some valid rows have src_row = -1."""
    from paths_amd import _lib
    D, Dp, ld, off = dims
    rng = np.random.default_rng(n_next * 100 + D + Dp)
    B, n_cur, cells = 3, 5, (6, 11, 4)
    num_out = np.array([0, n_next // 2, n_next], np.int64)
    grids = [_grid_values(rng, c, D, dtype).to(dev) for c in cells]
    src_cell = np.stack([rng.integers(0, c, n_next) for c in cells]).astype(np.int32)
    src_row = rng.integers(-1, n_cur, (B, n_next)).astype(np.int32)
    src_row[2, 0] = -1
    state = rng.standard_normal((B, n_cur, ld)).astype(np.float32) if Dp else None
    zero_row = torch.zeros((D,), device=dev)
    want = {}
    if dest != "ptrs":
        want["fts_out"] = _np_ffill((B, n_next, D))
    if dest != "copy":
        want["row_ptrs"] = np.full((B, n_next), FILL, np.int64)
    if Dp:
        want["state_out"] = _np_ffill((B, n_next, Dp))
    got = _like(dev, want)
    S.gather_rows([g.cpu().numpy() for g in grids], [g.data_ptr() for g in grids], src_cell, src_row, num_out, state_cur=state, n_cur=n_cur,
                  ld_state_cur=ld, state_off=off, Dp=Dp, zero_pad=zero_pad, zero_row_addr=zero_row.data_ptr(), **want)
    d_state = torch.from_numpy(state).to(dev) if Dp else None
    d_ptrs = torch.tensor([g.data_ptr() for g in grids], dtype=torch.int64, device=dev)
    d_cell, d_row, d_num = torch.from_numpy(src_cell).to(dev), torch.from_numpy(src_row).to(dev), torch.from_numpy(num_out).to(dev)
    p = lambda k: got[k].data_ptr() if k in got else None
    _lib.call("paths_gather_rows" + ("_h16" if dtype == F16 else ""), d_ptrs.data_ptr(), d_cell.data_ptr(), D,
              d_state.data_ptr() + 4 * off if Dp else None, n_cur, ld, d_row.data_ptr(), Dp, d_num.data_ptr(), B, n_next, p("fts_out"),
              p("state_out"), zero_pad, p("row_ptrs"), zero_row.data_ptr() if dest != "copy" else None, _lib.stream())
    torch.cuda.synchronize()
    _same(got, want)
    if "fts_out" in got:                            # the copies are the grid's values widened exactly
        for b in range(B):
            k = int(num_out[b])
            assert torch.equal(got["fts_out"][b, :k].view(torch.int32), grids[b].float()[d_cell[b, :k].long()].view(torch.int32))
            pad = _host(got["fts_out"][b, k:])
            assert (pad == (0 if zero_pad else NAN_FILL)).all()
    if Dp:
        assert (_host(got["state_out"][2, 0]) == 0).all(), "src_row = -1: a fresh zero context"


# ------------------------------------------------------------------------------------------------
# paths_level0_batch / paths_level0_batch_h16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dest", ["copy", "ptrs", "both"])
@pytest.mark.parametrize("zero_pad", [0, 1])
@pytest.mark.parametrize("D", [8, 1024])
@pytest.mark.parametrize("n0", [16, 20])
@pytest.mark.parametrize("dtype", [torch.float32, F16], ids=["f32", "f16"])
def test_level0_kernel_equals_the_numpy_contract(dev, dtype, n0, D, zero_pad, dest):
    from paths_amd import _lib
    rng = np.random.default_rng(n0 + D)
    shapes = ((3, 5), (1, 1), (4, 4))
    B = len(shapes)
    grids = [_grid_values(rng, X * Y, D, dtype).to(dev) for X, Y in shapes]
    gx, gy = np.array([s[0] for s in shapes], np.int32), np.array([s[1] for s in shapes], np.int32)
    zero_row = torch.zeros((D,), device=dev)
    want = dict(locs=np.full((B, n0, 2), FILL, np.int64), parent=np.full((B, n0), FILL, np.int64), num_ims=np.full((B,), FILL, np.int64))
    if dest != "ptrs":
        want["fts"] = _np_ffill((B, n0, D))
    if dest != "copy":
        want["row_ptrs"] = np.full((B, n0), FILL, np.int64)
    got = _like(dev, want)
    S.level0_batch([g.cpu().numpy() for g in grids], [g.data_ptr() for g in grids], gx, gy, 256, zero_pad=zero_pad,
                   zero_row_addr=zero_row.data_ptr(), **want)
    d_ptrs = torch.tensor([g.data_ptr() for g in grids], dtype=torch.int64, device=dev)
    d_gx, d_gy = torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev)
    p = lambda k: got[k].data_ptr() if k in got else None
    _lib.call("paths_level0_batch" + ("_h16" if dtype == F16 else ""), d_ptrs.data_ptr(), d_gx.data_ptr(), d_gy.data_ptr(), B, D, 256, n0,
              p("fts"), p("locs"), p("parent"), p("num_ims"), zero_pad, p("row_ptrs"), zero_row.data_ptr() if dest != "copy" else None,
              _lib.stream())
    torch.cuda.synchronize()
    _same(got, want)
    assert want["num_ims"].tolist() == [15, 1, 16]
    if "fts" in got:
        for b, (X, Y) in enumerate(shapes):
            assert torch.equal(got["fts"][b, :X * Y].view(torch.int32), grids[b].float().view(torch.int32))
            assert (_host(got["fts"][b, X * Y:]) == (0 if zero_pad else NAN_FILL)).all()


# ------------------------------------------------------------------------------------------------
# paths_tissue_mask, paths_tissue_mask_absmax, paths_tissue_mask_absmax_h16
# ------------------------------------------------------------------------------------------------
MASK_FILL = 0xF9


@pytest.mark.parametrize("D", [4, 8, 64, 1024])
def test_tissue_kernels_on_the_special_rows(dev, D):
    """7 cells per launch (not a multiple of the 4 cells of a workgroup; byte 7 of the mask keeps its fill), two windows over the
    eight special rows so that each is judged.  The three entry points agree; the fp16 grid gives what its fp32 twin gives."""
    from paths_amd import _lib
    rows, verdict = S.tissue_special_rows(D)
    assert S.tissue_mask(rows).tolist() == verdict.tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    g32 = torch.from_numpy(rows).to(dev)
    g16 = g32.to(F16)
    twin = g16.float().cpu().numpy()
    same = ((twin == rows) | (np.isnan(twin) & np.isnan(rows))).all(axis=1)
    assert same.tolist() == [True, True, True, False, True, True, True, True]
    st = _lib.stream()

    def run(name, grid, start, cells, with_mask=True):
        mask = torch.full((8,), MASK_FILL, dtype=torch.uint8, device=dev)
        bits = torch.zeros((1,), dtype=torch.int32, device=dev)
        at = grid.data_ptr() + start * D * grid.element_size()
        if name == "paths_tissue_mask":
            _lib.call(name, at, cells, D, mask.data_ptr(), st)
        else:
            _lib.call(name, at, cells, D, mask.data_ptr() if with_mask else None, bits.data_ptr(), st)
        torch.cuda.synchronize()
        return mask.cpu().numpy(), int(bits.item()) & 0xFFFFFFFF

    for start in (0, 1):
        win = slice(start, start + 7)
        want = np.append(verdict[win], MASK_FILL).astype(np.uint8)
        m, _ = run("paths_tissue_mask", g32, start, 7)
        np.testing.assert_array_equal(m, want)
        m, bits = run("paths_tissue_mask_absmax", g32, start, 7)
        np.testing.assert_array_equal(m, want)
        assert bits == S.absmax_bits(rows[win]) and not np.isfinite(_lib.float_from_bits(bits)), "a NaN in the grid: not finite"
        m, bits2 = run("paths_tissue_mask_absmax", g32, start, 7, with_mask=False)
        assert (m == MASK_FILL).all() and bits2 == bits
        m, bits = run("paths_tissue_mask_absmax_h16", g16, start, 7)
        np.testing.assert_array_equal(m, np.append(S.tissue_mask(twin[win]), MASK_FILL).astype(np.uint8))
        np.testing.assert_array_equal(m[:7][same[win]], want[:7][same[win]])
        assert bits == S.absmax_bits(twin[win])
        m, bits2 = run("paths_tissue_mask_absmax_h16", g16, start, 7, with_mask=False)
        assert (m == MASK_FILL).all() and bits2 == bits
    for name, grid in (("paths_tissue_mask_absmax", g32), ("paths_tissue_mask_absmax_h16", g16)):
        m, bits = run(name, grid, 0, 6)
        assert bits == S.absmax_bits(rows[:6]) and _lib.float_from_bits(bits) == 1.5 and (m[6:] == MASK_FILL).all()


# ------------------------------------------------------------------------------------------------
# paths_scale_add_rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_h", [True, False], ids=["h", "no_h"])
@pytest.mark.parametrize("use_alpha", [0, 1])
@pytest.mark.parametrize("D", [4, 1024])
def test_scale_add_rows_vs_fp64(dev, D, use_alpha, with_h):
    """z = a x + h in fp32 is two roundings (a x, then the sum) or one if the compiler contracts them to an FMA: per element
    |z - exact| <= 2^-24 (|a x| + |a x + h|) (1 + slack).  Rows without h (padding, or h null) are ONE rounding: NumPy's float32 product."""
    from paths_amd import _lib
    rng = np.random.default_rng(D + use_alpha)
    rows, num_ims = 5, np.array([5, 2, 0], np.int64)
    M = rows * len(num_ims)
    x, h = rng.standard_normal((M, D)).astype(np.float32), rng.standard_normal((M, D)).astype(np.float32)
    alpha = rng.standard_normal((M,)).astype(np.float32)
    d_x, d_h, d_a, d_num = (torch.from_numpy(a).to(dev) for a in (x, h, alpha, num_ims))
    z = _ffill(dev, (M, D))
    _lib.call("paths_scale_add_rows", d_x.data_ptr(), d_a.data_ptr() if use_alpha else None, d_h.data_ptr() if with_h else None, d_num.data_ptr(),
              rows, D, M, use_alpha, z.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    got = z.cpu().numpy()
    ref = S.scale_add_rows(x, alpha, h if with_h else None, num_ims, rows, use_alpha)
    ax = (alpha.astype(np.float64)[:, None] if use_alpha else 1.0) * x.astype(np.float64)
    bound = 2.0 ** -24 * (np.abs(ax) + np.abs(ref)) * 1.01
    err = np.abs(got.astype(np.float64) - ref)
    print(f"scale_add_rows D={D} use_alpha={use_alpha} h={with_h}: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    valid = (np.arange(M) % rows) < num_ims[np.arange(M) // rows]
    exact = ~valid if with_h else np.ones(M, bool)
    prod = (alpha[:, None] * x) if use_alpha else x
    np.testing.assert_array_equal(got[exact].view(np.int32), prod[exact].astype(np.float32).view(np.int32))
    assert valid.sum() == 7


# ------------------------------------------------------------------------------------------------
# argument rejection: -1 without a launch
# ------------------------------------------------------------------------------------------------
def test_selection_entry_points_reject_bad_arguments(dev):
    from paths_amd import _lib
    z = torch.zeros((64,), dtype=torch.int64, device=dev)
    a, st = z.data_ptr(), _lib.stream()

    def refused(name, args):
        with pytest.raises(_lib.PathsHipError, match=name + r" failed \(-1\)"):
            _lib.call(name, *args)

    # paths_expand_children(keep_idx, ldk, keep_count, locs, n_cur, patch, next_x, next_y, mask_ptrs, B, n_next, num_out, locs_out,
    #                       parent_out, src_row, src_cell, status, child_pos, hp_row, stream)
    exp = [a, 2, a, a, 4, 256, a, a, a, 1, 8, a, a, a, a, a, a, None, None, st]
    for at, v in ((9, 0), (5, 0), (10, 0), (4, 0), (1, 0), (1, 1 << 29)):
        bad = list(exp)
        bad[at] = v
        assert S.check_expand_args(bad[9], bad[4], bad[10], bad[5], bad[1]) == -1
        refused("paths_expand_children", bad)
    assert S.check_expand_args(exp[9], exp[4], exp[10], exp[5], exp[1]) == 0
    for at in (0, 2, 3, 6, 7, 8, 11, 12, 13, 14, 15, 16):
        refused("paths_expand_children", exp[:at] + [None] + exp[at + 1:])
    # paths_fallback_all_cells(next_x, next_y, mask_ptrs, patch, B, n_next, num_out, locs_out, parent_out, src_row, src_cell, status, hp_row, stream)
    fb = [a, a, a, 256, 1, 8, a, a, a, a, a, a, None, st]
    for at in (4, 3, 5):
        bad = list(fb)
        bad[at] = 0
        assert S.check_fallback_args(bad[4], bad[5], bad[3]) == -1
        refused("paths_fallback_all_cells", bad)
    for at in (0, 1, 2, 6, 7, 8, 9, 10, 11):
        refused("paths_fallback_all_cells", fb[:at] + [None] + fb[at + 1:])
    # paths_gather_rows*(grid_ptrs, src_cell, D, state_cur, n_cur, ld_state_cur, src_row, Dp, num_out, B, n_next, fts_out, state_out, zero_pad,
    #                    row_ptrs, zero_row, stream)
    for name in ("paths_gather_rows", "paths_gather_rows_h16"):
        ok = [a, a, 8, a, 4, 8, a, 8, a, 1, 4, a, a, 1, a, a, st]
        for change in ({2: 6}, {7: 6}, {5: 6}, {9: 0}, {10: 0}, {11: None, 14: None}, {15: None}, {3: None}, {12: None}):
            refused(name, [change.get(i, v) for i, v in enumerate(ok)])
    # paths_level0_batch*(grid_ptrs, gx, gy, B, D, patch, n0, fts, locs, parent, num_ims, zero_pad, row_ptrs, zero_row, stream)
    for name in ("paths_level0_batch", "paths_level0_batch_h16"):
        ok = [a, a, a, 1, 8, 256, 4, a, a, a, a, 1, a, a, st]
        for change in ({4: 6}, {3: 0}, {6: 0}, {7: None, 12: None}, {13: None}):
            refused(name, [change.get(i, v) for i, v in enumerate(ok)])
    # paths_topk(scores, ld, num_ims, B, n_max, keep, keep_idx, ldk, keep_count, stream) / paths_topk_rows(..., row_base, row_ld, slide_rows,
    #            kept_rows, zero_row, stream)
    for name, tail in (("paths_topk", [st]), ("paths_topk_rows", [a, 12, 8192, a, a, st])):
        for n_max, keep, ldk in ((8193, 512, 512), (100, 0, 100), (100, 50, 49), (100, -1, 99), (100, 50, 8193), (0, 1, 1)):
            assert S.check_topk_args(1, n_max, keep, ldk) == -1
            refused(name, [a, n_max, a, 1, n_max, keep, a, ldk, a] + tail)
    for change in ({9: None}, {12: None}, {13: None}, {10: 0}, {11: 50}):      # the row table: pointers, row_ld > 0, slide_rows >= n_max
        ok = [a, 100, a, 1, 100, 50, a, 50, a, a, 12, 100, a, a, st]
        refused("paths_topk_rows", [change.get(i, v) for i, v in enumerate(ok)])
    torch.cuda.synchronize()
