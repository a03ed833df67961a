"""NumPy statement of the contracts of the selection chain's kernels (paths_amd/csrc/select.hip, include/paths_hip.h): top-K, the
resident 4-child expansion, the all-cells fallback, the row gathers, the level-0 batch, the tissue predicate and the non-LSTM context
update, for the CPU and GPU tests.

Like on_demand_ref the functions WRITE INTO the output arrays they are given: what the contract leaves untouched keeps the caller's
fill, so a test that pre-fills the device buffers with the same sentinel can compare every byte.  Addresses are plain integers."""
import numpy as np

from tests import on_demand_ref as OD

TOPK_MAX = 8192


# ------------------------------------------------------------------------------------------------
# argument checks (the PATHS_REQUIRE conditions of the entry points; null pointers are checked by the tests themselves)
# ------------------------------------------------------------------------------------------------
def check_expand_args(B: int, n_cur: int, n_next: int, patch_size: int, ldk: int) -> int:
    return 0 if (B > 0 and n_cur > 0 and n_next > 0 and patch_size > 0 and 0 < ldk and 4 * ldk <= 1 << 30) else -1


def check_fallback_args(B: int, n_next: int, patch_size: int) -> int:
    return 0 if (B > 0 and n_next > 0 and patch_size > 0) else -1


def check_topk_args(B: int, n_max: int, keep: int, ldk: int) -> int:
    ok = B > 0 and 0 < n_max <= TOPK_MAX and (keep == -1 or keep > 0)
    ok = ok and ldk >= (n_max if keep < 0 else min(keep, n_max)) and ldk <= TOPK_MAX
    return 0 if ok else -1


# ------------------------------------------------------------------------------------------------
# top-K
# ------------------------------------------------------------------------------------------------
def topk_key(scores, idx):
    """csrc/rank_key.h: the float's bits mapped monotonically to uint32 (negative: all bits flipped, otherwise the sign bit set),
    complemented, shifted left 32, OR the index.  Ascending keys = descending bit-pattern order, ties by ascending index."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    neg = (u & np.uint64(0x80000000)) != 0
    u = np.where(neg, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return ((~u & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def topk(scores, ld: int, num_ims, keep: int, keep_idx, keep_count, kept_rows=None, row_base_addr: int = 0, row_ld: int = 0,
         slide_rows: int = 0, zero_row_addr: int = 0):
    """scores: float32, row b = elements [b ld, b ld + num_ims[b]) (nothing else is read); keep_idx [B, ldk] int32; keep_count [B]
    int32.  count = n if keep < 0 else min(n, keep); keep_idx[b, :count] = the indices in ascending key order (keep < 0: original
    order); keep_idx[b, count:] untouched.  kept_rows [B, ldk] int64 (paths_topk_rows): the address of float row
    (b slide_rows + index) of a table with row_ld floats per row, and the zero row's address in [count, ldk).

    The key orders BIT PATTERNS: +0.0 before -0.0, a NaN with a clear sign bit before +inf, a NaN with the sign bit set after -inf.
    torch.topk ranks every NaN first, so a negative NaN is where this contract and the reference differ."""
    flat = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    B, ldk = keep_idx.shape
    for b in range(B):
        n = int(num_ims[b])
        count = n if keep < 0 else min(n, keep)
        keep_count[b] = count
        if keep < 0:
            order = np.arange(n)
        else:
            order = np.argsort(topk_key(flat[b * ld:b * ld + n], np.arange(n)), kind="stable")[:count]
        keep_idx[b, :count] = order
        if kept_rows is not None:
            kept_rows[b, :count] = row_base_addr + ((b * slide_rows + order.astype(np.int64)) * row_ld) * 4
            kept_rows[b, count:] = zero_row_addr
    return keep_idx, keep_count


# ------------------------------------------------------------------------------------------------
# expansion (resident form) and the all-cells fallback
# ------------------------------------------------------------------------------------------------
def expand_children(keep_idx, keep_count, locs, patch_size: int, next_x, next_y, masks, n_next: int, num_out, locs_out, parent_out,
                    src_row, src_cell, hp_row=None, child_pos=None) -> int:
    """paths_expand_children: masks[b] is the uint8 [X, Y] tissue mask of slide b's next grid.  The composition of the split form
    (on_demand_ref.candidate_children -> the candidates' mask bytes -> on_demand_ref.admit_children), so the two expansions share one
    statement; the one difference is src_cell, here the grid cell cx * Y + cy of the child.  Returns the status bits."""
    B, ldk = keep_idx.shape
    cc, cells, slot = OD.candidate_children(keep_idx, keep_count, locs, patch_size, next_x, next_y, np.zeros((B,), np.int32),
                                            np.zeros((B, 4 * ldk, 2), np.int64), np.zeros((B, 4 * ldk), np.int32))
    cand_mask = np.zeros((B, 4 * ldk), np.uint8)
    for b in range(B):
        q = cells[b, :cc[b]]
        cand_mask[b, :cc[b]] = np.asarray(masks[b]).reshape(int(next_x[b]), int(next_y[b]))[q[:, 0], q[:, 1]]
    status = OD.admit_children(cc, cells, slot, cand_mask, keep_idx, keep_count, patch_size, n_next, num_out, locs_out, parent_out,
                               src_row, src_cell, hp_row=hp_row, child_pos=child_pos)
    for b in range(B):
        k = int(num_out[b])
        if k <= n_next:                                  # (a slide over capacity wrote num_out only)
            q = cells[b, src_cell[b, :k]]
            src_cell[b, :k] = q[:, 0] * int(next_y[b]) + q[:, 1]
    return status


def fallback_all_cells(next_x, next_y, masks, patch_size: int, n_next: int, num_out, locs_out, parent_out, src_row, src_cell,
                       hp_row=None) -> int:
    """paths_fallback_all_cells: only slides with num_out[b] == 0 are touched.  They continue with the tissue cells of their next grid
    in row-major order, or with every cell if there is none: locs = cell * patch_size, parent_out = src_cell = cell index,
    src_row = hp_row = -1.  n_out > n_next: num_out only, status bit of value 2.  Rows at and beyond n_out are NOT rewritten."""
    status = 0
    for b in range(len(num_out)):
        if int(num_out[b]) != 0:
            continue
        X, Y = int(next_x[b]), int(next_y[b])
        m = np.asarray(masks[b]).reshape(-1)[:X * Y] != 0
        cell = np.nonzero(m)[0] if m.any() else np.arange(X * Y)
        k = len(cell)
        num_out[b] = k
        if k > n_next:
            status |= 2
            continue
        locs_out[b, :k, 0] = (cell // Y) * patch_size
        locs_out[b, :k, 1] = (cell % Y) * patch_size
        parent_out[b, :k] = cell
        src_row[b, :k] = -1
        src_cell[b, :k] = cell
        if hp_row is not None:
            hp_row[b, :k] = -1
    return status


# ------------------------------------------------------------------------------------------------
# gathers and the level-0 batch
# ------------------------------------------------------------------------------------------------
def gather_rows(grids, grid_addrs, src_cell, src_row, num_out, state_cur=None, n_cur: int = 0, ld_state_cur: int = 0, state_off: int = 0,
                Dp: int = 0, fts_out=None, state_out=None, zero_pad: int = 0, row_ptrs=None, zero_row_addr: int = 0):
    """paths_gather_rows / _h16.  grids[b]: [cells, D] float32 or float16, grid_addrs[b] its address.  Row j < num_out[b]:
    fts_out[b, j] = the fp32 widening of grids[b][src_cell[b, j]]; row_ptrs[b, j] = the grid row's address; state_out[b, j] =
    Dp floats of the flat float32 state_cur from element state_off + (b n_cur + src_row[b, j]) ld_state_cur, or zeros if
    src_row[b, j] < 0.  Padding rows: row_ptrs = the zero row's address; the copies are zeros with zero_pad, untouched without."""
    B, n_next = src_cell.shape
    state = None if state_cur is None else np.ascontiguousarray(state_cur, dtype=np.float32).reshape(-1)
    for b in range(B):
        g = np.asarray(grids[b])
        D, size = g.shape[1], g.dtype.itemsize
        for j in range(n_next):
            if j < int(num_out[b]):
                cell = int(src_cell[b, j])
                if fts_out is not None:
                    fts_out[b, j] = g[cell].astype(np.float32)
                if row_ptrs is not None:
                    row_ptrs[b, j] = int(grid_addrs[b]) + cell * D * size
                if state_out is not None:
                    sr = int(src_row[b, j])
                    if sr >= 0:
                        at = state_off + (b * n_cur + sr) * ld_state_cur
                        state_out[b, j] = state[at:at + Dp]
                    else:
                        state_out[b, j] = 0
            else:
                if row_ptrs is not None:
                    row_ptrs[b, j] = zero_row_addr
                if zero_pad:
                    if fts_out is not None:
                        fts_out[b, j] = 0
                    if state_out is not None:
                        state_out[b, j] = 0


def level0_batch(grids, grid_addrs, gx, gy, patch_size: int, locs, parent, num_ims, fts=None, zero_pad: int = 0, row_ptrs=None,
                 zero_row_addr: int = 0):
    """paths_level0_batch / _h16.  grids[b]: [X Y, D]; num_ims[b] = X Y; row j < X Y: locs = (j // Y, j % Y) * patch_size,
    parent = j, fts = the fp32 widening of grid row j, row_ptrs = its address.  Padding rows: locs 0, parent 0, row_ptrs the zero
    row's address; their copy is zeroed only with zero_pad."""
    B, n0 = parent.shape
    for b in range(B):
        g = np.asarray(grids[b])
        D, size = g.shape[1], g.dtype.itemsize
        X, Y = int(gx[b]), int(gy[b])
        num_ims[b] = X * Y
        for j in range(n0):
            if j < X * Y:
                locs[b, j] = ((j // Y) * patch_size, (j % Y) * patch_size)
                parent[b, j] = j
                if fts is not None:
                    fts[b, j] = g[j].astype(np.float32)
                if row_ptrs is not None:
                    row_ptrs[b, j] = int(grid_addrs[b]) + j * D * size
            else:
                locs[b, j] = 0
                parent[b, j] = 0
                if fts is not None and zero_pad:
                    fts[b, j] = 0
                if row_ptrs is not None:
                    row_ptrs[b, j] = zero_row_addr


# ------------------------------------------------------------------------------------------------
# tissue predicate, range word, context update
# ------------------------------------------------------------------------------------------------
def tissue_mask(grid):
    """[cells, D] (float32, or float16 widened exactly) -> uint8 [cells]: 1 iff the row's float32 sum != 0.  A NaN sum (a NaN in the
    row, or +inf and -inf together) is != 0: tissue.  The order of the sum is the kernel's business; the tests use rows whose verdict
    does not depend on it."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(grid).astype(np.float32).sum(axis=1, dtype=np.float32)
    return (s != 0).astype(np.uint8)


def absmax_bits(grid) -> int:
    """The maximum over the grid of the values' float32 bit patterns with the sign cleared (a NaN's pattern is above +inf's)."""
    bits = np.ascontiguousarray(np.asarray(grid).astype(np.float32)).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return int(bits.max())


def tissue_special_rows(D: int, a: float = 1.5):
    """The rows of the tissue tests and their verdicts (none depends on the order of the sum): all zero; only -0.0; one nonzero element
    in the last column; one fp32 subnormal (2^-149); [a, -a, 0, ...] (the pair inside one 4-vector); [a, 0, ..., 0, -a] (for D >= 8 the
    pair is in different lanes); a NaN; +inf and -inf together."""
    r = np.zeros((8, D), np.float32)
    r[1] = -0.0
    r[2, D - 1] = -0.375
    r[3, D // 2] = np.float32(2.0 ** -149)
    r[4, 0], r[4, 1] = a, -a
    r[5, 0], r[5, D - 1] = a, -a
    r[6, 1] = np.nan
    r[7, 0], r[7, D - 1] = np.inf, -np.inf
    return r, np.array([0, 0, 1, 1, 0, 0, 1, 1], np.uint8)


def scale_add_rows(x, alpha, h, num_ims, rows_per_slide: int, use_alpha: int):
    """paths_scale_add_rows in float64: z[row] = a x[row] (+ h[row] on rows idx < num_ims[b]), a = alpha[row] or 1.  x, h: [M, D]."""
    x64 = np.asarray(x, np.float64)
    M = x64.shape[0]
    a = np.asarray(alpha, np.float64).reshape(M, 1) if use_alpha else np.ones((M, 1))
    z = a * x64
    if h is not None:
        rows = np.arange(M)
        valid = (rows % rows_per_slide) < np.asarray(num_ims)[rows // rows_per_slide]
        z[valid] += np.asarray(h, np.float64)[valid]
    return z
