"""NumPy statement of the contracts of the two selection kernels behind on-demand slides (include/paths_hip.h:
paths_candidate_children, paths_admit_children), for the CPU and GPU tests.

Both functions WRITE INTO the output arrays they are given, like the kernels: what the contract leaves untouched keeps the caller's
fill, so a test that pre-fills the device buffers with the same sentinel can compare every byte."""
import numpy as np


def check_candidate_args(B: int, n_cur: int, patch_size: int, ldk: int) -> int:
    return 0 if (B > 0 and n_cur > 0 and patch_size > 0 and 0 < ldk and 4 * ldk <= 1 << 30) else -1


def check_admit_args(B: int, n_next: int, patch_size: int, ldk: int) -> int:
    return 0 if (B > 0 and n_next > 0 and patch_size > 0 and 0 < ldk and 4 * ldk <= 1 << 30) else -1


def candidate_children(keep_idx, keep_count, locs, patch_size: int, next_x, next_y, cand_count, cand_cells, cand_slot):
    """keep_idx [B, ldk] int32, keep_count [B], locs [B, n_cur, 2] int64 pixel coordinates, next_x / next_y [B] ->
    cand_count [B] int32, cand_cells [B, 4 ldk, 2] int64, cand_slot [B, 4 ldk] int32.  Children of the kept patches in the block order
    (2x,2y) | (2x,2y+1) | (2x+1,2y) | (2x+1,2y+1), each block in kept order, those inside the next grid, order preserved; the entries
    behind them are -1."""
    B, ldk = keep_idx.shape
    for b in range(B):
        count = max(0, min(int(keep_count[b]), ldk))
        rows = keep_idx[b, :count].astype(np.int64)
        cell = locs[b, rows] // patch_size                                    # [count, 2] (floor division of non-negative pixels)
        base = 2 * cell
        cand = np.concatenate([base + np.array(off, np.int64) for off in ((0, 0), (0, 1), (1, 0), (1, 1))], axis=0)
        slot = np.tile(np.arange(count, dtype=np.int32), 4)
        ok = (cand[:, 0] >= 0) & (cand[:, 1] >= 0) & (cand[:, 0] < int(next_x[b])) & (cand[:, 1] < int(next_y[b]))
        n = int(ok.sum())
        cand_count[b] = n
        cand_cells[b, :n] = cand[ok]
        cand_slot[b, :n] = slot[ok]
        cand_cells[b, n:] = -1
        cand_slot[b, n:] = -1
    return cand_count, cand_cells, cand_slot


def admit_children(cand_count, cand_cells, cand_slot, cand_mask, keep_idx, keep_count, patch_size: int, n_next: int,
                   num_out, locs_out, parent_out, src_row, src_cell, hp_row=None, child_pos=None) -> int:
    """The candidates whose mask byte is set (and whose slot is a kept slot), order preserved, in the format of
    paths_expand_children: num_out [B] int64, locs_out [B, n_next, 2] int64 pixels, parent_out [B, n_next] int64 (kept slot),
    src_row [B, n_next] int32 (= keep_idx[b, slot]), src_cell [B, n_next] int32 (= index in the slide's candidate rows), hp_row
    (= b ldk + slot), child_pos [B, 4 ldk] (indexed block * count + slot; -1 = dropped); padding tail 0 / 0 / -1 / -1 / -1.
    Returns the status bits (1: a slide admitted nothing, 2: n_next exceeded - that slide writes num_out only)."""
    B, ldk = keep_idx.shape
    status = 0
    for b in range(B):
        count = max(0, min(int(keep_count[b]), ldk))
        n = max(0, min(int(cand_count[b]), 4 * ldk))
        slot = cand_slot[b, :n].astype(np.int64)
        adm = np.nonzero((cand_mask[b, :n] != 0) & (slot >= 0) & (slot < count))[0]
        k = len(adm)
        num_out[b] = k
        if k == 0:
            status |= 1
        if k > n_next:
            status |= 2
            continue
        s = slot[adm]
        cells = cand_cells[b, adm]
        locs_out[b, :k] = cells * patch_size
        parent_out[b, :k] = s
        src_row[b, :k] = keep_idx[b, s]
        src_cell[b, :k] = adm
        locs_out[b, k:] = 0
        parent_out[b, k:] = 0
        src_row[b, k:] = -1
        src_cell[b, k:] = -1
        if hp_row is not None:
            hp_row[b, :k] = b * ldk + s
            hp_row[b, k:] = -1
        if child_pos is not None:
            child_pos[b, :4 * count] = -1
            blk = (cells[:, 0] & 1) * 2 + (cells[:, 1] & 1)
            child_pos[b, blk * count + s] = np.arange(k)
    return status

