"""numpy restatement of the two kernels of the removal curves on the free path (include/paths_hip.h: paths_removal_masks /
paths_visited_overlap) and of the count formula of paths_amd.saliency.removal_curves: the reference of the CPU and GPU tests."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np


def counts(n, steps: int, max_fraction: float) -> np.ndarray:
    """[steps + 1, B]: (2 s m_b + steps) // (2 steps) with m_b = floor(max_fraction n_b), python integers."""
    m = [int(math.floor(max_fraction * int(nb))) for nb in n]
    return np.array([[(2 * s * mb + steps) // (2 * steps) for mb in m] for s in range(steps + 1)], dtype=np.int64).reshape(steps + 1, len(n))


def chosen(num_ims, rank, thr) -> np.ndarray:
    """[C, B, N] bool: the rows a member turns to background - valid, with 0 <= rank < thr.  rank [B, N]; thr [C, B]."""
    num_ims, rank, thr = np.asarray(num_ims), np.asarray(rank), np.asarray(thr)
    valid = np.arange(rank.shape[1])[None, :] < num_ims[:, None]
    return valid[None] & (rank[None] >= 0) & (rank[None] < thr[:, :, None])


def all_valid(num_ims, N: int) -> np.ndarray:
    """[1, B, N] bool: every valid row (the members' `chosen` of the recorded-cells bitmap)."""
    return (np.arange(N)[None, :] < np.asarray(num_ims)[:, None])[None]


def removal_masks(src: Sequence[Optional[np.ndarray]], locs, patch_size: int, pick: np.ndarray, set_cells: bool = False):
    """(masks: list over members of a list over slides of uint8 [X_b, Y_b], left [C, B] int32).  src[b]: the source mask uint8
    [X_b, Y_b]; locs [B, N, 2] in pixels (only the picked rows' are looked at); pick [C, B, N] bool (:func:`chosen` /
    :func:`all_valid`).  Member (c, b) is src[b] with cell locs // patch_size of every picked row set to 0 (``set_cells``: to 1);
    left counts its non-zero bytes."""
    locs = np.asarray(locs)
    C, B, _ = pick.shape
    masks: List[List[np.ndarray]] = []
    left = np.zeros((C, B), np.int32)
    for c in range(C):
        row = []
        for b in range(B):
            m = np.array(src[b], dtype=np.uint8, copy=True)
            r = np.nonzero(pick[c, b])[0]
            cx, cy = locs[b, r, 0] // patch_size, locs[b, r, 1] // patch_size
            m[cx, cy] = 1 if set_cells else 0
            row.append(m)
            left[c, b] = np.count_nonzero(m)
        masks.append(row)
    return masks, left


def visited_overlap(bitmaps: Sequence[np.ndarray], locs_m, num_m, patch_size: int) -> np.ndarray:
    """[C * B] int32: the rows r < num_m[v] of locs_m [C * B, Nm, 2] whose cell is non-zero in bitmaps[v % B]."""
    locs_m, num_m = np.asarray(locs_m), np.asarray(num_m)
    B = len(bitmaps)
    out = np.zeros(len(num_m), np.int32)
    for v in range(len(num_m)):
        cells = locs_m[v, :int(num_m[v])] // patch_size
        out[v] = np.count_nonzero(bitmaps[v % B][cells[:, 0], cells[:, 1]])
    return out
