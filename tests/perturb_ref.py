"""numpy restatement of the two kernels of the deletion / insertion curves (include/paths_hip.h: paths_rank_joint /
paths_path_mask_points) and of the count formula of paths_amd.saliency.perturbation_curves: the reference of the CPU and GPU tests."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def valid_mask(seg: Sequence[int], num_ims, level_on: Optional[Sequence[int]] = None) -> np.ndarray:
    """[B, Ntot] bool: the joint elements that are ranked.  seg: the level capacities N_l; num_ims [L, B]; level_on [L] (None: all)."""
    num_ims = np.asarray(num_ims)
    L, B = num_ims.shape
    on = [1] * L if level_on is None else list(level_on)
    return np.concatenate([(np.arange(n)[None, :] < num_ims[l][:, None]) & bool(on[l]) for l, n in enumerate(seg)], axis=1)


def rank_joint(scores, seg: Sequence[int], num_ims, level_on: Optional[Sequence[int]] = None, ascending: bool = False):
    """(rank [B, Ntot] int32, count [B] int32): np.lexsort on (joint index, -value; +value with ``ascending``) over the valid elements,
    -0 read as +0; -1 where an element is not valid.  Scores of elements that are not valid are not looked at."""
    scores = np.asarray(scores, np.float32)
    valid = valid_mask(seg, num_ims, level_on)
    assert scores.shape == valid.shape
    rank = np.full(scores.shape, -1, np.int32)
    for b in range(scores.shape[0]):
        idx = np.nonzero(valid[b])[0]
        v = scores[b, idx].astype(np.float64) + 0.0                 # (-0) + (+0) = +0
        order = np.lexsort((idx, v if ascending else -v))
        rank[b, idx[order]] = np.arange(len(idx), dtype=np.int32)
    return rank, valid.sum(1).astype(np.int32)


def kept(rank, thr, insert, num_ims) -> np.ndarray:
    """[C, B, N] bool: the rows a member keeps.  rank [B, N]; thr [C, B]; insert [C]; num_ims [B].  Padded rows: False."""
    rank, thr, insert = np.asarray(rank), np.asarray(thr), np.asarray(insert)
    valid = np.arange(rank.shape[1])[None, :] < np.asarray(num_ims)[:, None]
    k = np.where(insert[:, None, None] != 0, rank[None] < thr[:, :, None], rank[None] >= thr[:, :, None]) | (rank[None] < 0)
    return k & valid[None]


def mask_points(x, base, rank, thr, insert, num_ims) -> np.ndarray:
    """out [C*B, N, D] in x's dtype: np.where between the recorded row and the baseline (None: +0), +0 on padded rows.  No arithmetic:
    compare the result bit for bit."""
    x = np.asarray(x)
    B, N, D = x.shape
    k = kept(rank, thr, insert, num_ims)
    valid = np.arange(N)[None, :] < np.asarray(num_ims)[:, None]
    bs = np.zeros(D, x.dtype) if base is None else np.asarray(base, x.dtype)
    out = np.where(k[..., None], x[None], np.broadcast_to(bs, x.shape)[None])
    out = np.where(valid[None, :, :, None], out, np.zeros((), x.dtype))
    return out.reshape(len(k) * B, N, D)


def counts(n, steps: int) -> np.ndarray:
    """[steps + 1, B]: (2 s n_b + steps) // (2 steps), python integers."""
    return np.array([[(2 * s * int(nb) + steps) // (2 * steps) for nb in n] for s in range(steps + 1)], dtype=np.int64).reshape(steps + 1, len(n))


def curve_members(count, steps: int):
    """(thr [2 (steps + 1), B], insert [2 (steps + 1)]): the deletion points s = 0 .. steps followed by the insertion points."""
    c = counts(count, steps)
    return np.concatenate([c, c]), np.concatenate([np.zeros(steps + 1, np.int64), np.ones(steps + 1, np.int64)])
