"""Float64 restatement of the two row kernels of the frozen-path attributions (include/paths_hip.h: paths_path_points /
paths_path_accumulate, with the counter-based Gaussian generator), and the oracle run along a recorded path: the reference of
paths_amd.saliency.integrated_gradients / smooth_grad for the CPU and GPU tests."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from paths_amd import synthetic as syn

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------
# the generator (csrc/dropout.h: drop_hash; include/paths_hip.h: paths_path_points)
# ------------------------------------------------------------------------------------------------
def drop_hash(idx, key_lo: int, key_hi: int) -> np.ndarray:
    """fmix32(((uint32) idx * 0x9E3779B1 + key_lo) ^ fmix32((uint32)(idx >> 32) * 0x85EBCA77 + key_hi)) on uint64 arrays."""
    idx = np.asarray(idx, np.uint64)
    inner = syn.fmix32((((idx >> np.uint64(32)) & M32) * np.uint64(0x85EBCA77) + np.uint64(key_hi)) & M32)
    return syn.fmix32(((((idx & M32) * np.uint64(0x9E3779B1)) + np.uint64(key_lo)) & M32) ^ inner)


def gauss(key_lo: int, key_hi: int, e) -> np.ndarray:
    """z(key, e) in float64: one Box-Muller pair per element pair (e & ~1, e | 1); the cosine for even e, the sine for odd e."""
    e = np.asarray(e, np.uint64)
    h0 = drop_hash(e & ~np.uint64(1), key_lo, key_hi)
    h1 = drop_hash(e | np.uint64(1), key_lo, key_hi)
    u1 = ((h0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = (h1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.where((e & np.uint64(1)) == 0, rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2))


def split_key(key: int):
    return int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------
# the two kernel contracts
# ------------------------------------------------------------------------------------------------
def path_points(x, base, alpha, sigma, keys, num_ims):
    """x [B,N,D], base [D] or None, alpha / sigma [C], keys [C*B] python ints, num_ims [B].  Returns (out, det, rms) in float64:
    out [C*B,N,D], det = |base| + |alpha (x - base)| (the scale of the noise-free part's bound), rms [B,N]; zero on padded rows."""
    x = np.asarray(x, np.float64)
    B, N, D = x.shape
    C = len(alpha)
    bs = np.zeros(D) if base is None else np.asarray(base, np.float64)
    valid = np.arange(N)[None, :] < np.asarray(num_ims)[:, None]
    xv = np.where(valid[..., None], x, 0.0)
    rms = np.sqrt((xv * xv).sum(-1) / D)
    out = np.zeros((C * B, N, D))
    det = np.zeros((C * B, N, D))
    e = (np.arange(N, dtype=np.uint64)[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None, :])
    for c in range(C):
        for b in range(B):
            v = c * B + b
            t = float(alpha[c]) * (xv[b] - bs)
            o = bs + t
            if float(sigma[c]) != 0.0:
                o = o + float(sigma[c]) * rms[b][:, None] * gauss(*split_key(keys[v]), e)
            out[v] = o * valid[b][:, None]
            det[v] = (np.abs(bs) + np.abs(t)) * valid[b][:, None]
    return out, det, rms


def path_accumulate(dx, x, base, w, num_ims):
    """dx [C*B,N,D], x [B,N,D], w [C].  Returns float64 (gxi [B,N], sq [B,N], adx [B,N,D], abs_gxi, abs_sq): the weighted sums over
    the members and sum_c |w_c| sum_d |dx (x - base)| / sum_c |w_c| sum_d dx^2 (the scales of the bounds); zero on padded rows."""
    dx, x = np.asarray(dx, np.float64), np.asarray(x, np.float64)
    B, N, D = x.shape
    C = len(w)
    bs = np.zeros(D) if base is None else np.asarray(base, np.float64)
    valid = (np.arange(N)[None, :] < np.asarray(num_ims)[:, None])
    t = np.where(valid[..., None], x - bs, 0.0)
    d = np.where(valid[None, ..., None], dx.reshape(C, B, N, D), 0.0)
    wv = np.asarray(w, np.float64)[:, None, None]
    g = (d * t[None]).sum(-1)
    q = (d * d).sum(-1)
    return ((wv * g).sum(0), (wv * q).sum(0), (wv[..., None] * d).sum(0), (np.abs(wv) * np.abs(d * t[None]).sum(-1)).sum(0),
            (np.abs(wv) * q).sum(0))


# ------------------------------------------------------------------------------------------------
# the oracle along a recorded path
# ------------------------------------------------------------------------------------------------
def target_of(name: str, logits: torch.Tensor) -> torch.Tensor:
    if name == "risk":
        return -torch.cumprod(1 - torch.sigmoid(logits), dim=1).sum(dim=1)
    assert name.startswith("logit:")
    return logits[:, int(name[6:])]


def recorded_rows(grids, otrace, patch_size: int = 256) -> List[torch.Tensor]:
    """The feature rows the oracle's recursion visited, per level [B,N,D] in the oracle trace's own row order (zero on padding).
    ``grids``: per slide, an object with ``rows(level, x, y)`` (oracle.paths_oracle.DenseGrids / LazyGrids)."""
    out = []
    for l, rec in enumerate(otrace):
        B, N = rec["locs"].shape[:2]
        rows = None
        for b in range(B):
            n = int(rec["num_ims"][b])
            cells = torch.div(rec["locs"][b, :n], patch_size, rounding_mode="floor")
            r = grids[b].rows(l, cells[:, 0], cells[:, 1]).detach()
            if rows is None:
                rows = torch.zeros((B, N, r.shape[1]), dtype=r.dtype)
            rows[b, :n] = r
        out.append(rows)
    return out


def oracle_order(rec, orec, b: int, patch_size: int = 256) -> torch.Tensor:
    """Row indices into slide ``b`` of the HIP trace record ``rec`` in the order of the oracle record ``orec``: rows are matched by
    location (the two location sets must be identical)."""
    n = int(orec["num_ims"][b])
    assert int(rec["num_ims"][b]) == n
    where = {tuple(c): i for i, c in enumerate(torch.div(rec["locs"][b, :n].cpu(), patch_size, rounding_mode="floor").tolist())}
    ocells = torch.div(orec["locs"][b, :n], patch_size, rounding_mode="floor").tolist()
    assert len(where) == n and sorted(where) == sorted(map(tuple, ocells)), f"slide {b}: the location sets differ"
    return torch.tensor([where[tuple(c)] for c in ocells], dtype=torch.int64)


def to_oracle_order(trace, otrace, key: str, patch_size: int = 256) -> List[torch.Tensor]:
    """trace[l][key] ([B,N,...]; "points": [S,B,N,D]) re-ordered into the oracle's rows, per level (CPU, zero on padding)."""
    out = []
    for rec, orec in zip(trace, otrace):
        t = rec[key].detach().cpu()
        if key != "points":
            t = t[None]
        B, N = orec["locs"].shape[:2]
        o = torch.zeros((t.shape[0], B, N) + tuple(t.shape[3:]), dtype=t.dtype)
        for b in range(B):
            idx = oracle_order(rec, orec, b, patch_size)
            o[:, b, :len(idx)] = t[:, b, idx]
        out.append(o if key == "points" else o[0])
    return out


def frozen_path(params, ocfg, grids, otrace, points_per_level: Optional[Sequence[torch.Tensor]] = None, target: str = "risk"):
    """The oracle's levels (process_level) over the oracle trace's OWN recorded locs / keep_inds / parent_inds, with the given rows
    [B,N,D] per level (oracle row order; None: the recorded rows of ``grids``) as features.  The selection is never re-made (no
    top-K) and the background predicate never re-evaluated: a child's parent state is out["ctx_patch"] of the recorded parent row,
    zero for the rows of a slide that took the fallback.  Returns {"target" [B], "logits" [B,C], "grads": d sum(target) / d rows per
    level}."""
    from oracle import paths_oracle as orc
    L = len(otrace)
    rows = recorded_rows(grids, otrace, ocfg.patch_size) if points_per_level is None else points_per_level
    leaves = [r.detach().clone().requires_grad_(True) for r in rows]
    B = leaves[0].shape[0]
    Dp = ocfg.patch_embed_dim + (ocfg.hierarchical_ctx_mlp_hidden_dim if ocfg.lstm else 0)
    dt = leaves[0].dtype
    ctx_slide = torch.zeros((B, 0, ocfg.trans_dim), dtype=dt)
    ctx_patch = torch.zeros((B, leaves[0].shape[1], 0, Dp), dtype=dt)
    out = None
    for l in range(L):
        rec = otrace[l]
        assert leaves[l].shape[:2] == rec["locs"].shape[:2]
        out = orc.process_level(params, ocfg, l, leaves[l], rec["locs"], rec["num_ims"], ctx_slide, ctx_patch)
        if l == L - 1:
            break
        nxt = otrace[l + 1]
        ctx_slide = torch.cat((ctx_slide, out["ctx_slide"][:, None]), dim=1)
        ctx_patch = torch.zeros((B, nxt["locs"].shape[1], 1, Dp), dtype=dt)
        for b in range(B):
            if nxt["fallback"][b]:
                continue
            n = int(nxt["num_ims"][b])
            parent_row = rec["keep_inds"][b][nxt["parent_inds"][b, :n]]
            ctx_patch[b, :n, 0] = out["ctx_patch"][b, parent_row]
    tgt = target_of(target, out["logits"])
    grads = torch.autograd.grad(tgt.sum(), leaves, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(x) for g, x in zip(grads, leaves)]
    return {"target": tgt.detach(), "logits": out["logits"].detach(), "grads": grads}


def normal_cdf(z: np.ndarray) -> np.ndarray:
    return 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(z, np.float64) / math.sqrt(2.0)))
