"""Float64 reference of the masked self-attention and its gradients, the yardstick of the attention backward kernels.

Per slide b only the first lens[b] tokens exist: scores = score_mul * q k^T over those keys, P = softmax(scores), the attention
probabilities that reach V are P * drop_mask (mask multipliers already scaled by 1 / (1 - p16)), O = (P * drop_mask) V.  The loss is
sum <O[q], d_o[q]> over the valid queries q < max_queries (max_queries = 0: all of them); dq / dk / dv are its gradients by
torch.autograd in float64, on whichever device the inputs are on.  Rows >= lens[b] of every output are zero, and so are the rows
>= max_queries of o, lse and dq: queries without an output gradient are not evaluated.

Kernel conventions (include/paths_hip.h):
  - head-major kernels (x6, f32, token0): q is stored pre-scaled by log2(e) / sqrt(hd), so score_mul = ln 2 and dq is the gradient of
    that pre-scaled q;
  - token-major kernels (any, wide): q is unscaled, score_mul = qscale * ln 2 with qscale = log2(e) / sqrt(hd), dq is the gradient
    of the unscaled q;
  - lse is in the log2 domain: log2 sum_k exp2(scores / ln 2), the softmax before dropout.
"""
from __future__ import annotations

import math

import torch

LN2 = math.log(2.0)


def attn_ref_fwd_bwd(q, k, v, lens, score_mul, d_o, drop_mask=None, max_queries=0):
    """q, k, v, d_o [B, H, T, hd]; drop_mask [B, H, >= T or >= max_queries, T] multipliers or None.  Returns float64 tensors
    o, dq, dk, dv [B, H, T, hd] and lse [B, H, T] (log2 domain)."""
    B, H, T, hd = q.shape
    f64 = dict(dtype=torch.float64, device=q.device)
    out = {n: torch.zeros((B, H, T, hd), **f64) for n in ("o", "dq", "dk", "dv")}
    out["lse"] = torch.zeros((B, H, T), **f64)
    for b, n in enumerate(lens):
        n = int(n)
        nq = min(n, max_queries) if max_queries > 0 else n
        qb = q[b, :, :nq].to(torch.float64).requires_grad_(True)
        kb, vb = (x[b, :, :n].to(torch.float64).requires_grad_(True) for x in (k, v))
        s = score_mul * (qb @ kb.transpose(1, 2))
        p = torch.softmax(s, dim=-1)
        if drop_mask is not None:
            p = p * drop_mask[b, :, :nq, :n].to(torch.float64)
        o = p @ vb
        (o * d_o[b, :, :nq].to(torch.float64)).sum().backward()
        out["o"][b, :, :nq] = o.detach()
        out["lse"][b, :, :nq] = torch.logsumexp(s.detach(), dim=-1) / LN2
        out["dq"][b, :, :nq], out["dk"][b, :, :n], out["dv"][b, :, :n] = qb.grad, kb.grad, vb.grad
    return out
