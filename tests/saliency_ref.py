"""Float64 restatement of the saliency row contract (include/paths_hip.h: paths_saliency_rows) and the error bounds its kernel is
held to, for the CPU and GPU tests."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of an n-term fp32 sum of products in ANY order."""
    return n * U / (1.0 - n * U)


def saliency_rows(dx: np.ndarray, x: np.ndarray, num_ims: np.ndarray):
    """dx, x [B,N,D]; num_ims [B].  Returns (gxi [B,N], gnorm [B,N], absdot [B,N]) in float64: sum_d dx x, sqrt(sum_d dx^2) and
    sum_d |dx x| (the scale of the gxi bound); rows at or beyond num_ims[b] are zero in all three."""
    dx, x = np.asarray(dx, np.float64), np.asarray(x, np.float64)
    B, N, _ = dx.shape
    valid = np.arange(N)[None, :] < np.asarray(num_ims)[:, None]
    gxi = (dx * x).sum(-1) * valid
    gnorm = np.sqrt((dx * dx).sum(-1)) * valid
    absdot = np.abs(dx * x).sum(-1) * valid
    return gxi, gnorm, absdot


def risk_score(logits: np.ndarray) -> np.ndarray:
    """-sum_k cumprod(1 - sigmoid(logits))_k in float64 (reference eval.py:60-61)."""
    h = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)))
    return -np.cumprod(1.0 - h, axis=1).sum(axis=1)
