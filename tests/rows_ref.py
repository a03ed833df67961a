"""Float64 references of the row-wise backward kernels (csrc/bwd_rows.hip, csrc/generic_bwd.hip), the slab reductions
(csrc/gemm_bwd.hip, csrc/reduce_multi.hip) and the gradients passed between levels (csrc/select.hip).

Every derivative is evaluated in float64 FROM THE SAME fp32 SAVED TENSORS THE KERNEL READS (o, tc, frm, alpha, hid, pproj, xhat,
rstd), not from recomputed pre-activations: the conditioning of 1 - o near o = 1, or of 1 - alpha, is then not counted as kernel
error.  tests/test_cpu_rows_reference.py checks each closed form against torch.autograd over the oracle's forward formulas.

Conventions the kernels rely on (include/paths_hip.h, paths_amd/backward.py):
  - rows are [B * N] with N = rows_per_slide; row b * N + i is valid iff i < num_ims[b].  Every row-wise kernel writes every row:
    padded rows get exact zeros (the weight-gradient GEMMs read them).
  - LSTM (reference model/interface.py:49-56): f, r = sigmoid, m = tanh of the gate pre-activations, c1 = c0 f + r m,
    o = sigmoid, tc = tanh(Wc c1 + bc), h1 = o tc.  frm [M, 3 Hc] holds f | r | m AFTER the activation, packed per 32-unit block:
    unit j = 32 blk + jj sits at columns 96 blk + jj (f), 96 blk + 32 + jj (r), 96 blk + 64 + jj (m).  The gate gradient dG
    [M, 3 Hc + D] uses the same packing for df | dr | dm in columns [0, 3 Hc) (paths_lstm_bwd_b) and holds dpre_o in columns
    [3 Hc, 3 Hc + D) (paths_lstm_bwd_a).  Each kernel leaves the other's columns untouched.
      lstm_bwd_a: dpre_o = g tc o (1 - o), dpre_h = g o (1 - tc^2), g = dh1 (+ dh1b, the h half of d_state_out)
      lstm_bwd_b: dc = dc1_h (+ dc1_ext, the c half of d_state_out); df = dc c0 f (1 - f), dr = dc m r (1 - r), dm = dc r (1 - m^2),
                  dc0 = dc f   (c0 = 0 at depth 0: c0 null)
  - importance + proj_in (reference model/paths.py:95-98,119-124): hid = relu(Y W1^T + b1), alpha = valid sigmoid(w2 . hid + b2),
    P = pproj = Y Wp^T, tokens[b, 1 + i] = alpha P + bp + PE (importance_mode mul) or P + bp + PE (none).  The kernels read the
    token gradient at dtok[b, i + 1] (row 0 of every slide is the special token, never read).
      du [M, ldu] = [dhid (Hi) | dP (d) | zeros up to ldu]: dP = alpha g (mul) or g, dalpha = g . P (mul) or 0,
      dz = dalpha alpha (1 - alpha) on valid rows, dhid = (hid > 0) dz w2 (gradient of the pre-relu), da = dz, dah = dz hid.
    The lstm = false form (paths_importance_rows_bwd*) has Z = alpha X: dalpha = dZ . X over the D columns, dh = (hid > 0) dz w2.
  - LayerNorm (nn.LayerNorm, eps 1e-5): xhat = (x - mean) rstd, rstd = 1 / sqrt(var + eps) (biased variance, over d),
    dx = rstd (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat)); dgamma = sum_rows dy xhat, dbeta = sum_rows dy.
    paths_layernorm_bwd* also write dy xhat; the _sums forms write one slab [sum dy xhat | sum dy | sum dx] (3 d floats) per block of
    rows_per_block rows, which paths_reduce_slabs_f32 adds.
  - child positions (paths_expand_children): child_pos[b, 4 ldk] holds, for child block blk in 0..3 of kept parent i, the row of
    that child in the next level or -1, at index blk * keep_count[b] + i: the stride is the slide's count, not ldk.  The gradient of
    a kept parent is the sum of its surviving children's rows in block order 0..3, starting from 0 (at most four fp32 adds, so the
    plumbing references below are evaluated in fp32 in that order: bit equality, not a tolerance).  Rows of parents that were not
    kept are not written.
"""
from __future__ import annotations

import torch

F64 = torch.float64


def valid_rows(num_ims, N):
    """[B * N] bool: row b * N + i is a patch (i < num_ims[b])."""
    n = torch.as_tensor(num_ims).to(torch.int64).reshape(-1)
    return (torch.arange(N, device=n.device)[None, :] < n[:, None]).reshape(-1)


def _d(t):
    return None if t is None else t.to(F64)


# ---- LSTM -----------------------------------------------------------------------------------------------------------------------
def pack_gates(f, r, m):
    """[M, Hc] x 3 -> [M, 3 Hc] in the packed order of frm / dG (f | r | m per 32-unit block)."""
    M, Hc = f.shape
    return torch.stack((f.reshape(M, Hc // 32, 32), r.reshape(M, Hc // 32, 32), m.reshape(M, Hc // 32, 32)), 2).reshape(M, 3 * Hc)


def unpack_gates(x):
    """[M, 3 Hc] packed -> (f, r, m) [M, Hc] each."""
    M = x.shape[0]
    Hc = x.shape[1] // 3
    g = x.reshape(M, Hc // 32, 3, 32)
    return g[:, :, 0].reshape(M, Hc), g[:, :, 1].reshape(M, Hc), g[:, :, 2].reshape(M, Hc)


def lstm_bwd_a_ref(dh1, dh1b, o, tc, valid):
    """dh1, dh1b (or None), o, tc [M, D] -> (dpre_o, dpre_h) [M, D] float64, zero on padded rows."""
    g = _d(dh1) if dh1b is None else _d(dh1) + _d(dh1b)
    o, tc = _d(o), _d(tc)
    v = valid[:, None]
    return (torch.where(v, g * tc * o * (1 - o), 0.0), torch.where(v, g * o * (1 - tc * tc), 0.0))


def lstm_bwd_b_ref(dc1_h, dc1_ext, frm, c0, valid, swap_rm=False):
    """dc1_h, dc1_ext (or None), c0 (or None: depth 0) [M, Hc], frm [M, 3 Hc] packed -> (dgates [M, 3 Hc] packed, dc0 [M, Hc]).
    swap_rm: read r and m from each other's planes (a wrong reference, for the sensitivity checks)."""
    dc = _d(dc1_h) if dc1_ext is None else _d(dc1_h) + _d(dc1_ext)
    f, r, m = (_d(t) for t in unpack_gates(frm))
    if swap_rm:
        r, m = m, r
    cp = torch.zeros_like(dc) if c0 is None else _d(c0)
    v = valid[:, None]
    df = torch.where(v, dc * cp * f * (1 - f), 0.0)
    dr = torch.where(v, dc * m * r * (1 - r), 0.0)
    dm = torch.where(v, dc * r * (1 - m * m), 0.0)
    return pack_gates(df, dr, dm), torch.where(v, dc * f, 0.0)


# ---- importance MLP + scaling + proj_in ------------------------------------------------------------------------------------------
def importance_bwd_ref(dtok, pproj, hid, alpha, w2, valid, N, imp_mul):
    """dtok [B, N + 1, d] (row 0: special token), pproj [M, d], hid [M, Hi], alpha [M], w2 [Hi] ->
    (dhid [M, Hi], dP [M, d], da [M], dah [M, Hi]) float64.  Also returns the per-row terms |g_c P_c| summed (the conditioning of
    dalpha) as the fifth value."""
    B = dtok.shape[0]
    d = dtok.shape[-1]
    g = _d(dtok)[:, 1:N + 1].reshape(B * N, d)
    g = torch.where(valid[:, None], g, 0.0)
    P, h, a, w = _d(pproj), _d(hid), _d(alpha), _d(w2).reshape(-1)
    if imp_mul:
        dalpha = (g * P).sum(1)
        dP = a[:, None] * g
    else:
        dalpha = torch.zeros_like(a)
        dP = g
    dz = torch.where(valid, dalpha * a * (1 - a), 0.0)
    dhid = torch.where(h > 0, dz[:, None] * w[None, :], 0.0)
    cond = (g * P).abs().sum(1) * (a * (1 - a)).abs() if imp_mul else torch.zeros_like(a)
    return dhid, dP, dz, dz[:, None] * h, cond


def importance_rows_bwd_ref(dz_rows, x, hid, alpha, w2, valid):
    """lstm = false: dz_rows, x [M, D], hid [M, Hi], alpha [M], w2 [Hi] -> (dh [M, Hi], da [M], dah [M, Hi], cond [M]) float64."""
    g, X, h, a, w = _d(dz_rows), _d(x), _d(hid), _d(alpha), _d(w2).reshape(-1)
    dz = torch.where(valid, (g * X).sum(1) * a * (1 - a), 0.0)
    cond = (g * X).abs().sum(1) * (a * (1 - a)).abs()
    return torch.where(h > 0, dz[:, None] * w[None, :], 0.0), dz, dz[:, None] * h, cond


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
def ln_fwd_ref(x, add, gamma, beta, eps=1e-5, ddof=0):
    """x [rows, d] (+ add [d]) -> (y or None, xhat, rstd [rows]) float64.  ddof = 1: variance over d - 1 (a wrong reference)."""
    v = _d(x) if add is None else _d(x) + _d(add)[None, :]
    mean = v.mean(1, keepdim=True)
    c = v - mean
    var = (c * c).sum(1, keepdim=True) / (v.shape[1] - ddof)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = c * rstd
    y = None if gamma is None else xh * _d(gamma)[None, :] + _d(beta)[None, :]
    return y, xh, rstd[:, 0]


def ln_bwd_ref(dy, xhat, rstd, gamma, ddof=0):
    """dy, xhat [rows, d], rstd [rows], gamma [d] -> dict of float64: dx, dyxhat [rows, d]; dgamma, dbeta, dxsum [d] (column sums
    over the rows) and their conditioning |.|-sums dgamma_abs, dbeta_abs, dxsum_abs.  dx_abs [rows, d] is the conditioning of dx itself,
    rstd (|dy gamma| + mean|dy gamma| + |xhat| mean|dy gamma xhat|): dx cancels, so the column sum of dx is judged against the column
    sum of dx_abs.  ddof = 1: means over d - 1 (a wrong reference)."""
    dy, xh, rs, g = _d(dy), _d(xhat), _d(rstd), _d(gamma)
    n = dy.shape[1] - ddof
    dg = dy * g[None, :]
    m1 = dg.sum(1, keepdim=True) / n
    m2 = (dg * xh).sum(1, keepdim=True) / n
    dx = rs[:, None] * (dg - m1 - xh * m2)
    dx_abs = rs.abs()[:, None] * (dg.abs() + dg.abs().sum(1, keepdim=True) / n + xh.abs() * (dg * xh).abs().sum(1, keepdim=True) / n)
    dyx = dy * xh
    return {"dx": dx, "dyxhat": dyx, "dgamma": dyx.sum(0), "dbeta": dy.sum(0), "dxsum": dx.sum(0), "dx_abs": dx_abs,
            "dgamma_abs": dyx.abs().sum(0), "dbeta_abs": dy.abs().sum(0), "dxsum_abs": dx_abs.sum(0)}


# ---- the gradients passed between levels (fp32, block order) --------------------------------------------------------------------
def _children(child_pos, keep_count, b, ldk, i):
    c = int(keep_count[b])
    return [int(child_pos[b, blk * c + i]) for blk in range(4)]


def sibling_sum_ref(src, child_pos, keep_count, ldk, width, dst, keep_idx=None):
    """dst[b, row(i), :width] = sum over blk = 0..3 of src[b, child_pos[b, blk * count + i], :width] (holes: -1 skipped), in fp32,
    starting from 0, for i < keep_count[b]; row(i) = keep_idx[b, i] or i.  src [B, n_src, >= width], dst [B, n_dst, >= width] (a
    copy is returned; other rows and columns untouched).  Also the reference of paths_gather_rows_bwd (width = Dp)."""
    out = dst.clone()
    cp, kc = child_pos.cpu(), keep_count.cpu()
    ki = keep_idx.cpu() if keep_idx is not None else None
    B = src.shape[0]
    for b in range(B):
        c = int(kc[b])
        if c == 0:
            continue
        pos = cp[b, :4 * c].reshape(4, c).to(torch.int64)            # [blk, i]
        s = torch.zeros((c, width), dtype=src.dtype, device=src.device)
        for blk in range(4):
            p = pos[blk].to(src.device)
            rows = src[b, p.clamp(min=0), :width]
            s = s + torch.where((p >= 0)[:, None], rows, torch.zeros_like(rows))
        dst_rows = torch.arange(c) if ki is None else ki[b, :c].to(torch.int64)
        out[b, dst_rows.to(src.device), :width] = s
    return out


def scatter_kept_rows_ref(src, keep_idx, keep_count, dst, width):
    """dst[b, keep_idx[b, i], :width] = src[b, i, :width] for i < keep_count[b]; src [B, ldk, >= width]."""
    out = dst.clone()
    for b in range(src.shape[0]):
        c = int(keep_count[b])
        out[b, keep_idx[b, :c].to(torch.int64), :width] = src[b, :c, :width]
    return out


def gather_kept_rows_ref(src, keep_idx, keep_count, ldk, D):
    """out[b, i] = src[b, keep_idx[b, i], :D] for i < keep_count[b], zeros beyond: [B, ldk, D]."""
    B = src.shape[0]
    out = torch.zeros((B, ldk, D), dtype=src.dtype, device=src.device)
    for b in range(B):
        c = int(keep_count[b])
        out[b, :c] = src[b, keep_idx[b, :c].to(torch.int64), :D]
    return out
