"""Plain references of the forward LSTM cell and of the importance / projection / positional-encoding step, in pure torch and with
no project kernel, plus the per-element forward-error bounds the kernel tests hold the HIP kernels to.

Both references are dtype- and device-agnostic: on float64 copies of the fp32 operands they are the reference; on the fp32 operands
themselves (on the device) they are "the same formula evaluated by torch in fp32" of the tests' second condition.

Bounds (all computed in float64 from the reference's own intermediate values; U = 2^-23 bounds one fp32 ulp relative to a value):
  * a dot product with S = sum_k |a_k| |w_k| is off by at most GEMM_REL * S (the bar tests/test_gpu_parity.py::test_x6_gemm_matches_fp64
    holds these GEMMs to, for planes 2, 3 and the f32 kernel), plus U times the sum of the magnitudes that meet in the additions around
    it (bias, the parent partial `hp`, the product itself): each of those additions rounds once, at the magnitude of its operands;
  * an activation adds ACT = 2e-7 absolute (csrc/common.h documents 1e-7 for tanh_acc; twice that covers the result's own rounding;
    sigmoid_acc is held to the same); sigmoid is 1/4-Lipschitz, tanh and relu 1-Lipschitz;
  * every further product or sum adds U times its magnitude.
"""
from __future__ import annotations

import math

import torch

GEMM_REL = 5e-7
ACT = 2e-7
U = 2.0 ** -23

GATES = ("forget_gate", "remember_gate", "remember_map", "out_select_gate", "mem_to_out")


# ------------------------------------------------------------------------------------------------
# packed layouts (what ops.pack_lstm / ops.pack_level build; tests/test_cpu_chain_reference.py pins them to those)
# ------------------------------------------------------------------------------------------------
def packed_gate_columns(Hc: int, D: int):
    """(f, r, m, o): for every memory unit / output channel its column in the packed gate order: 96-column groups
    [forget(32) | remember(32) | map(32)] of one block of 32 memory units, then the D output-gate columns."""
    u = torch.arange(Hc)
    base = 96 * (u // 32) + u % 32
    return base, base + 32, base + 64, 3 * Hc + torch.arange(D)


def pack_gates(w: dict):
    """(w_gates [3Hc + D, 2D], b_gates [3Hc + D]) in the packed row order, from the five modules' tensors."""
    Hc, D = w["forget_gate.weight"].shape[0], w["out_select_gate.weight"].shape[0]
    cf, cr, cm, co = packed_gate_columns(Hc, D)
    wg = w["forget_gate.weight"].new_zeros((3 * Hc + D, w["forget_gate.weight"].shape[1]))
    bg = w["forget_gate.bias"].new_zeros((3 * Hc + D,))
    for name, cols in (("forget_gate", cf), ("remember_gate", cr), ("remember_map", cm), ("out_select_gate", co)):
        wg[cols.to(wg.device)] = w[name + ".weight"]
        bg[cols.to(wg.device)] = w[name + ".bias"]
    return wg, bg


def interleave_ip(w1, wp):
    """[W1[0:64] ; Wp[0:64] ; W1[64:128] ; Wp[64:128]]: the row order of the forward importance / projection weight."""
    return torch.cat([w1[:64], wp[:64], w1[64:], wp[64:]], dim=0)


# ------------------------------------------------------------------------------------------------
# LSTM cell
# ------------------------------------------------------------------------------------------------
def lstm_ref(w: dict, x, prev=None, bounds: bool = False):
    """reference model/interface.py:49-56 (oracle.lstm_cell's formulas) + Y = X + h1.

    w: "<gate>.weight" / "<gate>.bias" of the five modules (gate weights [*, 2D] over [x | h], mem_to_out [D, Hc]); x [M, D].
    prev: None (zero state) | {"h0": [M, D], "c0": [M, Hc]} | {"hp": [rows, 3Hc + D] (the h half of the pre-activations per parent, in
    the packed column order: an INPUT, its value is added as it is), "hp_row": [M] integers (< 0: zero), "c0": [M, Hc]}.
    Returns f, r, m, c1, o, tc, h1, y; with bounds=True also "tol_<name>" per element (see the module docstring):
      d(gate)  = GEMM_REL * S + U * (|x part| + |h part| + |bias| + |pre|)
      tol(f), tol(r), tol(o) = d / 4 + ACT;  tol(m) = d + ACT
      tol(c1)  = |c0| tol(f) + tol(r) + tol(m) + U * (|c0 f| + |r m| + |c1|)
      d(tc)    = |Wc| tol(c1) + GEMM_REL * (|c1| |Wc|^T) + U * (|Wc c1| + |bc| + |pre|);  tol(tc) = d(tc) + ACT
      tol(h1)  = tol(o) + tol(tc) + U * |h1|;   tol(y) = tol(h1) + U * (|x| + 1)
    """
    M, D = x.shape
    Hc = w["forget_gate.weight"].shape[0]
    cols = dict(zip(GATES[:4], packed_gate_columns(Hc, D)))
    c0 = None if prev is None else prev["c0"]
    out, mags = {}, {}
    for g in GATES[:4]:
        W, b = w[g + ".weight"], w[g + ".bias"]
        xp = x @ W[:, :D].T
        S = x.abs() @ W[:, :D].abs().T
        if prev is None:
            hpart = torch.zeros_like(xp)
        elif "h0" in prev:
            hpart = prev["h0"] @ W[:, D:].T
            S = S + prev["h0"].abs() @ W[:, D:].abs().T
        else:
            row = prev["hp_row"].long()
            hpart = prev["hp"][row.clamp(min=0)][:, cols[g].to(x.device)] * (row >= 0)[:, None].to(x.dtype)
        pre = xp + hpart + b
        out[g] = pre
        mags[g] = GEMM_REL * S + U * (xp.abs() + hpart.abs() + b.abs() + pre.abs())
    f, r, o = torch.sigmoid(out["forget_gate"]), torch.sigmoid(out["remember_gate"]), torch.sigmoid(out["out_select_gate"])
    m = torch.tanh(out["remember_map"])
    c0v = torch.zeros_like(f) if c0 is None else c0
    c1 = c0v * f + r * m
    Wc, bc = w["mem_to_out.weight"], w["mem_to_out.bias"]
    ptc = c1 @ Wc.T + bc
    tc = torch.tanh(ptc)
    h1 = o * tc
    res = {"f": f, "r": r, "m": m, "c1": c1, "o": o, "tc": tc, "h1": h1, "y": x + h1}
    if bounds:
        tf, tr, to = (mags[g] / 4 + ACT for g in ("forget_gate", "remember_gate", "out_select_gate"))
        tm = mags["remember_map"] + ACT
        tc1 = c0v.abs() * tf + tr + tm + U * ((c0v * f).abs() + (r * m).abs() + c1.abs())
        dtc = tc1 @ Wc.abs().T + GEMM_REL * (c1.abs() @ Wc.abs().T) + U * ((c1 @ Wc.T).abs() + bc.abs() + ptc.abs())
        ttc = dtc + ACT
        th = to + ttc + U * h1.abs()
        res.update({"tol_f": tf, "tol_r": tr, "tol_m": tm, "tol_c1": tc1, "tol_o": to, "tol_tc": ttc, "tol_h1": th,
                    "tol_y": th + U * (x.abs() + 1)})
    return res


LSTM_ACTIVATIONS = {"f": 1, "r": 1, "m": 1, "o": 1, "c1": 3, "tc": 4, "h1": 5, "y": 5}     # activations on each output's path


def packed_frm(res: dict, suffix: str = ""):
    """[M, 3Hc]: f | r | m (or their bounds, suffix "tol_") in the packed column order of save_frm."""
    f = res[suffix + "f"]
    M, Hc = f.shape
    cf, cr, cm = (c.to(f.device) for c in packed_gate_columns(Hc, 0)[:3])
    out = f.new_zeros((M, 3 * Hc))
    out[:, cf], out[:, cr], out[:, cm] = f, res[suffix + "r"], res[suffix + "m"]
    return out


# ------------------------------------------------------------------------------------------------
# positional encoding: the angle is the FP32 product of the fp32 position and the fp32 div_term entry; sin / cos of that fp32 value
# ------------------------------------------------------------------------------------------------
def pe_angles(pos, div_term, reps: int):
    """[n, reps * 2 * len(div_term)] fp32 angles: channel c of a group of 2 * len(div_term) uses div_term[c >> 1]."""
    ang = pos.to(torch.float32)[:, None] * div_term.to(torch.float32)[None, :]          # fp32 product: part of the contract
    return ang.repeat_interleave(2, dim=1).repeat(1, reps)


def pe_values(ang32, dtype=torch.float64):
    """sin (even channels) / cos (odd channels) of the fp32 angles, evaluated in ``dtype``."""
    a = ang32.to(dtype)
    even = (torch.arange(a.shape[1], device=a.device) % 2 == 0)[None, :]
    return torch.where(even, torch.sin(a), torch.cos(a))


def pe_ref(pe_mode: int, d: int, div_term, locs=None, patch_size: int = 1, idx=None, dtype=torch.float64):
    """[M, d].  pe_mode 2: channels [0, d/2) from floor(x / patch_size), [d/2, d) from floor(y / patch_size), div_term has d/4
    entries; pe_mode 1: every channel from the row's index within its slide, div_term has d/2 entries (reference utils.py:16-23,47-67)."""
    if pe_mode == 2:
        pos = torch.div(locs, patch_size, rounding_mode="floor")
        return torch.cat([pe_values(pe_angles(pos[:, 0], div_term, 1), dtype), pe_values(pe_angles(pos[:, 1], div_term, 1), dtype)], dim=1)
    return pe_values(pe_angles(idx, div_term, 1), dtype)


def pe_table_ref(pe_mode: int, d: int, div_term, rows: int, dtype=torch.float64):
    """paths_pe_table's output: [rows, d/2] (pe_mode 2: one coordinate's half) or [rows, d] (pe_mode 1)."""
    return pe_values(pe_angles(torch.arange(rows, device=div_term.device), div_term, 1), dtype)


PE_TOL = 4 * U      # sinf / cosf of the same fp32 angle: 4 ulp (the OpenCL / device-library bound), taken at |value| <= 1


# ------------------------------------------------------------------------------------------------
# importance MLP + masked sigmoid + alpha * proj_in + bias + PE + special token
# ------------------------------------------------------------------------------------------------
def imp_proj_ref(p: dict, Y, locs, num_ims, N: int, patch_size: int, pe_mode: int, imp_mul: int, bounds: bool = False, splitk: bool = False):
    """reference model/paths.py:95-98,119-124; model/aggregator.py:37-65.

    p: W1 [Hi, D], b1, w2 [Hi], b2 [1], Wp [d, D], bp, special [d], div_term (fp32); Y [M = B N, D] (for the kernels' y + y_add forms
    the caller passes the fp32 sum); locs [M, 2] integers (pe_mode 2); num_ims [B].
    Returns importance [M] (0 on padded rows), tokens [B, N + 1, d] (special first; alpha = importance if imp_mul else 1, padded rows
    included: alpha = 0 there with imp_mul, so a padded row's token is bp + PE; with imp_mul = 0 alpha is 1 there too and the token
    is pproj + bp + PE, in the reference model and in the paths_importance_proj* kernels alike), hid (post-relu) and pproj (before
    alpha, bias and PE), valid [M].  bounds=True adds
      tol_hid   = GEMM_REL * S1 + U * (|Y W1^T| + |b1| + |pre|) (+ U |Y W1^T| for the split-K form's one extra addition)
      tol_pproj = GEMM_REL * Sp + U * |pproj|                   (likewise)
      tol_logit = |w2| . tol_hid + 5 U sum |hid w2| + U (|b2| + |logit|)   (one product and at most 9 additions per term of the
                  128-term dot: two in the lane's own sum, five butterfly levels, the two halves, b2; each rounds by <= 2^-24 of a
                  partial sum bounded by sum |hid w2|)
      tol_importance = tol_logit / 4 + ACT on valid rows, 0 on padded ones (exactly 0.0)
      tol_tokens = tol_alpha |pproj| + |alpha| tol_pproj + PE_TOL + U (|alpha pproj| + |bp| + |PE| + |token|); special rows 0 (a copy)
    """
    M, D = Y.shape
    B = num_ims.shape[0]
    d = p["Wp"].shape[0]
    dt = Y.dtype
    idx = torch.arange(M, device=Y.device) % N
    valid = idx < num_ims.to(Y.device).repeat_interleave(N)
    pre1 = Y @ p["W1"].T + p["b1"]
    hid = torch.relu(pre1)
    logit = hid @ p["w2"] + p["b2"]
    imp = torch.where(valid, torch.sigmoid(logit), torch.zeros_like(logit))
    pproj = Y @ p["Wp"].T
    alpha = imp if imp_mul else torch.ones_like(imp)
    pe = pe_ref(pe_mode, d, p["div_term"], locs, patch_size, idx, dt)
    tok = alpha[:, None] * pproj + p["bp"] + pe
    tokens = torch.cat([p["special"].to(dt).view(1, 1, d).expand(B, 1, d), tok.view(B, N, d)], dim=1)
    res = {"importance": imp, "tokens": tokens, "hid": hid, "pproj": pproj, "valid": valid, "pe": pe}
    if bounds:
        extra = 2.0 if splitk else 1.0
        x1 = Y @ p["W1"].T
        thid = GEMM_REL * (Y.abs() @ p["W1"].abs().T) + U * (extra * x1.abs() + p["b1"].abs() + pre1.abs())
        tpp = GEMM_REL * (Y.abs() @ p["Wp"].abs().T) + U * extra * pproj.abs()
        tlogit = thid @ p["w2"].abs() + 5 * U * (hid @ p["w2"].abs()) + U * (p["b2"].abs() + logit.abs())
        timp = torch.where(valid, tlogit / 4 + ACT, torch.zeros_like(tlogit))
        talpha = timp if imp_mul else torch.zeros_like(timp)
        ttok = talpha[:, None] * pproj.abs() + alpha.abs()[:, None] * tpp + PE_TOL \
            + U * ((alpha[:, None] * pproj).abs() + p["bp"].abs() + pe.abs() + tok.abs())
        res.update({"tol_hid": thid, "tol_pproj": tpp, "tol_importance": timp,
                    "tol_tokens": torch.cat([ttok.new_zeros((B, 1, d)), ttok.view(B, N, d)], dim=1)})
    return res


IMP_ACTIVATIONS = {"importance": 1, "tokens": 1, "hid": 0, "pproj": 0}


# ------------------------------------------------------------------------------------------------
# the generic forward row kernels (csrc/generic.hip, the d = 128 twins of csrc/tlayer_f32.hip, paths_pe_table, paths_linear_f32)
# ------------------------------------------------------------------------------------------------
def _ln(v, e_v, gamma, beta, eps: float, nsum: int = 17):
    """(y, tol) of y = (v - mean) / sqrt(var + eps) * gamma + beta over the last axis (biased variance, two passes), for inputs that
    carry an absolute error e_v per element.  A row's sum goes through at most nsum fp32 additions (paths_layernorm_rows: 3 inside a
    4-vector, 8 chunks, 6 butterfly levels = 17), each rounding by <= U / 2 of a partial sum bounded by sum |v|; h = (nsum + 1) / 2:
      e_m   = h U mean|v| + mean(e_v)                     (error of the mean; the division included)
      e_c   = e_m + e_v + U |c|                           (error of c = v - mean)
      d_var = e_m^2 + 2 mean(|c| (U |c| + e_v + mean e_v)) + (h + 2) U var   (the mean's own error enters only squared: sum c = 0)
      r     = d_var / (2 (var + eps)) + 2 U               (relative error of rstd: square root and reciprocal round once each)
      tol   = |gamma| rstd (e_c + |c| (r + 2 U)) + U (|y| + |beta|)"""
    mean = v.mean(dim=-1, keepdim=True)
    c = v - mean
    var = (c * c).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = c * rstd * gamma + beta
    me = e_v.mean(dim=-1, keepdim=True) if torch.is_tensor(e_v) else torch.zeros_like(mean)
    h = (nsum + 1) / 2
    e_m = h * U * v.abs().mean(dim=-1, keepdim=True) + me
    e_c = e_m + e_v + U * c.abs()
    d_var = e_m * e_m + 2 * (c.abs() * (U * c.abs() + e_v + me)).mean(dim=-1, keepdim=True) + (h + 2) * U * var
    r = d_var / (2 * (var + eps)) + 2 * U
    tol = gamma.abs() * rstd * (e_c + c.abs() * (r + 2 * U)) + U * (y.abs() + beta.abs())
    return y, tol


def layernorm_ref(x, add, gamma, beta, eps: float):
    """(y, tol) of paths_layernorm_rows / paths_layernorm_f32: LayerNorm(x (+ add [d])) * gamma + beta; the sum x + add rounds once."""
    v = x if add is None else x + add
    return _ln(v, U * v.abs() if add is not None else 0.0, gamma, beta, eps)


def layernorm2_ref(x, g1, b1, add, g2, b2, eps: float):
    """(y, tol) of paths_layernorm2_rows: LN2(LN1(x) + add); the first norm's bound (and the addition's rounding) is the second's e_v."""
    y1, t1 = _ln(x, 0.0, g1, b1, eps)
    v = y1 if add is None else y1 + add
    return _ln(v, t1 + U * v.abs(), g2, b2, eps)


def importance_rows_ref(hid, w2, b2, num_ims, rps: int, relu: int):
    """(importance [M], tol): valid ? sigmoid((relu ? max(hid, 0) : hid) . w2 + b2) : 0.  A term of the Hi-term dot passes one fma per 64
    columns, six butterfly levels and the + b2: tol_logit = (ceil(Hi / 64) + 7) U / 2 sum |h w2| + U (|b2| + |logit|); tol = / 4 + ACT."""
    M, Hi = hid.shape
    h = torch.relu(hid) if relu else hid
    logit = h @ w2 + b2
    valid = (torch.arange(M, device=hid.device) % rps) < num_ims.repeat_interleave(rps)
    tl = ((Hi + 63) // 64 + 7) * U / 2 * (h.abs() @ w2.abs()) + U * (b2.abs() + logit.abs())
    zero = torch.zeros_like(logit)
    return torch.where(valid, torch.sigmoid(logit), zero), torch.where(valid, tl / 4 + ACT, zero), valid


def tokens_assemble_ref(P, importance, imp_mul: int, bp, special, div_term, locs, N: int, patch_size: int, pe_mode: int):
    """(tokens [B, N + 1, d], tol): special first, then alpha P + bp + PE with alpha = the given importance (0 on padded rows: the token is
    bp + PE there) or 1.  tol = PE_TOL + U (|alpha P| + |bp| + |PE| + |token|); the special rows are copies."""
    M, d = P.shape
    B = M // N
    idx = torch.arange(M, device=P.device) % N
    pe = pe_ref(pe_mode, d, div_term, locs, patch_size, idx, P.dtype)
    a = importance[:, None] if imp_mul else torch.ones_like(P[:, :1])
    tok = a * P + bp + pe
    tol = PE_TOL + U * ((a * P).abs() + bp.abs() + pe.abs() + tok.abs())
    sp = special.to(P.dtype).view(1, 1, d).expand(B, 1, d)
    return torch.cat([sp, tok.view(B, N, d)], dim=1), torch.cat([torch.zeros_like(sp), tol.view(B, N, d)], dim=1)


def importance_tokens_rows_ref(hid, Hi: int, w2, b2, num_ims, N: int, relu: int, imp_mul: int, bp, special, table, locs, patch_size: int,
                               pe_mode: int):
    """(importance [M], tokens [B, N + 1, d], tol_importance, tol_tokens) of paths_importance_tokens_rows over hid [M, Hi + d] = [hidden
    pre-activations | projection P]: importance as importance_rows_ref; token = (valid ? alpha P : 0) + bp + PE with alpha = importance or
    1 and the PE READ from ``table`` (paths_pe_table's layout; an input: its entries are added as they are, so no PE_TOL here); padded
    rows are bp + PE for either imp_mul.  tol_tokens = tol_importance |P| + U (|alpha P| + |bp| + |PE| + |token|); special rows copies."""
    M, d = hid.shape[0], hid.shape[1] - Hi
    B = M // N
    imp, timp, valid = importance_rows_ref(hid[:, :Hi], w2, b2, num_ims, N, relu)
    P = torch.where(valid[:, None], hid[:, Hi:], torch.zeros_like(hid[:, Hi:]))
    if pe_mode == 2:
        pos = torch.div(locs, patch_size, rounding_mode="floor").clamp(0, table.shape[0] - 1)
        pe = torch.cat([table[pos[:, 0]], table[pos[:, 1]]], dim=1)
    else:
        pe = table[(torch.arange(M, device=hid.device) % N).clamp(max=table.shape[0] - 1)]
    pe = pe.to(hid.dtype)
    a = imp[:, None] if imp_mul else torch.ones_like(P[:, :1])
    tok = a * P + bp + pe
    tol = (timp[:, None] * P.abs() if imp_mul else 0.0) + U * ((a * P).abs() + bp.abs() + pe.abs() + tok.abs())
    sp = special.to(hid.dtype).view(1, 1, d).expand(B, 1, d)
    return imp, torch.cat([sp, tok.view(B, N, d)], dim=1), timp, torch.cat([torch.zeros_like(sp), tol.view(B, N, d)], dim=1)


def final_head_ref(x, lng, lnb, ctx_prev, ctx_all, wcls, bcls, eps: float):
    """(ctx_out [B, d], logits [B, L], tol_ctx, tol_logits): f = LayerNorm(x) (+ ctx_prev); logits = wcls [ctx_all flattened | f] + bcls
    (reference model/aggregator.py:75, model/paths.py:130-139).  A term of the classifier's dot passes ceil(cls_in / 64) additions in its
    lane, six butterfly levels and the bias: tol_logits = |w_f| tol_f + (ceil(cls_in / 64) + 8) U / 2 sum |w in| + U |logit|."""
    f, tf = _ln(x, 0.0, lng, lnb, eps, (x.shape[1] + 63) // 64 + 6)      # a lane sums d / 64 values, then six butterfly levels
    if ctx_prev is not None:
        f = f + ctx_prev
        tf = tf + U * f.abs()
    inp = f if ctx_all is None else torch.cat([ctx_all.reshape(x.shape[0], -1), f], dim=1)
    k = f.shape[1]
    logits = inp @ wcls.T + bcls
    steps = (inp.shape[1] + 63) // 64 + 8
    tl = tf @ wcls[:, -k:].abs().T + steps * U / 2 * (inp.abs() @ wcls.abs().T) + U * logits.abs()
    return f, logits, tf, tl


def linear_ref(a, w, b, act: int):
    """(out, tol, S) of paths_linear_f32: act(a W^T + b); tol = GEMM_REL S + U (|a W^T| + |b| + |out|)."""
    prod = a @ w.T
    out = prod if b is None else prod + b
    if act:
        out = torch.relu(out)
    S = a.abs() @ w.abs().T
    return out, GEMM_REL * S + U * (prod.abs() + (b.abs() if b is not None else 0.0) + out.abs()), S


# ------------------------------------------------------------------------------------------------
# the aggregator's decoder layers (reference model/aggregator.py:25-33, 70-75 = torch's post-LN TransformerDecoderLayer over an empty
# memory; model/paths.py:130-139).  A layer is a dict wqkv [3d, d], bqkv, wo, bo, ln1g, ln1b, cab (the cross-attention's out_proj bias:
# all an empty memory leaves of it), ln2g, ln2b, w1 [4d, d], b1, w2 [d, 4d], b2, ln3g, ln3b, eps - the keys of ops.pack_level's layers.
# ------------------------------------------------------------------------------------------------
def _lin(a, e_a, w, b, act: int = 0):
    """(out, tol, S) of act(a W^T + b) for an input that carries the absolute error e_a per element (0.0: exact):
    tol = e_a |W|^T + GEMM_REL S + U (|a W^T| + |b| + |out|), S = |a| |W|^T; relu is 1-Lipschitz."""
    prod = a @ w.T
    out = prod + b
    S = a.abs() @ w.abs().T
    tol = GEMM_REL * S + U * (prod.abs() + b.abs() + out.abs())
    if torch.is_tensor(e_a):
        tol = tol + e_a @ w.abs().T
    return (torch.relu(out) if act else out), tol, S


def in_proj_ref(lay: dict, x, H: int, e_x=0.0):
    """q, k, v [B, H, T, d / H] (q UNscaled) of x [B, T, d], their bounds tol_q / tol_k / tol_v and S_q / S_k / S_v = |x| |W|^T."""
    B, T, d = x.shape
    qkv, tol, S = _lin(x, e_x, lay["wqkv"], lay["bqkv"])
    heads = lambda t: t.view(B, T, H, d // H).transpose(1, 2)
    res = {}
    for i, n in enumerate("qkv"):
        res[n], res["tol_" + n], res["S_" + n] = (heads(t[..., i * d:(i + 1) * d]) for t in (qkv, tol, S))
    return res


def special_index(num_ims, special_last: bool = False):
    """[B] index of the special token: 0 (the reference's order) or num_ims[b] (the fused finish's: patches first)."""
    return num_ims.long() if special_last else torch.zeros_like(num_ims.long())


def attention_ref(q, k, v, num_ims, special_last: bool = False, query: str = "all", qk_scale=None, bounds: bool = False, errs=None):
    """softmax(qk_scale q k^T) v per head (qk_scale: 1 / sqrt(hd), or what the caller's pre-scaled q asks for: ln 2 for a q that holds
    log2(e) / sqrt(hd) times the projection) with keys t < num_ims[b] + 1 valid (the special token and the patches of the slide, in
    EITHER token order: the special token is row 0, or - special_last - row num_ims[b], right behind the patches; the valid keys are
    rows [0, num_ims[b]] both times).  q, k, v [B, H, T, hd].  query "all": o [B, T, H hd], every row's attention over the valid
    keys (rows past the valid ones included: the kernels' contract for them differs and is stated by each test); "special": o [B, H hd],
    the special token's row only (its index follows special_last).
    bounds=True: (o, tol) with tol [.., H hd] = (2 delta + (log2(T) + 8) U) max_t |v_t| per (query, head, channel): a score is off by at
    most delta = qk_scale GEMM_REL max_t(|q| . |k_t|) + ACT (the product, then the exponential), which moves every weight of the convex
    combination by at most that relative amount in numerator and denominator; its sum passes log2(T) + 8 rounding additions.
    errs = (e_q, e_k, e_v), the absolute errors q, k, v themselves carry (in_proj_ref's tol_q, tol_k, tol_v): delta grows by
    qk_scale max_t(e_q . |k_t| + |q| . e_k_t) and tol by max_t e_v_t."""
    B, H, T, hd = q.shape
    scale = 1.0 / (hd ** 0.5) if qk_scale is None else qk_scale
    mask = torch.arange(T, device=q.device)[None, :] > num_ims.to(q.device)[:, None]
    if query == "special":
        at = special_index(num_ims, special_last).to(q.device)
        q = q[torch.arange(B, device=q.device), :, at][:, :, None]                 # [B, H, 1, hd]
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, q.shape[2], H * hd)
    o = o[:, 0] if query == "special" else o
    if not bounds:
        return o
    smax = ((q.abs() @ k.abs().transpose(-1, -2)) * scale).masked_fill(mask[:, None, None, :], 0.0).amax(dim=-1)       # [B, H, Q]
    vmax = v.abs().masked_fill(mask[:, None, :, None], 0.0).amax(dim=2)                                             # [B, H, hd]
    rel = 2 * (GEMM_REL * smax + ACT) + (math.log2(T) + 8) * U
    tol = rel[..., None] * vmax[:, :, None, :]                                                                        # [B, H, Q, hd]
    if errs is not None:
        eq, ek, ev = errs
        if query == "special":
            eq = eq[torch.arange(B, device=q.device), :, at][:, :, None]
        ds = ((eq @ k.abs().transpose(-1, -2) + q.abs() @ ek.transpose(-1, -2)) * scale).masked_fill(mask[:, None, None, :], 0.0).amax(dim=-1)
        tol = tol + 2 * ds[..., None] * vmax[:, :, None, :] + ev.masked_fill(mask[:, None, :, None], 0.0).amax(dim=2)[:, :, None, :]
    tol = tol.transpose(1, 2).reshape(B, q.shape[2], H * hd)
    return o, (tol[:, 0] if query == "special" else tol)


def decoder_post_ref(lay: dict, x, attn, bounds: bool = False, e_attn=0.0):
    """x_out = norm3(x' + ffn(x')), x' = norm2(norm1(x + out_proj(attn)) + cab) over the last axis of x / attn [..., d].
    bounds=True: (x_out, tol), every stage's bound the next one's input error (_lin, _ln; an addition rounds once at its result);
    e_attn: the absolute error attn itself carries (0.0: an input, exact)."""
    eps = lay["eps"]
    y0, t0, _ = _lin(attn, e_attn, lay["wo"], lay["bo"])
    v1 = x + y0
    x1, t1 = _ln(v1, t0 + U * v1.abs(), lay["ln1g"], lay["ln1b"], eps)
    v2 = x1 + lay["cab"]
    x2, t2 = _ln(v2, t1 + U * v2.abs(), lay["ln2g"], lay["ln2b"], eps)
    h, th, _ = _lin(x2, t2, lay["w1"], lay["b1"], 1)
    f, tf, _ = _lin(h, th, lay["w2"], lay["b2"])
    v3 = x2 + f
    x3, t3 = _ln(v3, t2 + tf + U * v3.abs(), lay["ln3g"], lay["ln3b"], eps)
    return (x3, t3) if bounds else x3


def decoder_layer_ref(lay: dict, x, num_ims, H: int, attn=None, special_last: bool = False, query: str = "all"):
    """One decoder layer on x [B, T, d]: in_proj, masked softmax attention (attention_ref), out_proj, norm1, + cab, norm2, FFN, norm3.
    attn given ([B, T, d]): it stands in for the attention's output (the layer kernels take it as an input).  query "special": the
    layer at the special token's row only (what the last layer is read at).  Returns q, k, v (+ their tol_ / S_), attn, x_out, tol_x_out
    (the chain's bound for the attn it was given: exact when attn was passed in)."""
    B, T, d = x.shape
    res = in_proj_ref(lay, x, H)
    if attn is None:
        attn = attention_ref(res["q"], res["k"], res["v"], num_ims, special_last, query)
    xin = x
    if query == "special":
        xin = x[torch.arange(B, device=x.device), special_index(num_ims, special_last).to(x.device)]
    res["attn"] = attn
    res["x_out"], res["tol_x_out"] = decoder_post_ref(lay, xin, attn, bounds=True)
    return res


def token0_tail_ref(lay: dict, lvl: dict, x, num_ims, H: int, ctx_prev=None, ctx_all=None, special_last: bool = False, qkv=None,
                    qk_scale=None):
    """The LAST layer at one query per slide (the special token's), decoder.norm (lvl lnfg, lnfb, lnf_eps), the slide context (ctx_prev
    [B, d] added, or ctx_all [B, depth, d] concatenated in front) and the classifier (lvl wcls, bcls): reference model/aggregator.py:70-75,
    model/paths.py:130-139.  qkv = (q, k, v) [B, H, T, hd] stands in for the layer's in_proj (paths_token0_tail takes them as inputs;
    qk_scale as in attention_ref for a pre-scaled q).  Returns ctx_out [B, d], logits, tol_ctx, tol_logits (final_head_ref's bounds on top of the chain's)."""
    B, T, d = x.shape
    at = special_index(num_ims, special_last).to(x.device)
    if qkv is None:
        r = in_proj_ref(lay, x, H)
        qkv = (r["q"], r["k"], r["v"])
    a, ta = attention_ref(*qkv, num_ims, special_last, "special", qk_scale, bounds=True)
    x3, t3 = decoder_post_ref(lay, x[torch.arange(B, device=x.device), at], a, bounds=True, e_attn=ta)
    f, tf = _ln(x3, t3, lvl["lnfg"], lvl["lnfb"], lvl["lnf_eps"], (d + 63) // 64 + 6)
    if ctx_prev is not None:
        f = f + ctx_prev
        tf = tf + U * f.abs()
    inp = f if ctx_all is None else torch.cat([ctx_all.reshape(B, -1), f], dim=1)
    logits = inp @ lvl["wcls"].T + lvl["bcls"]
    steps = (inp.shape[1] + 63) // 64 + 8
    tl = tf @ lvl["wcls"][:, -d:].abs().T + steps * U / 2 * (inp.abs() @ lvl["wcls"].abs().T) + U * logits.abs()
    return f, logits, tf, tl


def fused_token_order(tokens, num_ims):
    """imp_proj_ref's tokens [B, N + 1, d] (special first, patch i at row i + 1) in the fused finish's order: patch i at row i and
    `special` at row num_ims[b]; a row j behind it is padding and holds the token of the (padded) patch min(j, N - 1), the slot's own
    patch row as the fused finish reads it.  Returns (tokens in that order, perm [B, N + 1] with out[b, j] = tokens[b, perm[b, j]])."""
    B, T = tokens.shape[:2]
    j = torch.arange(T, device=tokens.device)[None, :].expand(B, T)
    n = num_ims.to(tokens.device).long()[:, None]
    perm = torch.where(j < n, j + 1, torch.where(j == n, torch.zeros_like(j), (j + 1).clamp(max=T - 1)))
    return torch.gather(tokens, 1, perm[:, :, None].expand_as(tokens)), perm


# normalisation stages on each output's path (the second condition's n): the chain's three LayerNorms, decoder.norm on top for the tail
LAYER_ACTIVATIONS = {"x_out": 3, "q": 3, "k": 3, "v": 3, "q_only": 0, "k_only": 0, "v_only": 0}
TAIL_ACTIVATIONS = {"ctx_out": 4, "logits": 4}
ATTN_ACTIVATIONS = {"o": 1}          # the softmax's exponential
