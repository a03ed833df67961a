"""Float64 restatement of the special token's attention rollout (Abnar & Zuidema 2020) as the project defines it.

Per slide with T = num_ims + 1 valid tokens and A_l^h layer l's softmax attention of head h over the valid keys (valid query rows only,
T x T): Â_l = 0.5 mean_h(A_l^h) + 0.5 I and r = e_s^T Â_{L-1} ... Â_0.  ``rollout`` [B, T-1] is r at the patches (0 on padding),
``rollout_self`` [B] r at the special token.  The full matrices are formed explicitly here; the HIP kernels never materialise them."""
import math

import torch


def canonical_rows(x: torch.Tensor, num_ims, special_last: int) -> torch.Tensor:
    """Rows of x [B, T, d] in the reference's order (special token first, then the patches); rows past num_ims[b] keep their place."""
    if not special_last:
        return x
    out = x.clone()
    for b in range(x.shape[0]):
        n = int(min(max(int(num_ims[b]), 0), x.shape[1] - 1))
        out[b, 0] = x[b, n]
        out[b, 1:n + 1] = x[b, :n]
    return out


def layer_attention64(x, num_ims, w_in, b_in, nhead) -> list:
    """Per slide, the [H, T_b, T_b] softmax attention of one layer over its valid rows (special token first), from the layer's input
    rows x [B, T, d] and its in_proj (bias included) in float64."""
    x = torch.as_tensor(x).double()
    w_in, b_in = torch.as_tensor(w_in).double(), torch.as_tensor(b_in).double()
    B, T, d = x.shape
    hd = d // nhead
    out = []
    for b in range(B):
        n = int(min(max(int(num_ims[b]), 0), T - 1))
        rows = x[b, : n + 1]
        q = rows @ w_in[:d].T + b_in[:d]
        k = rows @ w_in[d:2 * d].T + b_in[d:2 * d]
        q, k = (t.reshape(n + 1, nhead, hd).transpose(0, 1) for t in (q, k))
        out.append(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1))
    return out


def rollout_from_attention(per_layer: list, T: int):
    """per_layer[l][b]: [H, T_b, T_b] (or [T_b, T_b], already averaged over heads) -> (rollout [B, T-1], rollout_self [B]) float64."""
    B = len(per_layer[0])
    roll = torch.zeros((B, T - 1), dtype=torch.float64)
    self_ = torch.zeros((B,), dtype=torch.float64)
    for b in range(B):
        n1 = per_layer[0][b].shape[-1]
        r = torch.zeros((n1,), dtype=torch.float64)
        r[0] = 1.0
        for l in range(len(per_layer) - 1, -1, -1):
            a = per_layer[l][b].double()
            a = a.mean(0) if a.dim() == 3 else a
            r = r @ (0.5 * a + 0.5 * torch.eye(n1, dtype=torch.float64))
        roll[b, : n1 - 1] = r[1:]
        self_[b] = r[0]
    return roll, self_


def step64(x, num_ims, w_in, b_in, nhead, special_last: int, r_in) -> torch.Tensor:
    """One rollout step through a layer: r_out = 0.5 r_in + 0.5 mean_h(r_in^T A^h), r in canonical order [B, T] (0 past num_ims)."""
    x = canonical_rows(torch.as_tensor(x), num_ims, special_last)
    att = layer_attention64(x, num_ims, w_in, b_in, nhead)
    r_in = torch.as_tensor(r_in).double()
    out = torch.zeros_like(r_in)
    for b, a in enumerate(att):
        n1 = a.shape[-1]
        out[b, :n1] = 0.5 * r_in[b, :n1] + 0.5 * (r_in[b, :n1] @ a.mean(0))
    return out


def decoder_rollout64(p, prefix: str, S, num_ims, nhead: int, layers: int, eps: float = 1e-5):
    """The post-LN decoder stack (layer keys ``prefix + "layers.{l}."``, the oracle's empty-memory form: cross-attention adds its
    out_proj bias) in float64 on S [B, T, d] (special token first): (rollout [B, T-1], rollout_self [B])."""
    S = torch.as_tensor(S).double()
    B, T, d = S.shape
    g = lambda name: torch.as_tensor(p[prefix + name]).double()
    ln = lambda v, w, bb: torch.nn.functional.layer_norm(v, (d,), w, bb, eps)
    hd = d // nhead
    key_pad = torch.arange(T)[None, :] >= (torch.as_tensor(num_ims) + 1)[:, None]
    per_layer = []
    for l in range(layers):
        q_ = f"layers.{l}."
        w_in, b_in = g(q_ + "self_attn.in_proj_weight"), g(q_ + "self_attn.in_proj_bias")
        per_layer.append(layer_attention64(S, num_ims, w_in, b_in, nhead))
        qkv = S @ w_in.T + b_in
        q, k, v = (t.reshape(B, T, nhead, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        sc = ((q @ k.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(key_pad[:, None, None, :], float("-inf"))
        o = (torch.softmax(sc, dim=-1) @ v).transpose(1, 2).reshape(B, T, d) @ g(q_ + "self_attn.out_proj.weight").T
        S = ln(S + o + g(q_ + "self_attn.out_proj.bias"), g(q_ + "norm1.weight"), g(q_ + "norm1.bias"))
        S = ln(S + g(q_ + "multihead_attn.out_proj.bias"), g(q_ + "norm2.weight"), g(q_ + "norm2.bias"))
        ff = torch.relu(S @ g(q_ + "linear1.weight").T + g(q_ + "linear1.bias")) @ g(q_ + "linear2.weight").T + g(q_ + "linear2.bias")
        S = ln(S + ff, g(q_ + "norm3.weight"), g(q_ + "norm3.bias"))
    return rollout_from_attention(per_layer, T)


def oracle_level_rollout(params, depth: int, xs, num_ims, nhead: int, layers: int):
    """The rollout of one level of the oracle: ``xs`` [B, N, dim] = the aggregator's input rows (orc.process_level's probe["xs"])."""
    pre = f"procs.{depth}.global_agg."
    B = xs.shape[0]
    S = torch.cat((torch.as_tensor(params[pre + "special_token"]).view(1, 1, -1).repeat(B, 1, 1), torch.as_tensor(xs)), dim=1)
    return decoder_rollout64(params, pre + "transformer.decoder.", S, num_ims, nhead, layers)
