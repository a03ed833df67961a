"""Float64 restatement of the special token's gradient-weighted attention relevance (Chefer, Gur & Wolf 2021) as the project
defines it, with explicit T_b x T_b matrices.

Per slide with T_b = num_ims + 1 valid tokens (row 0 = special token s), A_l^h layer l's softmax attention of head h over the valid
keys and gradA_l^h = d target / d A_l^h (entry (i, j) = dO_i^h . V_j^h):

    Abar_l = mean_h (A_l^h * gradA_l^h)^+          r = e_s^T (I + Abar_{L-1}) ... (I + Abar_0)

A slide without patches (num_ims = 0) keeps r = e_s.  ``absval`` puts |.| in place of (.)^+: the envelope that scales the end-to-end
tolerance.  The HIP kernels (csrc/attn_relevance.hip) never materialise these matrices."""
import math

import torch

LN2 = math.log(2.0)


def valid_last(num_ims, b: int, T: int) -> int:
    return int(min(max(int(num_ims[b]), 0), T - 1))


def _rect(x: torch.Tensor, absval: bool) -> torch.Tensor:
    return x.abs() if absval else x.clamp_min(0.0)


def lse64(q, k, num_ims, qscale: float) -> torch.Tensor:
    """[B, H, T] float64: log2-domain log-sum-exp of qscale * q_i . k_j over the valid keys (NaN on padded query rows: never read).
    q, k [B, H, T, hd]."""
    q, k = torch.as_tensor(q).double(), torch.as_tensor(k).double()
    B, H, T, _ = q.shape
    out = torch.full((B, H, T), float("nan"), dtype=torch.float64)
    for b in range(B):
        n1 = valid_last(num_ims, b, T) + 1
        s = qscale * (q[b, :, :n1] @ k[b, :, :n1].transpose(-1, -2))
        out[b, :, :n1] = torch.logsumexp(s * LN2, dim=-1) / LN2
    return out


def seed64(q, k, v, da0, num_ims, qscale: float, absval: bool = False) -> torch.Tensor:
    """r [B, T] float64 of the last layer, read at token 0: e_s + mean_h (a0^h * (da0^h . V_j^h))^+ with its own softmax.
    q, k, v [B, H, T, hd]; da0 [B, H*hd]; scores qscale * q . k in the log2 domain."""
    q, k, v = (torch.as_tensor(t).double() for t in (q, k, v))
    B, H, T, hd = q.shape
    da0 = torch.as_tensor(da0).double().reshape(B, H, hd)
    r = torch.zeros((B, T), dtype=torch.float64)
    for b in range(B):
        n1 = valid_last(num_ims, b, T) + 1
        r[b, 0] = 1.0
        if n1 == 1:
            continue
        a0 = torch.softmax(LN2 * qscale * torch.einsum("he,hje->hj", q[b, :, 0], k[b, :, :n1]), dim=-1)
        g0 = torch.einsum("he,hje->hj", da0[b], v[b, :, :n1])
        r[b, :n1] += _rect(a0 * g0, absval).mean(0)
    return r


def step64(q, k, v, d_o, num_ims, qscale: float, r_in, absval: bool = False) -> torch.Tensor:
    """r_out [B, T] float64 = r_in + r_in^T mean_h (A^h * (dO^h V^h^T))^+ through one full layer with its own softmax.
    q, k, v [B, H, T, hd]; d_o [B, T, >= H*hd] with head h at columns [h*hd, (h+1)*hd); r_in [B, T] (rows past num_ims ignored)."""
    q, k, v = (torch.as_tensor(t).double() for t in (q, k, v))
    B, H, T, hd = q.shape
    d_o = torch.as_tensor(d_o).double()[:, :, :H * hd].reshape(B, T, H, hd).permute(0, 2, 1, 3)
    r_in = torch.as_tensor(r_in).double()
    out = torch.zeros((B, T), dtype=torch.float64)
    for b in range(B):
        n1 = valid_last(num_ims, b, T) + 1
        out[b, :n1] = r_in[b, :n1]
        if n1 == 1:
            continue
        a = torch.softmax(LN2 * qscale * (q[b, :, :n1] @ k[b, :, :n1].transpose(-1, -2)), dim=-1)
        g = d_o[b, :, :n1] @ v[b, :, :n1].transpose(-1, -2)
        out[b, :n1] += r_in[b, :n1] @ _rect(a * g, absval).mean(0)
    return out


def relevance_from_attention(att: list, grad: list, num_ims, T: int, absval: bool = False):
    """att[l] / grad[l]: [B, H, T, T] attention and its gradient of layer l (grad None: no path to the target) ->
    (relevance [B, T-1], relevance_self [B]) float64: R <- R + Abar R from R = I, layers 0 .. L-1, read at row 0."""
    B = att[0].shape[0]
    rel = torch.zeros((B, T - 1), dtype=torch.float64)
    self_ = torch.ones((B,), dtype=torch.float64)
    if any(g is None for g in grad):
        return rel, self_
    for b in range(B):
        n1 = valid_last(num_ims, b, T) + 1
        if n1 == 1:
            continue
        R = torch.eye(n1, dtype=torch.float64)
        for a, g in zip(att, grad):
            abar = _rect(a[b, :, :n1, :n1].double() * g[b, :, :n1, :n1].double(), absval).mean(0)
            R = R + abar @ R
        rel[b, :n1 - 1] = R[0, 1:]
        self_[b] = R[0, 0]
    return rel, self_


def _stack64(p, prefix: str, S: torch.Tensor, num_ims, nhead: int, layers: int, eps: float):
    """The post-LN decoder stack + final norm (the oracle's empty-memory form) in float64 on S [B, T, d]; every layer's attention
    probabilities [B, H, T, T] keep their gradient (retain_grad).  Returns (token 0 of the output [B, d], the probabilities)."""
    B, T, d = S.shape
    S = S.detach().clone().requires_grad_()        # (the token rows are the graph's leaves: every probability below is an interior node)
    g = lambda name: torch.as_tensor(p[prefix + name]).double()
    ln = lambda x, w, bb: torch.nn.functional.layer_norm(x, (d,), w, bb, eps)
    hd = d // nhead
    key_pad = torch.arange(T)[None, :] >= (torch.as_tensor(num_ims) + 1)[:, None]
    probs = []
    for l in range(layers):
        q_ = f"layers.{l}."
        qkv = S @ g(q_ + "self_attn.in_proj_weight").T + g(q_ + "self_attn.in_proj_bias")
        q, k, v = (t.reshape(B, T, nhead, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        sc = ((q @ k.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(key_pad[:, None, None, :], float("-inf"))
        a = torch.softmax(sc, dim=-1)
        a.retain_grad()
        probs.append(a)
        o = (a @ v).transpose(1, 2).reshape(B, T, d) @ g(q_ + "self_attn.out_proj.weight").T
        S = ln(S + o + g(q_ + "self_attn.out_proj.bias"), g(q_ + "norm1.weight"), g(q_ + "norm1.bias"))
        S = ln(S + g(q_ + "multihead_attn.out_proj.bias"), g(q_ + "norm2.weight"), g(q_ + "norm2.bias"))
        ff = torch.relu(S @ g(q_ + "linear1.weight").T + g(q_ + "linear1.bias")) @ g(q_ + "linear2.weight").T + g(q_ + "linear2.bias")
        S = ln(S + ff, g(q_ + "norm3.weight"), g(q_ + "norm3.bias"))
    return ln(S, g("norm.weight"), g("norm.bias"))[:, 0], probs


def decoder_relevance64(params, levels: list, nhead: int, layers: int, slide_ctx_mode: str, target, eps: float = 1e-5):
    """Every level's relevance from the oracle's own token rows.  ``levels[depth]`` = (xs [B, N, d] - orc.process_level's probe["xs"] -,
    num_ims [B]); ``target``: logits [B, C] -> [B].  Each level's stack runs in float64 on its token rows (special token first), the
    levels' outputs are chained through the slide context (reference model/paths.py:130-137: residual / concat / none) to the last
    level's logits and the target, and ONE backward() gives every level's gradA.  Returns per level
    ((relevance, relevance_self), (envelope, envelope_self)), the envelope with |.| in place of (.)^+."""
    with torch.enable_grad():
        ctx, probs, logits = [], [], None
        for depth, (xs, num_ims) in enumerate(levels):
            pre = f"procs.{depth}."
            xs = torch.as_tensor(xs).double()
            special = torch.as_tensor(params[pre + "global_agg.special_token"]).double().view(1, 1, -1).repeat(xs.shape[0], 1, 1)
            agg, pr = _stack64(params, pre + "global_agg.transformer.decoder.", torch.cat((special, xs), dim=1), num_ims, nhead, layers, eps)
            probs.append(pr)
            if slide_ctx_mode == "residual" and ctx:
                agg = agg + ctx[-1]
            ft = torch.cat(ctx + [agg], dim=1) if slide_ctx_mode == "concat" else agg
            logits = ft @ torch.as_tensor(params[pre + "classification_layer.weight"]).double().T \
                + torch.as_tensor(params[pre + "classification_layer.bias"]).double()
            ctx.append(agg)
        target(logits).sum().backward()
    out = []
    for (xs, num_ims), pr in zip(levels, probs):
        att, grad = [a.detach() for a in pr], [a.grad for a in pr]
        T = xs.shape[1] + 1
        out.append((relevance_from_attention(att, grad, num_ims, T), relevance_from_attention(att, grad, num_ims, T, absval=True)))
    return out
