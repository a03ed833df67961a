"""The float64 attention reference (tests/attn_ref.py) on its own: every GPU assertion of tests/test_gpu_attention_backward.py rests
on it, so it is checked here against the hand-written gradients of softmax attention (no GPU needed)."""
import math

import pytest
import torch

from tests.attn_ref import LN2, attn_ref_fwd_bwd


def closed_form(q, k, v, n, c, d_o, mask=None, max_queries=0):
    """One slide, all heads, by the textbook formulas: P = softmax(c q k^T), Pm = P m, O = Pm V, G = dO on the rows that carry a
    gradient, dV = Pm^T G, dP = (G V^T) m, D = rowsum(G O), dS = P (dP - D), dQ = c dS K, dK = c dS^T Q."""
    q, k, v, d_o = (x[:, :n].double() for x in (q, k, v, d_o))
    m = mask[:, :n, :n].double() if mask is not None else torch.ones(q.shape[0], n, n, dtype=torch.float64)
    s = c * q @ k.transpose(1, 2)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)
    o = (p * m) @ v
    g = d_o.clone()
    if max_queries > 0:
        g[:, max_queries:] = 0
    dv = (p * m).transpose(1, 2) @ g
    dp = (g @ v.transpose(1, 2)) * m
    D = (g * o).sum(-1, keepdim=True)
    ds = p * (dp - D)
    lse2 = torch.log2(torch.exp2(s / LN2).sum(-1))
    return {"o": o, "lse": lse2, "dq": c * ds @ k, "dk": c * ds.transpose(1, 2) @ q, "dv": dv}


def inputs(B, H, T, hd, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, d_o = (torch.randn(B, H, T, hd, generator=g, dtype=torch.float64) for _ in range(4))
    q[:, 1] *= 4                                     # a sharp head
    k[:, 2] = k[:, 2, :1] + 0.01 * k[:, 2]           # a near-uniform head
    return q, k, v, d_o


def assert_matches_closed_form(ref, q, k, v, lens, c, d_o, mask=None, max_queries=0):
    for b, n in enumerate(lens):
        want = closed_form(q[b], k[b], v[b], n, c, d_o[b], None if mask is None else mask[b], max_queries)
        for name, w in want.items():
            if max_queries > 0 and name in ("o", "lse"):       # rows >= max_queries of the forward are not evaluated
                w = w[:, :max_queries]
            got = ref[name][b][:, :w.shape[1]]
            assert torch.allclose(got, w, rtol=1e-11, atol=1e-12 * float(w.abs().max() + 1)), (b, name)
            assert not ref[name][b][:, n:].any(), (b, name)                                 # rows >= len stay zero


def test_reference_matches_the_closed_form_on_ragged_slides():
    B, H, T, hd = 4, 3, 13, 8
    lens = [13, 7, 1, 2]
    q, k, v, d_o = inputs(B, H, T, hd, 0)
    c = 0.37
    ref = attn_ref_fwd_bwd(q, k, v, lens, c, d_o)
    assert_matches_closed_form(ref, q, k, v, lens, c, d_o)
    assert ref["dq"].dtype == torch.float64 and float(ref["dq"][0].abs().max()) > 0.1
    # a single key: P = 1 exactly, so dq and dk vanish and dv = dO
    assert float(ref["dq"][2, :, :1].abs().max()) == 0.0 and float(ref["dk"][2, :, :1].abs().max()) == 0.0
    assert torch.equal(ref["dv"][2, :, :1], d_o[2, :, :1].double())
    # what lies beyond a slide's end (the kernels see finite non-zero rows there) does not enter
    q2, k2, v2, g2 = (x.clone() for x in (q, k, v, d_o))
    for x in (q2, k2, v2, g2):
        x[1, :, 7:] = 1e3
    ref2 = attn_ref_fwd_bwd(q2, k2, v2, lens, c, g2)
    for name in ref:
        assert torch.equal(ref[name], ref2[name]), name


def test_reference_with_a_dropout_mask():
    B, H, T, hd = 3, 3, 11, 8
    lens = [11, 6, 1]
    q, k, v, d_o = inputs(B, H, T, hd, 1)
    g = torch.Generator().manual_seed(7)
    sc = 1.0 / (1.0 - round(0.3 * 65536) / 65536.0)
    mask = (torch.rand(B, H, T, T, generator=g) >= 0.3).double() * sc
    c = LN2
    ref = attn_ref_fwd_bwd(q, k, v, lens, c, d_o, drop_mask=mask)
    assert_matches_closed_form(ref, q, k, v, lens, c, d_o, mask=mask)
    plain = attn_ref_fwd_bwd(q, k, v, lens, c, d_o)
    assert torch.equal(ref["lse"], plain["lse"])                           # lse is the softmax before dropout
    for name in ("o", "dq", "dk", "dv"):
        assert float((ref[name] - plain[name]).abs().max()) > 1e-2, name  # the mask is applied


def test_reference_with_max_queries_one():
    B, H, T, hd = 3, 3, 9, 8
    lens = [9, 4, 1]
    q, k, v, d_o = inputs(B, H, T, hd, 2)
    c = 0.5
    ref = attn_ref_fwd_bwd(q, k, v, lens, c, d_o, max_queries=1)
    assert_matches_closed_form(ref, q, k, v, lens, c, d_o, max_queries=1)
    assert float(ref["dq"][:, :, 1:].abs().max()) == 0.0                   # only query 0 carries an output gradient
    g0 = d_o.clone()
    g0[:, :, 1:] = 0
    full = attn_ref_fwd_bwd(q, k, v, lens, c, g0)
    for name in ("dq", "dk", "dv"):
        assert torch.allclose(ref[name], full[name], rtol=0, atol=1e-13), name
    for name in ("o", "lse"):                                               # the forward of query 0 only
        assert torch.allclose(ref[name][:, :, :1], full[name][:, :, :1], rtol=1e-14, atol=0), name
        assert not ref[name][:, :, 1:].any(), name
    # a mask given for the evaluated query rows only
    sc = 1.0 / (1.0 - round(0.5 * 65536) / 65536.0)
    mask = (torch.rand(B, H, 1, T, generator=torch.Generator().manual_seed(3)) >= 0.5).double() * sc
    mref = attn_ref_fwd_bwd(q, k, v, lens, c, d_o, drop_mask=mask, max_queries=1)
    full_mask = torch.ones(B, H, T, T, dtype=torch.float64)
    full_mask[:, :, :1] = mask
    assert_matches_closed_form(mref, q, k, v, lens, c, d_o, mask=full_mask, max_queries=1)


def test_reference_with_a_zero_padded_head():
    """True head_dim 40 carried in 48 columns (ops.padded_head_dim): the padded q / k / v columns are zero and the scale comes from
    40; gradients equal those of the unpadded attention, zero in the padded columns."""
    B, H, T, hd, hp = 2, 3, 10, 40, 48
    lens = [10, 3]
    q, k, v, d_o = inputs(B, H, T, hd, 3)
    pad = lambda x: torch.cat((x, torch.zeros(B, H, T, hp - hd, dtype=x.dtype)), dim=-1)  # noqa: E731
    gp = pad(d_o)
    gp[..., hd:] = 0.5                                     # whatever dO holds there: dv of a zero v column still sees it
    qscale = math.log2(math.e) / math.sqrt(hd)
    ref = attn_ref_fwd_bwd(q, k, v, lens, qscale * LN2, d_o)
    refp = attn_ref_fwd_bwd(pad(q), pad(k), pad(v), lens, qscale * LN2, gp)
    for name in ("o", "dq", "dk", "dv"):
        assert torch.allclose(refp[name][..., :hd], ref[name], rtol=1e-12, atol=1e-13), name
    for name in ("o", "dq", "dk"):
        assert float(refp[name][..., hd:].abs().max()) == 0.0, name
    assert torch.allclose(refp["lse"], ref["lse"], rtol=1e-13, atol=0)
    # the scale is that of the true width: 1 / sqrt(40) in natural units, not 1 / sqrt(48)
    s = (q[0, :, :10].double() @ k[0, :, :10].double().transpose(1, 2)) / math.sqrt(hd)
    assert torch.allclose(refp["lse"][0, :, :10], torch.logsumexp(s, -1) / LN2, rtol=1e-13, atol=0)


def test_head_major_and_token_major_conventions_agree():
    """A pre-scaled q with score_mul = ln 2 (x6 / f32 / token0) and the unscaled q with score_mul = qscale ln 2 (any / wide) are the
    same attention; the gradients of the two q's differ by the factor qscale."""
    B, H, T, hd = 2, 3, 8, 16
    lens = [8, 5]
    q, k, v, d_o = inputs(B, H, T, hd, 4)
    qscale = math.log2(math.e) / math.sqrt(hd)
    tok = attn_ref_fwd_bwd(q, k, v, lens, qscale * LN2, d_o)
    head = attn_ref_fwd_bwd(q * qscale, k, v, lens, LN2, d_o)
    for name in ("o", "lse", "dk", "dv"):
        assert torch.allclose(tok[name], head[name], rtol=1e-12, atol=1e-13), name
    assert torch.allclose(tok["dq"], head["dq"] * qscale, rtol=1e-12, atol=1e-13)
    # and both are the scaled dot-product attention of torch
    sdpa = torch.nn.functional.scaled_dot_product_attention(q[0].double(), k[0].double(), v[0].double())
    assert torch.allclose(tok["o"][0], sdpa, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("max_queries", [0, 1])
def test_reference_follows_the_input_device_and_keeps_fp32_inputs_exact(max_queries):
    B, H, T, hd = 2, 3, 6, 8
    q, k, v, d_o = (x.float() for x in inputs(B, H, T, hd, 5))
    ref = attn_ref_fwd_bwd(q, k, v, [6, 2], LN2, d_o, max_queries=max_queries)
    ref64 = attn_ref_fwd_bwd(q.double(), k.double(), v.double(), [6, 2], LN2, d_o.double(), max_queries=max_queries)
    for name in ref:
        assert ref[name].device == q.device and ref[name].dtype == torch.float64
        assert torch.equal(ref[name], ref64[name]), name
