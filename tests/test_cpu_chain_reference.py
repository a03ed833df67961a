"""tests/chain_ref.py (the float64 references of the forward LSTM cell and importance / projection kernels) against the oracle, and
the packed layouts it assumes against ops.pack_lstm / ops.pack_level.  No GPU."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import paths_oracle as orc
from tests import chain_ref as R
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _lstm_weights(D, Hc, seed):
    g = torch.Generator().manual_seed(seed)
    w = {}
    for name in R.GATES:
        rows, cols = (D if name in ("out_select_gate", "mem_to_out") else Hc), (Hc if name == "mem_to_out" else 2 * D)
        w[name + ".weight"] = ((torch.rand((rows, cols), generator=g, dtype=F64) * 2 - 1) / math.sqrt(cols))
        w[name + ".bias"] = torch.rand((rows,), generator=g, dtype=F64) - 0.5
    return w, g


def _oracle_lstm_params(w):
    return {f"lstm.{k.replace('.', '.0.')}": v for k, v in w.items()}


@pytest.fixture(scope="module")
def model():
    from paths_amd.config import Config
    cfg = Config.load(os.path.join(ROOT, "tests", "golden", "sample"), test_mode=True)
    torch.manual_seed(3)
    return cfg.get_model()


@pytest.mark.parametrize("form", ["none", "h0c0", "hp"])
def test_lstm_ref_equals_the_oracle_in_float64(form):
    """All three previous-state forms.  For hp the table is built in float64 from h_parent and the packed w_gates[:, D:2D]: the
    reference must read the packed column order (f|r|m per 32 units, then o) for the result to agree."""
    D, Hc, M, P = 64, 64, 37, 9
    w, g = _lstm_weights(D, Hc, 11)
    x = torch.rand((M, D), generator=g, dtype=F64) * 3 - 1.5
    c0 = torch.rand((M, Hc), generator=g, dtype=F64) * 4 - 2
    if form == "none":
        prev, hs, cs = None, torch.zeros((M, D), dtype=F64), torch.zeros((M, Hc), dtype=F64)
    elif form == "h0c0":
        hs, cs = torch.rand((M, D), generator=g, dtype=F64) * 2 - 1, c0
        prev = {"h0": hs, "c0": c0}
    else:
        hpar = torch.rand((P, D), generator=g, dtype=F64) * 2 - 1
        row = torch.randint(0, P, (M,), generator=g)
        row[::5] = -1
        wg, _ = R.pack_gates(w)
        prev = {"hp": hpar @ wg[:, D:].T, "hp_row": row.to(torch.int32), "c0": c0}
        hs, cs = hpar[row.clamp(min=0)] * (row >= 0)[:, None], c0
    got = R.lstm_ref(w, x, prev, bounds=True)
    h1, c1 = orc.lstm_cell(_oracle_lstm_params(w), x, hs, cs)
    torch.testing.assert_close(got["h1"], h1, rtol=0, atol=1e-13)
    torch.testing.assert_close(got["c1"], c1, rtol=0, atol=1e-13)
    torch.testing.assert_close(got["y"], x + h1, rtol=0, atol=1e-13)
    for k in ("f", "r", "m", "c1", "o", "tc", "h1", "y"):
        t = got["tol_" + k]
        assert t.shape == got[k].shape and bool((t > 0).all()) and float(t.max()) < 1e-3, k


def test_pack_gates_is_ops_pack_lstm(model):
    from paths_amd import ops
    pk = ops.pack_lstm(model.lstm)
    w = {f"{n}.{k}": getattr(model.lstm, n)[0].__getattr__(k).detach() for n in R.GATES for k in ("weight", "bias")}
    wg, bg = R.pack_gates(w)
    assert torch.equal(pk["w_gates"], wg) and torch.equal(pk["b_gates"], bg)
    assert torch.equal(pk["w_mem"], w["mem_to_out.weight"]) and torch.equal(pk["b_mem"], w["mem_to_out.bias"])
    Hc, D = pk["Hc"], w["out_select_gate.weight"].shape[0]
    cf, cr, cm, co = R.packed_gate_columns(Hc, D)
    assert sorted(torch.cat([cf, cr, cm, co]).tolist()) == list(range(3 * Hc + D))       # a permutation
    assert torch.equal(wg[cm[33]], w["remember_map.weight"][33]) and int(cm[33]) == 96 + 64 + 1
    packed = R.packed_frm({"f": torch.full((2, Hc), 1.0), "r": torch.full((2, Hc), 2.0), "m": torch.full((2, Hc), 3.0)})
    assert packed[0, :96].tolist() == [1.0] * 32 + [2.0] * 32 + [3.0] * 32


def test_interleave_is_ops_pack_level(model):
    from paths_amd import ops
    proc = model.procs[0]
    pk = ops.pack_level(proc)
    w1, wp = proc.importance_mlp[0].weight.detach(), proc.global_agg.proj_in.weight.detach()
    assert torch.equal(pk["w_ip_fwd"], R.interleave_ip(w1, wp))
    assert torch.equal(pk["w_ip_fwd"][64:128], wp[:64]) and torch.equal(pk["w_ip_fwd"][128:192], w1[64:])
    d = wp.shape[0]
    k = 10000.0
    assert torch.equal(pk["div_2d"].cpu(), torch.exp(torch.arange(0, d // 2, 2) * (-math.log(k) / d)).float())
    assert torch.equal(pk["div_1d"].cpu(), torch.exp(torch.arange(0, d, 2) * (-math.log(k) / d)).float())


def _divs(d):
    k = 10000.0
    return (torch.exp(torch.arange(0, d, 2) * (-math.log(k) / d)).float(), torch.exp(torch.arange(0, d // 2, 2) * (-math.log(k) / d)).float())


def test_pe_equals_the_oracle():
    """The oracle evaluates position * div_term and sin / cos in fp32; the reference takes the same fp32 angle and evaluates in
    float64: they differ by the fp32 rounding of a value in [-1, 1] (and the fp32 sin's own error)."""
    d = 128
    div1, div2 = _divs(d)
    xs, ys = torch.tensor([0, 1, 7, 63, 1000, 65535, 5592404]), torch.tensor([3, 0, 7, 12, 999, 1, 2])
    want = orc.positional_encoding_2d_from_pos(xs, ys, d)
    got = R.pe_ref(2, d, div2, torch.stack([xs * 3 + 2, ys * 3], dim=1), 3)            # floor((3 x + 2) / 3) = x
    assert float((got - want.double()).abs().max()) <= 3 * 2.0 ** -23
    want1 = orc.positional_encoding(50, d)
    got1 = R.pe_ref(1, d, div1, idx=torch.arange(50))
    assert float((got1 - want1.double()).abs().max()) <= 3 * 2.0 ** -23
    assert torch.equal(R.pe_table_ref(1, d, div1, 50), got1)
    assert torch.equal(R.pe_table_ref(2, d, div2, 9)[7], got[2, :64])
    # the angle is the fp32 product: at a position this large the float64 product's sine is a different number
    big = R.pe_angles(torch.tensor([5592404]), div2, 1)
    assert big.dtype == torch.float32 and float((torch.sin(big.double()) - torch.sin(5592404.0 * div2.double().repeat_interleave(2))).abs().max()) > 1e-3


@pytest.mark.parametrize("imp_mul", [1, 0])
def test_imp_proj_ref_equals_the_oracle_pieces_in_float64(imp_mul):
    """A full slide, a padded one and an empty one (reference model/paths.py:95-98,119-124 as oracle.process_level writes them)."""
    D, d, Hi, B, N, ps = 64, 128, 128, 3, 6, 224
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=F64) * 2 - 1
    p = {"W1": rnd(Hi, D) / 8, "b1": rnd(Hi) / 2, "w2": rnd(Hi) / 11, "b2": rnd(1) / 2, "Wp": rnd(d, D) / 8, "bp": rnd(d) / 2,
         "special": rnd(d), "div_term": _divs(d)[1]}
    Y = rnd(B * N, D) * 1.5
    num_ims = torch.tensor([N, 2, 0])
    locs = torch.randint(0, 40 * ps, (B * N, 2), generator=g)
    got = R.imp_proj_ref(p, Y, locs, num_ims, N, ps, 2, imp_mul, bounds=True)
    valid = (torch.arange(N)[None, :] < num_ims[:, None]).reshape(-1)
    a = F.linear(torch.relu(F.linear(Y[valid], p["W1"], p["b1"])), p["w2"][None], p["b2"])
    imp = torch.zeros(B * N, dtype=F64)
    imp[valid] = torch.sigmoid(a)[:, 0]
    Z = Y * imp[:, None] if imp_mul else Y
    pl = torch.div(locs, ps, rounding_mode="floor")
    t = F.linear(Z, p["Wp"], p["bp"]) + orc.positional_encoding_2d_from_pos(pl[:, 0], pl[:, 1], d).double()
    assert torch.equal(got["valid"], valid)
    torch.testing.assert_close(got["importance"], imp, rtol=0, atol=1e-14)
    assert bool((got["importance"][~valid] == 0).all())
    assert float((got["tokens"][:, 1:].reshape(-1, d) - t).abs().max()) <= 3 * 2.0 ** -23
    assert torch.equal(got["tokens"][:, 0], p["special"].expand(B, d))
    torch.testing.assert_close(got["hid"], torch.relu(F.linear(Y, p["W1"], p["b1"])), rtol=0, atol=1e-14)
    torch.testing.assert_close(got["pproj"], F.linear(Y, p["Wp"]), rtol=0, atol=1e-14)
    for k in ("importance", "tokens", "hid", "pproj"):
        assert got["tol_" + k].shape == got[k].shape and float(got["tol_" + k].max()) < 1e-4
    assert bool((got["tol_importance"][~valid] == 0).all()) and bool((got["tol_tokens"][:, 0] == 0).all())


@pytest.mark.parametrize("pe_mode", [2, 1])
def test_importance_tokens_rows_ref_equals_imp_proj_ref_on_its_products(pe_mode):
    """Given hid = [Y W1^T + b1 | Y Wp^T] and a float64 PE table, the row reference reads imp_proj_ref's importance and tokens (imp_mul 1;
    with imp_mul 0 on valid rows: its padded rows are bp + PE, imp_proj_ref's pproj + bp + PE)."""
    D, d, Hi, B, N, ps = 64, 128, 128, 3, 6, 224
    g = torch.Generator().manual_seed(6)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=F64) * 2 - 1
    p = {"W1": rnd(Hi, D) / 8, "b1": rnd(Hi) / 2, "w2": rnd(Hi) / 11, "b2": rnd(1) / 2, "Wp": rnd(d, D) / 8, "bp": rnd(d) / 2,
         "special": rnd(d), "div_term": _divs(d)[pe_mode - 1]}
    Y = rnd(B * N, D) * 1.5
    num_ims = torch.tensor([N, 2, 0])
    locs = torch.randint(0, 40 * ps, (B * N, 2), generator=g)
    hid = torch.cat([F.linear(Y, p["W1"], p["b1"]), F.linear(Y, p["Wp"])], dim=1)
    table = R.pe_table_ref(pe_mode, d, p["div_term"], 40)
    for imp_mul in (1, 0):
        want = R.imp_proj_ref(p, Y, locs, num_ims, N, ps, pe_mode, imp_mul)
        imp, tok, ti, tt = R.importance_tokens_rows_ref(hid, Hi, p["w2"], p["b2"], num_ims, N, 1, imp_mul, p["bp"], p["special"], table, locs,
                                                        ps, pe_mode)
        torch.testing.assert_close(imp, want["importance"], rtol=0, atol=1e-14)
        keep = torch.cat([torch.ones(B, 1, dtype=torch.bool), want["valid"].view(B, N) | bool(imp_mul)], dim=1)
        assert float(((tok - want["tokens"]).abs() * keep[:, :, None]).max()) < 1e-13
        pad = ~want["valid"]
        torch.testing.assert_close(tok[:, 1:].reshape(-1, d)[pad], (p["bp"] + want["pe"])[pad], rtol=0, atol=1e-14)
        assert ti.shape == imp.shape and tt.shape == tok.shape and bool((ti[pad] == 0).all()) and bool((tt[:, 0] == 0).all())


def test_imp_proj_ref_equals_process_level_in_fp32():
    """The whole oracle level (fp32, shipped geometry) reads the same importance and token sequence."""
    cfg = H.oracle_config()
    p = H.oracle_params(cfg, 7)
    info = {"dseed": 3, "depth": 0, "B": 3, "N": 8, "num_ims": [8, 3, 0]}
    inp = {k: torch.from_numpy(v) for k, v in H.single_level_inputs(info, cfg).items()}
    lstm = cfg.lstm
    cfg.lstm = False                # Y = X: the importance / projection step on its own
    cfg.hierarchical_ctx = False
    probe = {}
    out = orc.process_level(p, cfg, 0, inp["fts"], inp["locs"], inp["num_ims"], inp["ctx_slide"], inp["ctx_patch"], probe)
    cfg.lstm = lstm
    q = {"W1": p["procs.0.importance_mlp.0.weight"], "b1": p["procs.0.importance_mlp.0.bias"],
         "w2": p["procs.0.importance_mlp.2.weight"].view(-1), "b2": p["procs.0.importance_mlp.2.bias"].view(-1),
         "Wp": p["procs.0.global_agg.proj_in.weight"], "bp": p["procs.0.global_agg.proj_in.bias"],
         "special": p["procs.0.global_agg.special_token"].view(-1)}
    q = {k: v.double() for k, v in q.items()}
    q["div_term"] = _divs(cfg.trans_dim)[1]
    got = R.imp_proj_ref(q, inp["fts"].reshape(-1, cfg.patch_embed_dim).double(), inp["locs"].reshape(-1, 2), inp["num_ims"], 8,
                         cfg.patch_size, 2, 1)
    assert float((got["importance"].view(3, 8) - out["importance"].double()).abs().max()) < 1e-6
    assert float((got["tokens"][:, 1:] - probe["xs"].double()).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------
# the decoder-layer references
# ------------------------------------------------------------------------------------------------
def _decoder_problem(d, H, lens, T, depth, seed):
    """Two random layers + head in float64, as chain_ref's layer dicts AND as the oracle's state-dict keys; tokens [B, T, d]."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=F64) * 2 - 1
    layers, p = [], {}
    pre = "agg.transformer"
    for l in range(2):
        lay = {"wqkv": rnd(3 * d, d) * 0.3, "bqkv": rnd(3 * d) * 0.1, "wo": rnd(d, d) * 0.1, "bo": rnd(d) * 0.1, "cab": rnd(d) * 0.1,
               "w1": rnd(4 * d, d) * 0.1, "b1": rnd(4 * d) * 0.1, "w2": rnd(d, 4 * d) * 0.05, "b2": rnd(d) * 0.1, "eps": 1e-5}
        for n in ("ln1", "ln2", "ln3"):
            lay[n + "g"], lay[n + "b"] = 1 + rnd(d) * 0.1, rnd(d) * 0.1
        layers.append(lay)
        q = f"{pre}.decoder.layers.{l}."
        p.update({q + "self_attn.in_proj_weight": lay["wqkv"], q + "self_attn.in_proj_bias": lay["bqkv"], q + "self_attn.out_proj.weight": lay["wo"],
                  q + "self_attn.out_proj.bias": lay["bo"], q + "multihead_attn.out_proj.bias": lay["cab"], q + "linear1.weight": lay["w1"],
                  q + "linear1.bias": lay["b1"], q + "linear2.weight": lay["w2"], q + "linear2.bias": lay["b2"]})
        for i, n in enumerate(("ln1", "ln2", "ln3")):
            p[q + f"norm{i + 1}.weight"], p[q + f"norm{i + 1}.bias"] = lay[n + "g"], lay[n + "b"]
    lvl = {"lnfg": 1 + rnd(d) * 0.1, "lnfb": rnd(d) * 0.1, "lnf_eps": 1e-5, "wcls": rnd(4, (depth + 1) * d) * 0.1, "bcls": rnd(4) * 0.1}
    p[pre + ".decoder.norm.weight"], p[pre + ".decoder.norm.bias"] = lvl["lnfg"], lvl["lnfb"]
    B = len(lens)
    num_ims = torch.tensor([n - 1 for n in lens])
    return layers, lvl, p, pre, rnd(B, T, d), num_ims, rnd(B, d), (rnd(B, depth, d) if depth else None)


DECODER_LENS = (9, [1, 9, 4, 7])            # T = N + 1 = 9: a slide with 0 patches, a full one, two ragged ones


@pytest.mark.parametrize("d,H", [(128, 4), (192, 4), (64, 2)])
def test_decoder_layer_ref_equals_the_oracle_in_float64(d, H):
    """in_proj + attention + out_proj against the oracle's _self_attention, a whole layer against its one-layer decoder_stack (whose
    decoder.norm is applied on top of decoder_layer_ref's rows here), every row of every slide: the oracle computes padded query
    rows over the valid keys like any other, and so does the reference."""
    T, lens = DECODER_LENS
    layers, lvl, p, pre, x, num_ims, _, _ = _decoder_problem(d, H, lens, T, 0, d + H)
    lay = layers[0]
    key_pad = torch.arange(T)[None, :] >= (num_ims + 1)[:, None]
    got = R.decoder_layer_ref(lay, x, num_ims, H)
    sa = orc._self_attention(x, lay["wqkv"], lay["bqkv"], lay["wo"], lay["bo"], H, key_pad)
    torch.testing.assert_close(got["attn"] @ lay["wo"].T + lay["bo"], sa, rtol=0, atol=1e-13)
    want = orc.decoder_stack(p, pre, x, key_pad, H, 1)
    torch.testing.assert_close(F.layer_norm(got["x_out"], (d,), lvl["lnfg"], lvl["lnfb"], 1e-5), want, rtol=0, atol=1e-13)
    # attn given: the chain alone on that input; the special-token query alone: row 0 of the full evaluation
    again = R.decoder_layer_ref(lay, x, num_ims, H, attn=got["attn"])
    assert torch.equal(again["x_out"], got["x_out"])
    one = R.decoder_layer_ref(lay, x, num_ims, H, query="special")
    torch.testing.assert_close(one["x_out"], got["x_out"][:, 0], rtol=0, atol=1e-13)
    for k in ("q", "k", "v"):
        assert got[k].shape == (len(lens), H, T, d // H) and got["tol_" + k].shape == got[k].shape and float(got["tol_" + k].max()) < 1e-4
    # (the chain's bound sums worst cases through three LayerNorms and two products: loose, a few 1e-2 here; the tests' second
    # condition is the one that binds for x_out)
    assert got["tol_x_out"].shape == got["x_out"].shape and bool((got["tol_x_out"] > 0).all()) and float(got["tol_x_out"].max()) < 0.1


@pytest.mark.parametrize("ctx_mode", ["residual", "concat", "none"])
def test_token0_tail_ref_equals_the_oracle_in_float64(ctx_mode):
    """Two layers: decoder_layer_ref, then token0_tail_ref, against the oracle's two-layer decoder_stack at token 0 and the head of
    oracle.process_level (model/paths.py:130-139: residual adds ctx_slide[:, -1], concat puts the flattened ctx_slide in front).
    (The bounds only have to exist here: summed worst cases through four LayerNorms and two products, they are far above any
    error a kernel shows; the kernel tests' second condition is the one that binds behind the feed-forward.)"""
    d, H = 128, 4
    T, lens = DECODER_LENS
    depth = 2 if ctx_mode == "concat" else 0
    layers, lvl, p, pre, x, num_ims, ctx_prev, ctx_all = _decoder_problem(d, H, lens, T, depth, 17)
    key_pad = torch.arange(T)[None, :] >= (num_ims + 1)[:, None]
    agg = orc.decoder_stack(p, pre, x, key_pad, H, 2)[:, 0]
    if ctx_mode == "residual":
        agg = agg + ctx_prev
    ft = torch.cat((torch.flatten(ctx_all, start_dim=1), agg), dim=1) if ctx_mode == "concat" else agg
    logits = F.linear(ft, lvl["wcls"], lvl["bcls"])
    x1 = R.decoder_layer_ref(layers[0], x, num_ims, H)["x_out"]
    ctx, lg, tc, tl = R.token0_tail_ref(layers[1], lvl, x1, num_ims, H, ctx_prev if ctx_mode == "residual" else None, ctx_all)
    torch.testing.assert_close(ctx, agg, rtol=0, atol=1e-13)
    torch.testing.assert_close(lg, logits, rtol=0, atol=1e-13)
    assert tc.shape == ctx.shape and tl.shape == lg.shape and bool((tc > 0).all()) and bool(torch.isfinite(tc).all()) and bool(torch.isfinite(tl).all())
    # q, k, v handed in (paths_token0_tail's form) change nothing
    r = R.in_proj_ref(layers[1], x1, H)
    again = R.token0_tail_ref(layers[1], lvl, x1, num_ims, H, ctx_prev if ctx_mode == "residual" else None, ctx_all, qkv=(r["q"], r["k"], r["v"]))
    assert torch.equal(again[0], ctx) and torch.equal(again[1], lg)


def test_special_last_order_leaves_the_special_token_unchanged():
    """fused_token_order: patch i at row i, the special token at row num_ims[b].  Masked self-attention is invariant under that
    permutation of the valid rows, so two layers read at the special token give the same ctx_out and logits in either order."""
    d, H = 128, 4
    T, lens = DECODER_LENS
    layers, lvl, p, pre, x, num_ims, ctx_prev, _ = _decoder_problem(d, H, lens, T, 0, 23)
    xs, perm = R.fused_token_order(x, num_ims)
    for b, n in enumerate(num_ims.tolist()):
        assert torch.equal(xs[b, n], x[b, 0]) and torch.equal(xs[b, :n], x[b, 1:n + 1])
        assert perm[b, :n].tolist() == list(range(1, n + 1)) and int(perm[b, n]) == 0
        assert perm[b, n + 1:].tolist() == [min(j + 1, T - 1) for j in range(n + 1, T)]
    assert R.special_index(num_ims, True).tolist() == num_ims.tolist() and R.special_index(num_ims).tolist() == [0] * len(lens)
    first = R.decoder_layer_ref(layers[0], x, num_ims, H)
    last = R.decoder_layer_ref(layers[0], xs, num_ims, H, special_last=True)
    for b, n in enumerate(num_ims.tolist()):                     # the valid rows of the layer's output are the permuted rows
        torch.testing.assert_close(last["x_out"][b, :n + 1], first["x_out"][b][perm[b, :n + 1]], rtol=0, atol=1e-13)
    a = R.token0_tail_ref(layers[1], lvl, first["x_out"], num_ims, H, ctx_prev)
    b_ = R.token0_tail_ref(layers[1], lvl, last["x_out"], num_ims, H, ctx_prev, special_last=True)
    torch.testing.assert_close(b_[0], a[0], rtol=0, atol=1e-13)
    torch.testing.assert_close(b_[1], a[1], rtol=0, atol=1e-13)
    o_first = R.attention_ref(first["q"], first["k"], first["v"], num_ims, False, "special")
    o_last = R.attention_ref(last["q"], last["k"], last["v"], num_ims, True, "special")
    torch.testing.assert_close(o_last, o_first, rtol=0, atol=1e-13)
