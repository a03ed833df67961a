"""No result depends on memory the contract leaves undefined.

The float64 tests fix WHAT a kernel computes; these fix which memory it may look at while doing so.  Everything here is a run under
the fill patterns of tests/poison.py - Z (zero bytes), F (finite noise), H (NaN / Inf / 3e38 / 0xff bytes) - in every place the
contract calls a don't-care: padded rows of float inputs, pad columns between a row's width and its stride, the contents of
workspaces and operand images on entry, read-behind zones, the pre-fill of outputs.  The project has no float atomics, so the
criterion needs no tolerance: the DEFINED part of every output is bit-identical across the patterns (and finite under H), and the
guard bands around every buffer sized by a query are untouched.

Part 3 (first in the file, and to be run first): the C ABI, one entry point at a time, on the problems of the existing float64 tests
(their builders are imported, not copied; the cached problems stay as they are - a run works on a shallow copy whose padded rows
are poisoned).  Part 2: whole recursions and training steps with torch.empty poisoned (poison.poisoned_empty, guard bands on), which
shows that the package hands its kernels what their contracts ask for.

Only float and byte buffers are ever poisoned: indices, counts and address tables stay valid (poison.py's docstring), and no buffer
is undersized - a guard band sits BEHIND a workspace of exactly the queried size.  Float or byte buffers whose values become an index
or a count were looked for before the first run (csrc: the PE table is indexed by locs, the top-K key of rank_key.h only orders
scores and ranks by counting, the tissue / pack flags and candidate masks are written in full by the kernel in front of their
reader, max|x| goes through atomicMax on bits of rows the gathers wrote or zeroed): none needed to be excluded from H.  The one
byte buffer a test here hands to a kernel as INPUT flags (paths_pack_index) is written by paths_pack_flags first."""
import contextlib
import math

import pytest
import torch

from tests import poison as P
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)
from tests.test_gpu_row_backward import COVERAGE_CONFIGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F16, U8, I32, I64 = torch.float32, torch.float16, torch.uint8, torch.int32, torch.int64
LOG2E = math.log2(math.e)


def _lib():
    from paths_amd import _lib as L
    return L


def poison_where(t, keep, pattern, seed=0):
    """t with the elements where ``keep`` (broadcastable bool) is False replaced by the pattern of t's dtype."""
    return torch.where(keep, t, P.fill_(torch.zeros_like(t).contiguous(), pattern, seed)).contiguous()


def poison_where_f16(t, keep, pattern, seed=0):
    """The same for fp32 rows that are stored as fp16 (the _h16 forms): the poison is the fp16 pattern's values."""
    bad = P.fill_(torch.zeros(t.shape, dtype=F16, device=t.device), pattern, seed).float()
    return torch.where(keep, t, bad).contiguous()


def G(shape, pattern, dtype=F32, seed=0):
    return P.guarded(shape, dtype, pattern, device=DEV, seed=seed)


def zfh(label, run, runs=P.PATTERNS):
    """run(pattern) -> {name: defined output}; bit-identical over the patterns, finite under H, every guard band intact."""
    def fn(pattern):
        out = run(pattern)
        torch.cuda.synchronize()
        P.check_guards(f"{label} [{pattern}]")
        return out
    return P.assert_independent(fn, label, runs=runs)


def rows_valid(num_ims, N):
    """[B * N] bool: row b * N + i is a patch."""
    return (torch.arange(N, device=num_ims.device)[None, :] < num_ims[:, None]).reshape(-1)


@contextlib.contextmanager
def pattern_buffers(monkeypatch, pattern):
    """Inside: what the builders of tests/test_gpu_chain_forward.py and tests/test_gpu_aggregator_forward.py fill with their NaN
    sentinel (outputs, the bands of strided inputs, workspaces) holds ``pattern`` between guard bands instead, and so does everything
    they take from torch.empty at a size a query returned."""
    from tests import test_gpu_aggregator_forward as AGG, test_gpu_chain_forward as CF
    fill = lambda *shape: G(shape, pattern)      # noqa: E731
    with monkeypatch.context() as mp, P.poisoned_empty(pattern, guard=True):
        for mod in (CF, AGG):
            mp.setattr(mod, "_ffill", fill)
            mp.setattr(mod, "TAIL", 0)           # no spare elements or rows behind a buffer: each has exactly its documented size
            mp.setattr(mod, "GUARD_ROWS", 0)
        yield


# ================================================================================================
# 3a. forward attention
# ================================================================================================
ATTN_SHAPES = {"129": (129, [128, 77, 1]), "300": (300, [300, 37])}      # a padded row inside a tile, a whole tile of padding, an empty slide


def _head_major(T, lens, H=4, hd=32, seed=0):
    B = len(lens)
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 + T + hd + seed)
    q = (torch.rand(B, H, T, hd, device=DEV, generator=g) * 2 - 1) * 1.5
    k = (torch.rand(B, H, T, hd, device=DEV, generator=g) * 2 - 1) * 1.5
    v = torch.rand(B, H, T, hd, device=DEV, generator=g) * 2 - 1
    num_ims = torch.tensor([n - 1 for n in lens], device=DEV, dtype=I64)
    valid = torch.arange(T, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None]       # [B, T]
    return q, k, v, num_ims, valid


def _token_major(T, lens, H, hd, pad_cols, spare_rows, pattern, seed=0):
    """qkv [B * T + spare_rows, 3 d + pad_cols]: valid rows random, padded rows / pad columns / spare rows hold the pattern."""
    B, d = len(lens), H * hd
    g = torch.Generator(device=DEV)
    g.manual_seed(2000 + T + hd + seed)
    body = torch.randn(B * T, 3 * d, device=DEV, generator=g)
    valid = (torch.arange(T, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None])
    qkv = P.fill_(torch.zeros((B * T + spare_rows, 3 * d + pad_cols), device=DEV), pattern, seed)
    qkv[:B * T, :3 * d] = poison_where(body, valid.reshape(-1, 1), pattern, seed + 1)
    num_ims = torch.tensor([n - 1 for n in lens], device=DEV, dtype=I64)
    return qkv, num_ims, valid


@pytest.mark.parametrize("m32", ["0", "1", "3"])
@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("shape", sorted(ATTN_SHAPES))
def test_attention_x6_and_f32_ignore_padded_rows_and_workspace_contents(dev, shape, planes, m32, monkeypatch):
    """paths_attention_x6 (planes 2 and 3; the 16x16x32 kernel and the two 32x32x16 forms of PATHS_ATTN_M32) and paths_attention_f32:
    q / k / v rows behind a slide's last token, the operand-image workspace on entry (exactly paths_attention_x6_workspace bytes) and
    the pre-fill of o / lse.  Defined: o and lse of the valid query rows."""
    L = _lib()
    monkeypatch.setenv("PATHS_ATTN_M32", m32)
    T, lens = ATTN_SHAPES[shape]
    q0, k0, v0, num_ims, valid = _head_major(T, lens)
    B, H, hd = q0.shape[0], 4, 32
    p, st = L.ptr, L.stream()
    vq = valid[:, None, :, None]

    def run(pattern):
        q, k, v = (poison_where(x, vq, pattern, i) for i, x in enumerate((q0, k0, v0)))
        ws = G(int(L.load().paths_attention_x6_workspace(B, T, H, hd, planes)), pattern, U8)
        o, lse = G((B, T, H * hd), pattern), G((B, H, T), pattern)
        L.call("paths_attention_x6", p(q), p(k), p(v), p(o), p(lse), p(num_ims), B, T, H, hd, 0, p(ws), planes, 0, st)
        out = {"o": torch.where(valid[:, :, None], o, 0.0), "lse": torch.where(valid[:, None, :], lse, 0.0)}
        if planes == 2 and m32 == "0":
            o32, lse32 = G((B, T, H * hd), pattern), G((B, H, T), pattern)
            L.call("paths_attention_f32", p(q), p(k), p(v), p(o32), p(lse32), p(num_ims), B, T, H, hd, 0, st)
            out.update(o_f32=torch.where(valid[:, :, None], o32, 0.0), lse_f32=torch.where(valid[:, None, :], lse32, 0.0))
        return out

    zfh(f"attention_x6 planes {planes} M32 {m32} T {T}", run)


@pytest.mark.parametrize("hd", [16, 48, 64])
@pytest.mark.parametrize("shape", sorted(ATTN_SHAPES))
def test_attention_h3_any_and_token0_any_ignore_padding(dev, shape, hd):
    """paths_attention_h3_any and paths_attention_token0_any on the token-major in_proj output at ld = 3 d + 8: padded rows, the pad
    columns, both workspaces.  Defined: o of the valid rows, a0 of every slide."""
    L = _lib()
    T, lens = ATTN_SHAPES[shape]
    B, H = len(lens), 4
    d = H * hd
    p, st = L.ptr, L.stream()
    qs = LOG2E / math.sqrt(hd)

    def run(pattern):
        qkv, num_ims, valid = _token_major(T, lens, H, hd, 8, 0, pattern)
        ws = G(int(L.load().paths_attention_h3_any_workspace(B, T, H, hd)), pattern, U8)
        o = G((B, T, d), pattern)
        L.call("paths_attention_h3_any", p(qkv), 3 * d + 8, p(o), p(num_ims), B, T, H, hd, qs, p(ws), st)
        ws0 = G((int(L.load().paths_attention_token0_workspace(B, T, H)),), pattern)
        a0 = G((B, d), pattern)
        L.call("paths_attention_token0_any", p(qkv), 3 * d + 8, p(num_ims), p(a0), p(ws0), B, T, H, hd, qs, st)
        return {"o": torch.where(valid[:, :, None], o, 0.0), "a0": a0}

    zfh(f"attention_h3_any / token0_any hd {hd} T {T}", run)


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("shape", sorted(ATTN_SHAPES))
def test_attention_fp8_ignores_padding(dev, shape, hd):
    """paths_attention_fp8 (head-major q / k / v, head_dim 32) and paths_attention_fp8_qkv (token-major, ld = 3 d + 8): e4m3 is coarse
    but deterministic, so the bitwise criterion holds.  Defined: o of the valid rows."""
    L = _lib()
    T, lens = ATTN_SHAPES[shape]
    B, H = len(lens), 4
    d = H * hd
    p, st = L.ptr, L.stream()
    q0, k0, v0, num_h, valid_h = _head_major(T, lens, H, hd, seed=8)

    def run(pattern):
        qkv, num_ims, valid = _token_major(T, lens, H, hd, 8, 0, pattern, seed=8)
        ws = G(int(L.load().paths_attention_fp8_workspace(B, T, H, hd)), pattern, U8)
        o = G((B, T, d), pattern)
        L.call("paths_attention_fp8_qkv", p(qkv), 3 * d + 8, p(o), p(num_ims), B, T, H, hd, LOG2E / math.sqrt(hd), p(ws), st)
        out = {"o_qkv": torch.where(valid[:, :, None], o, 0.0)}
        if hd == 32:
            q, k, v = (poison_where(x, valid_h[:, None, :, None], pattern, i) for i, x in enumerate((q0, k0, v0)))
            ws2 = G(int(L.load().paths_attention_fp8_workspace(B, T, H, hd)), pattern, U8)
            o2 = G((B, T, d), pattern)
            L.call("paths_attention_fp8", p(q), p(k), p(v), p(o2), p(num_h), B, T, H, hd, p(ws2), st)
            out["o"] = torch.where(valid_h[:, :, None], o2, 0.0)
        return out

    zfh(f"attention_fp8 hd {hd} T {T}", run)


# ================================================================================================
# 3b. training attention (the cases of tests/test_gpu_attention_backward.py)
# ================================================================================================
# entry, head_dim, true head_dim, H, max_queries, dropout p, planes (x6 only)
TRAIN_ATTN = [("x6", 32, 32, 4, 0, 0.0, 2), ("x6", 32, 32, 4, 0, 0.1, 3), ("x6d", 32, 32, 4, 0, 0.1, 3), ("f32", 32, 32, 4, 0, 0.0, 3),
              ("f32", 32, 32, 4, 0, 0.1, 3), ("any", 48, 48, 3, 0, 0.1, 3), ("any", 16, 16, 3, 1, 0.0, 3), ("wide", 128, 128, 3, 0, 0.1, 3),
              ("wide", 96, 80, 3, 1, 0.0, 3), ("token0", 32, 32, 4, 1, 0.1, 3)]
# "read, must be finite" (include/paths_hip.h): padded rows that enter a matrix product beside an exact zero - the probabilities and
# dS of a padded query are zero by a select, but the other operand of the MFMA (dO in dV = P^T dO, q in dK = dS^T q, V in O = P V of
# the wide form) or the row sum D = sum dO o that is multiplied by them is not looked at: 0 * NaN.  These rows get F where the run's
# pattern is H; measured one region at a time on an MI355X, every other region of every entry takes H.  Part 2 shows that the
# training step hands these kernels finite rows (it computes padded rows instead of skipping them).
TRAIN_ATTN_FINITE = {"x6": ("o", "d_o"), "x6d": ("o", "d_o"), "f32": ("q", "o", "d_o"), "wide": ("qkv", "d_o")}


@pytest.mark.parametrize("T", [129, 300])
@pytest.mark.parametrize("entry,hd,hd_true,H,mq,p,planes", TRAIN_ATTN, ids=[f"{e}-hd{hd}-mq{mq}-p{p}-pl{pl}" for e, hd, _, _, mq, p, pl in TRAIN_ATTN])
def test_training_attention_ignores_padded_rows_and_workspaces(dev, entry, hd, hd_true, H, mq, p, planes, T):
    """Every training-attention entry point - forward: paths_attention_x6_dropout, _any_train, _wide_fwd, _token0_fwd; backward:
    paths_attention_bwd_f32(_dropout), _bwd_x6_planes, _bwd_x6_dropout, _bwd_any, _wide_bwd, _token0_bwd - on the ragged cases of the
    float64 tests with q / k / v / o / d_o / lse poisoned on the padded rows, the 128 readable rows behind a token-major qkv poisoned
    too, and ws_dsum, the operand images, the score scratch and the token-0 partials taken from a poisoned, guarded torch.empty at
    exactly the queried size.  dqkv is zero on entry, as the header asks, and the rows of TRAIN_ATTN_FINITE hold finite noise where
    the others hold NaN / Inf.  Defined: the whole of dqkv (padded rows stay exactly zero) and o / lse of the rows with a forward
    output."""
    from tests import test_gpu_attention_backward as AB
    c = AB.Case(dev, entry, T, hd, hd_true, H, mq, p, seed=T * 3 + hd)
    base = {n: getattr(c, n).clone() for n in ("q", "k", "v", "o_tok", "g_tok", "lse")}
    qkv0 = c.qkv.clone() if entry not in AB.HEAD_MAJOR else None
    B, d = c.B, c.d
    v4, v3, vl = c.valid[:, None, :, None], c.valid[:, :, None], c.valid[:, None, :]

    finite = TRAIN_ATTN_FINITE.get(entry, ())

    def run(pattern):
        rp = lambda region: "F" if (pattern == "H" and region in finite) else pattern      # noqa: E731  ("read, must be finite")
        c.q, c.k, c.v = (poison_where(base[n], v4, rp(n), i) for i, n in enumerate(("q", "k", "v")))
        c.o_tok, c.g_tok = poison_where(base["o_tok"], v3, rp("o"), 3), poison_where(base["g_tok"], v3, rp("d_o"), 4)
        c.lse = poison_where(base["lse"], vl, pattern, 5)
        c.a0, c.da0, c.lse0 = c.o_tok[:, 0].contiguous(), c.g_tok[:, 0].contiguous(), c.lse[:, :, 0].contiguous()
        if qkv0 is not None:
            c.qkv = poison_where(qkv0, torch.zeros((), dtype=torch.bool, device=dev), pattern, 6)      # (the spare rows behind the last slide)
            c.qkv[:B * T] = poison_where(qkv0[:B * T], c.valid.reshape(-1, 1), rp("qkv"), 7)
        with P.poisoned_empty(pattern, guard=True):
            dqkv = c.backward(torch.zeros((B, T, 3, d), device=dev), planes=planes)
            out = {"dqkv": dqkv}
            if entry in ("x6", "any", "wide", "token0"):
                o, lse = AB.forward(c, planes=2 if planes == 2 else 3)
                out["o"] = torch.where(c.live[:, None, :, None], o, 0.0)
                out["lse"] = torch.where(c.live[:, None, :], lse, 0.0)
        return out

    res = zfh(f"training attention {entry} T {T} hd {hd} mq {mq} p {p}", run)
    assert not res["dqkv"][~c.valid].any(), "dq / dk / dv of a padded row is not zero"


# ================================================================================================
# 3c. token-layer chain
# ================================================================================================
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("kernel", ["f32", "h3", "ws_rows"])
@pytest.mark.parametrize("shape", ["65", "130"])
def test_token_layer_kernels_ignore_padded_rows(dev, kernel, shape, skip, monkeypatch):
    """paths_token_layer_f32 / _h3 / _ws_rows (the problems of test_token_layer_kernels_match_float64), do_post and do_qkv together:
    x_in and attn rows behind a slide's last token, the pre-fill of x_out / q / k / v / qkv_rows and the pad columns of qkv_rows.
    Defined: the valid rows of every output."""
    from tests import test_gpu_aggregator_forward as AGG
    T, lens = AGG.LAYER_SHAPES[shape]
    pr = AGG._layer_problem(AGG.LAYER_KERNELS[kernel][1], T, lens)
    AGG._layer_run(kernel, pr, "both", skip)                                 # (builds the cached weight images outside the patch)
    valid = (torch.arange(T, device=DEV)[None, :] <= pr["num_ims"][:, None])[:, :, None]

    def run(pattern):
        pr2 = dict(pr, x=poison_where(pr["x"], valid, pattern, 1), attn=poison_where(pr["attn"], valid, pattern, 2))
        with pattern_buffers(monkeypatch, pattern):
            bufs = AGG._layer_run(kernel, pr2, "both", skip)
        return {n: torch.where(valid, v, 0.0) for n, v in AGG._layer_views(kernel, pr2, bufs, "both").items()}

    zfh(f"token_layer_{kernel} T {T} skip_padding {skip}", run)


@pytest.mark.parametrize("head", ["residual", "concat"])
@pytest.mark.parametrize("shape", ["300", "65"])
def test_token0_tail_ignores_padded_rows_and_partials(dev, shape, head, monkeypatch):
    """paths_token0_tail: x_in / q / k / v rows behind a slide's last token and ws_partials on entry.  Defined: ctx_out, logits."""
    from tests import test_gpu_aggregator_forward as AGG
    T, lens = AGG.TAIL_SHAPES[shape]
    pr = AGG._tail_problem(T, lens, head)
    B = pr["B"]
    valid = torch.arange(T, device=DEV)[None, :] <= pr["num_ims"][:, None]

    def run(pattern):
        pr2 = dict(pr, x=poison_where(pr["x"], valid[:, :, None], pattern, 1))
        for i, n in enumerate("qkv"):
            pr2[n] = poison_where(pr[n], valid[:, None, :, None], pattern, 2 + i)
        with pattern_buffers(monkeypatch, pattern):
            bufs = AGG._tail_buffers(pr2)
            AGG._tail_call(pr2, bufs)
        return {"ctx_out": bufs["ctx_out"][:B * 128], "logits": bufs["logits"][:B * 4]}

    zfh(f"token0_tail T {T} {head}", run)


@pytest.mark.parametrize("d,ws", [(128, True), (128, False), (192, True)], ids=["d128-tlayer_ws", "d128-tlayer_h3", "d192"])
@pytest.mark.parametrize("T,lens", [(300, [300, 37, 129]), (65, [64, 65, 1])])
def test_weight_stationary_aggregator_ignores_padding_and_workspaces(dev, T, lens, d, ws, monkeypatch):
    """The launches of test_token_layer_ws_and_tail_ws_vs_fp64 (paths_tlayer_pack_ws, paths_token_layer_ws, paths_attention_h3_img,
    paths_token0_pack_ws_d, paths_token0_tail_ws; d = 192: paths_token_layer_ws_rows and the generic attention; tlayer_h3:
    paths_tlayer_pack_h3, paths_token_layer_h3 writing qkv_images, paths_attention_x6 on ready images, paths_token0_tail) with the
    token rows behind every slide's last one poisoned and every buffer the aggregator allocates - operand images, the attention
    output image, row buffers, ws_partials, the weight images before they are packed - poisoned between guard bands.
    Defined: ctx_slide and logits."""
    from paths_amd import ops
    if ops.GEMM_MODE != "h3":
        pytest.skip("default-mode kernels")
    B, Hh = len(lens), 4
    gen = torch.Generator(device=dev)
    gen.manual_seed(T + d)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=gen) * 2 - 1      # noqa: E731
    layers = []
    for _ in range(2):
        lay = {"wqkv": rnd(3 * d, d) * 0.15, "bqkv": rnd(3 * d) * 0.1, "wo": rnd(d, d) * 0.1, "bo": rnd(d) * 0.1, "cab": rnd(d) * 0.1,
               "w1": rnd(4 * d, d) * 0.1, "b1": rnd(4 * d) * 0.1, "w2": rnd(d, 4 * d) * 0.05, "b2": rnd(d) * 0.1, "eps": 1e-5}
        for n in ("ln1", "ln2", "ln3"):
            lay[n + "g"], lay[n + "b"] = 1 + rnd(d) * 0.1, rnd(d) * 0.1
        layers.append(lay)
    head = {"lnfg": 1 + rnd(d) * 0.1, "lnfb": rnd(d) * 0.1, "lnf_eps": 1e-5, "wcls": rnd(4, d) * 0.1, "bcls": rnd(4) * 0.1}

    class MC:
        trans_dim, trans_heads, trans_layers, slide_ctx_mode, importance_mlp_hidden_dim = d, Hh, 2, "residual", 128
    tokens0, ctx_prev = rnd(B, T, d), rnd(B, d)
    num_ims = torch.tensor([n - 1 for n in lens], device=dev, dtype=I64)
    valid = (torch.arange(T, device=dev)[None, :] <= num_ims[:, None])[:, :, None]
    monkeypatch.setattr(ops, "TLAYER_WS", ws)

    def run(pattern):
        lvl = dict(head, layers=[dict(lay) for lay in layers])                # fresh pack dicts: the weight images are packed in this run
        with P.poisoned_empty(pattern, guard=True) as sites:
            out = ops._aggregator_forward(MC, lvl, poison_where(tokens0, valid, pattern, 1), num_ims, ctx_prev, None)
        assert sites.filled_bytes() > 0
        return {"ctx_slide": out["ctx_slide"], "logits": out["logits"]}

    zfh(f"aggregator d {d} T {T} {'ws' if ws else 'h3'}", run)


# ================================================================================================
# 3d. gate and importance GEMMs
# ================================================================================================
LSTM_FORMS = [(2, "hp", "matrix", "inf"), (2, "none", "rows", "inf"), (2, "hp", "h16", "inf"), (2, "h0c0", "matrix", "train"),
              (2, "hp", "rows", "frm"), (3, "hp", "matrix", "train"), (3, "h0c0", "matrix", "y")]


@pytest.mark.parametrize("rps", [300, 60])
@pytest.mark.parametrize("planes,state,a_form,out_form", LSTM_FORMS, ids=[f"p{p}-{s}-{a}-{o}" for p, s, a, o in LSTM_FORMS])
def test_lstm_cell_x6_ignores_padded_rows(dev, planes, state, a_form, out_form, rps, monkeypatch):
    """paths_lstm_cell_x6 / _h16 with num_ims (M = 300 as one slide of 130 patches - the third 128-row block is all padding - and as
    five slides of 60, one of them empty): the rows of x (fp16 rows: the fp16 pattern) and of c0 / state_prev behind a slide's last
    patch, the pad columns of every strided operand, the ws_o scratch and the pre-fill of every output.  Defined: the valid rows of
    h1, c1 and, by form, y, f|r|m, tc and the output gate."""
    from tests import test_gpu_chain_forward as CF
    D, Hc, M = 256, 128, 300
    pr = CF._lstm_problem(D, Hc, M, state, False, a_form in ("rows", "h16"))
    num_ims = CF._ragged_counts(M, rps)
    valid = rows_valid(num_ims, rps)[:, None]
    CF._lstm_run(pr, planes, a_form, out_form, num_ims, rps)                 # (the cached weight images, outside the patch)

    def run(pattern):
        pw = poison_where_f16 if a_form == "h16" else poison_where
        pr2 = dict(pr, x=pw(pr["x"], valid, pattern, 1))
        if state == "hp":
            pr2["c0"] = poison_where(pr["c0"], valid, pattern, 2)
        elif state == "h0c0":
            st = G(tuple(pr["state_prev"].shape), pattern, seed=3)             # the band behind D + Hc holds the pattern too
            st[:, :D + Hc] = poison_where(pr["state_prev"][:, :D + Hc], valid, pattern, 2)
            pr2["state_prev"] = st
        with pattern_buffers(monkeypatch, pattern):
            bufs = CF._lstm_run(pr2, planes, a_form, out_form, num_ims, rps)
        return {n: torch.where(valid, v[:M], 0.0) for n, v in CF._lstm_rows(pr2, bufs, out_form).items()}

    zfh(f"lstm_cell p{planes} {state} {a_form} {out_form} rps {rps}", run)


IMP_RUNS = [("p2-add", "60x5", 1, 0, 0), ("p2-add", "4x64", 0, 1, 1), ("p3-y", "60x5", 1, 1, 0), ("sk-add", "60x5", 1, 1, 0), ("sk-add", "4x64", 1, 0, 0),
            ("sk-rows-add", "4x64", 0, 1, 0), ("h16", "60x5", 1, 0, 0), ("h16", "4x64", 1, 1, 0), ("p2-rows-add", "60x5", 0, 0, 1)]


@pytest.mark.parametrize("form,layout,imp_mul,skip,save", IMP_RUNS, ids=[f"{f}-{l}-mul{m}-skip{s}-save{v}" for f, l, m, s, v in IMP_RUNS])
def test_importance_proj_x6_ignores_padded_rows_and_splitk_workspace(dev, form, layout, imp_mul, skip, save, monkeypatch):
    """paths_importance_proj_x6 / _h16: the rows of y (fp16 rows: the fp16 pattern) and y_add behind a slide's last patch, the pad
    columns, the split-K workspace (exactly paths_importance_proj_x6_workspace bytes) and the pre-fill of the outputs.  Defined:
    importance (skip_padding 0: all of it, padded rows exactly +0.0), the token rows of valid patches and the special token's row,
    the saves of valid rows."""
    from tests import test_gpu_chain_forward as CF
    D, B, N, pe_mode, ps = CF.IMP_LAYOUTS[layout]
    pr = CF._imp_problem(D, B, N, pe_mode, ps)
    M = pr["M"]
    CF._imp_run(pr, form, True, imp_mul, skip, save)
    valid = rows_valid(pr["num_ims"], N)
    special = torch.ones((B, 1), dtype=torch.bool, device=DEV) if skip == 0 else (pr["num_ims"] > 0)[:, None]
    tokvalid = torch.cat([special, valid.view(B, N)], dim=1)

    def run(pattern):
        pw = poison_where_f16 if form == "h16" else poison_where
        pr2 = dict(pr, y=pw(pr["y"], valid[:, None], pattern, 1), y_add=poison_where(pr["y_add"], valid[:, None], pattern, 2))
        with pattern_buffers(monkeypatch, pattern):
            v = CF._imp_views(pr2, CF._imp_run(pr2, form, True, imp_mul, skip, save))
        out = {"importance": v["importance"] if skip == 0 else torch.where(valid, v["importance"], 0.0),
               "tokens": torch.where(tokvalid[:, :, None], v["tokens"], 0.0)}
        for n in ("hid", "pproj"):
            if n in v:
                out[n] = torch.where(valid[:, None], v[n], 0.0)
        return out

    res = zfh(f"importance_proj {form} {layout} imp_mul {imp_mul} skip {skip} save {save}", run)
    assert M == B * N and bool((res["importance"].view(I32)[~valid] == 0).all()), "importance of a padded row is not +0.0"


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("form", ["matrix", "rows", "h16"])
@pytest.mark.parametrize("layout", ["3x64", "5x64"])
def test_importance_qkv_x6_ignores_padded_rows_and_workspaces(dev, layout, form, skip, monkeypatch):
    """paths_importance_qkv_x6 / _h16 (phases 5) and paths_attention_x6 on the images it wrote: the rows of y and y_add behind a slide's
    last patch, splitk_ws and qkv_images on entry.  Defined: importance, the token slots up to the special token, o of those slots."""
    from tests import test_gpu_chain_forward as CF
    pr = CF._fq_problem(layout, 2)
    CF._fq_run(pr, form, 1, skip)
    valid, tokvalid, _ = CF._fq_masks(pr)

    def run(pattern):
        pw = poison_where_f16 if form == "h16" else poison_where
        pr2 = dict(pr, y_add=poison_where(pr["y_add"], valid[:, None], pattern, 2))
        with pattern_buffers(monkeypatch, pattern):
            v = CF._fq_views(pr2, CF._fq_run(pr2, form, 1, skip, y=pw(pr["y"], valid[:, None], pattern, 1)))
        return {"importance": v["importance"] if skip == 0 else torch.where(valid, v["importance"], 0.0),
                "tokens": torch.where(tokvalid[:, :, None], v["tokens"], 0.0), "o": torch.where(tokvalid[:, :, None], v["o"], 0.0)}

    zfh(f"importance_qkv {form} {layout} skip {skip}", run)


@pytest.mark.parametrize("form", ["matrix", "rows", "h16"])
@pytest.mark.parametrize("N,Npad", [(320, 384), (300, 512)])
def test_gemm_add_and_row_gemm_ignore_padded_rows(dev, N, Npad, form, monkeypatch):
    """paths_gemm_add_nt_x6 / _h16 with num_ims = [128, 0, 5] at 128 rows per slide (the second tile is all padding): the rows of a and
    a_add behind a slide's last patch, the pad columns, the pre-fill of out; and paths_gemm_rows_nt_x6 over the same rows (no row is
    padding there: every address counts), into a poisoned out.  Defined: the valid rows of out / every row."""
    from tests import test_gpu_chain_forward as CF
    L = _lib()
    M, K = 384, 256
    pr = CF._gemm_add_problem(M, N, Npad, K, form == "h16")
    num_ims = torch.tensor([128, 0, 5], dtype=I64, device=DEV)
    valid = rows_valid(num_ims, 128)[:, None]

    def run(pattern):
        pw = poison_where_f16 if form == "h16" else poison_where
        pr2 = dict(pr, a=pw(pr["a"], valid, pattern, 1), add=poison_where(pr["add"], valid, pattern, 2))
        with pattern_buffers(monkeypatch, pattern):
            out = CF._gemm_add_run(pr2, form, 1, True, num_ims, 128)
        res = {"out": torch.where(valid, out[:M, :N], 0.0)}
        if form == "rows" and Npad % 256 == 0:
            rows = (pr["a"].data_ptr() + torch.arange(M, device=DEV, dtype=I64) * (K * 4)).contiguous()
            o2 = G((M, Npad + 4), pattern)
            L.call("paths_gemm_rows_nt_x6", rows.data_ptr(), pr["img"].data_ptr(), K, 0, o2.data_ptr(), Npad + 4, M, Npad, K, 2, pr["w_scale"],
                   CF.A_SCALE, L.stream())
            res["rows_out"] = o2[:, :Npad]
        return res

    zfh(f"gemm_add {form} N {N} Npad {Npad}", run)


# ================================================================================================
# 3e. reductions over rows: every row of A and B counts; the slabs and the pre-fill of out do not
# ================================================================================================
def _mat(M, N, ld, pattern, seed):
    """[M, N] random values inside a pattern-filled [M, ld] buffer."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    buf = P.fill_(torch.zeros((M, ld), device=DEV), pattern, seed)
    buf[:, :N] = torch.rand((M, N), device=DEV, generator=g) * 2 - 1
    return buf


@pytest.mark.parametrize("kind,M,N1,N2,splits", [("f32", 333, 132, 260, 4), ("f32", 64, 36, 128, 1), ("x6p3", 300, 128, 256, 4), ("x6p2", 300, 256, 256, 3),
                                                 ("x6p2", 40, 128, 128, 4)])
def test_gemm_tn_ignores_slabs_and_pad_columns(dev, kind, M, N1, N2, splits):
    """paths_gemm_tn_f32 / paths_gemm_tn_x6 (planes 3 and 2): the split workspace (exactly paths_gemm_tn_workspace floats), the pad
    columns of A and B and the pre-fill of out (accumulate = 0).  Every ROW of A and B counts - the kernels sum over M without a mask."""
    L = _lib()
    p, st = L.ptr, L.stream()

    def run(pattern):
        a, b = _mat(M, N1, N1 + 4, pattern, 1), _mat(M, N2, N2 + 8, pattern, 2)
        ws = G((int(L.load().paths_gemm_tn_workspace(N1, N2, splits)),), pattern)
        out = G((N1, N2 + 4), pattern)
        if kind == "f32":
            L.call("paths_gemm_tn_f32", p(a), N1 + 4, p(b), N2 + 8, 0, None, 0, p(out), N2 + 4, M, N1, N2, splits, 0, p(ws), st)
        else:
            L.call("paths_gemm_tn_x6", p(a), N1 + 4, p(b), N2 + 8, 0, None, 0, p(out), N2 + 4, M, N1, N2, splits, 0, p(ws), int(kind[-1]), st)
        return {"out": out[:, :N2]}

    zfh(f"gemm_tn {kind} M {M} {N1}x{N2} splits {splits}", run)


@pytest.mark.parametrize("M,N,splits", [(777, 192, 12), (7, 36, 4), (1000, 129, 15)])
def test_colsum_ignores_slabs_and_pad_columns(dev, M, N, splits):
    """paths_colsum_f32 (16-byte and scalar kernels; splits above M leave slabs without rows): the slab workspace and the pre-fill of out."""
    L = _lib()

    def run(pattern):
        a = _mat(M, N, N + (4 if N % 4 == 0 else 1), pattern, 3)
        ws, out = G((splits * N,), pattern), G((N,), pattern)
        L.call("paths_colsum_f32", a.data_ptr(), a.stride(0), M, N, out.data_ptr(), splits, 0, ws.data_ptr(), L.stream())
        return {"out": out}

    zfh(f"colsum M {M} N {N} splits {splits}", run)


@pytest.mark.parametrize("d,rows,rpb", [(128, 300, 64), (128, 5, 7), (192, 300, 64), (36, 65, 256)])
def test_layernorm_bwd_sums_and_reduce_slabs_ignore_what_the_slabs_held(dev, d, rows, rpb):
    """paths_layernorm_bwd_sums / _any into poisoned dx and slabs, then paths_reduce_slabs_f32 over them into a poisoned out."""
    L = _lib()
    p, st = L.ptr, L.stream()
    g = torch.Generator(device=DEV)
    g.manual_seed(d + rows)
    dy, xh = (torch.randn(rows, d, device=DEV, generator=g) for _ in range(2))
    rs, gamma = torch.rand(rows, device=DEV, generator=g) + 0.5, torch.rand(d, device=DEV, generator=g) * 2 - 1
    nblk = (rows + rpb - 1) // rpb

    def run(pattern):
        dx, slabs, gb = G((rows, d), pattern), G((nblk, 3 * d), pattern), G((3 * d,), pattern)
        L.call("paths_layernorm_bwd_sums" + ("" if d == 128 else "_any"), p(dy), p(xh), p(rs), p(gamma), p(dx), p(slabs), rows, d, rpb, st)
        L.call("paths_reduce_slabs_f32", p(slabs), nblk, 3 * d, p(gb), 0, st)
        return {"dx": dx, "slabs": slabs, "sums": gb}

    zfh(f"layernorm_bwd_sums d {d} rows {rows} rpb {rpb}", run)


# ================================================================================================
# 3f. packers and the pack kernels: every byte of the image is written
# ================================================================================================
def test_weight_packers_write_every_byte_of_their_image(dev):
    """paths_x6_pack_weights (planes 2, 3, 4; rows padded to Npad), paths_x6_pack_weights_t (K padded behind Kvalid),
    paths_tlayer_pack_ws (d 128 and 192, both parts), paths_tlayer_pack_h3, paths_token0_pack_ws_d (128, 192) and paths_fp8_pack_weight
    into images of exactly the queried size that held zero bytes, finite noise or 0xff bytes: the images come out identical, so every
    byte is written (the contract the header states) and a consumer never sees what the buffer held."""
    L = _lib()
    lib = L.load()
    p, st = L.ptr, L.stream()
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    rnd = lambda *s: (torch.rand(*s, device=DEV, generator=g) * 2 - 1) * 0.1      # noqa: E731
    w, wt = rnd(300, 256), rnd(200, 384)
    lay = {d: {"wqkv": rnd(3 * d, d), "bqkv": rnd(3 * d), "wo": rnd(d, d), "bo": rnd(d), "w1": rnd(4 * d, d), "w2": rnd(d, 4 * d)} for d in (128, 192)}
    w8src = rnd(300, 128)

    def run(pattern):
        out = {}
        for planes in (2, 3, 4):
            img = G(int(lib.paths_x6_packed_bytes(384, 256, planes)), pattern, U8)
            L.call("paths_x6_pack_weights", p(w), 256, p(img), 300, 384, 256, planes, 64.0 if planes == 2 else 1.0, st)
            out[f"x6_p{planes}"] = img
        for planes in (3, 4):                                                # W^T of [Kvalid = 200, N = 384]: K padded to 256
            img = G(int(lib.paths_x6_packed_bytes(384, 256, planes)), pattern, U8)
            L.call("paths_x6_pack_weights_t", p(wt), 384, p(img), 384, 384, 256, 200, planes, st)
            out[f"x6_t_p{planes}"] = img
        for d in (128, 192):
            for part in (0, 1):
                img = G(int(lib.paths_tlayer_ws_image_bytes(part, d)), pattern, U8)
                ws = [lay[d]["wo"], lay[d]["w1"], lay[d]["w2"]] if part == 0 else [lay[d]["wqkv"], None, None]
                L.call("paths_tlayer_pack_ws", part, p(ws[0]), p(ws[1]), p(ws[2]), 1024.0, 1024.0, 1024.0, p(img), d, st)
                out[f"tlayer_ws_{d}_{part}"] = img
            img = G(int(lib.paths_token0_ws_image_bytes_d(d)), pattern, U8)
            L.call("paths_token0_pack_ws_d", p(lay[d]["wqkv"]), p(lay[d]["bqkv"]), p(lay[d]["wo"]), p(lay[d]["bo"]), p(lay[d]["w1"]), p(lay[d]["w2"]),
                   LOG2E / math.sqrt(d // 4), d, p(img), st)
            out[f"token0_ws_{d}"] = img
        assert int(lib.paths_token0_ws_image_bytes()) == int(lib.paths_token0_ws_image_bytes_d(128))
        for part in (0, 1):
            img = G(int(lib.paths_tlayer_h3_image_bytes(part)), pattern, U8)
            ws = [lay[128]["wo"], lay[128]["w1"], lay[128]["w2"]] if part == 0 else [lay[128]["wqkv"], None, None]
            L.call("paths_tlayer_pack_h3", part, p(ws[0]), p(ws[1]), p(ws[2]), 1024.0, 1024.0, 1024.0, p(img), st)
            out[f"tlayer_h3_{part}"] = img
        w8, sc, scratch = G((512, 128), pattern, U8), G((1,), pattern), torch.zeros((1,), dtype=I32, device=DEV)
        L.call("paths_fp8_pack_weight", p(w8src), 128, 300, 128, p(w8), p(sc), p(scratch), st)
        out["fp8_w8"], out["fp8_scale"] = w8, sc
        return out

    zfh("weight packers", run)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_pack_kernels_ignore_what_their_outputs_and_partials_held(dev, dtype):
    """paths_pack_flags[_h16] -> paths_pack_index -> paths_pack_rows[_h16] on a 37 x 29 grid with holes: flags (bytes, poisoned; written
    in full by the first kernel before the second counts them), the int32 partials (paths_pack_index_partials words between guard
    bands; integer buffers are never poisoned), index, count and rows.  Defined: all of index, count, and the packed rows."""
    L = _lib()
    p, st = L.ptr, L.stream()
    cells, D = 37 * 29, 64
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    grid = torch.randn(cells, D, device=DEV, generator=g)
    grid[torch.rand(cells, device=DEV, generator=g) < 0.4] = 0
    grid = grid.to(dtype).contiguous()
    sfx = "_h16" if dtype == F16 else ""
    n = int((grid != 0).any(dim=1).sum())

    def run(pattern):
        flags = G((cells,), pattern, U8)
        index, count = G((cells,), pattern, I32), G((1,), pattern, I32)
        partials = G((int(L.load().paths_pack_index_partials(cells)),), pattern, I32)
        rows = G((n, D), pattern, dtype)
        L.call("paths_pack_flags" + sfx, p(grid), cells, D, p(flags), st)
        L.call("paths_pack_index", p(flags), cells, p(index), p(count), p(partials), st)
        L.call("paths_pack_rows" + sfx, p(grid), cells, D, p(index), n, p(rows), st)
        return {"flags": flags, "index": index, "count": count, "rows": rows}

    res = zfh(f"pack kernels {dtype}", run)
    assert int(res["count"]) == n and int(res["flags"].sum()) == n


# (the size queries behind these buffers are listed, each with its guarded run, in tests/test_gpu_chain_forward.py:SIZE_QUERY_RUNS)


# ================================================================================================
# 2. end to end: inference
# ================================================================================================
def _bases(base):
    """Three slides whose level-0 grids differ, so that level 0 has padded rows too (level 0 keeps every cell of a grid: three equal
    grids would leave it without padding)."""
    return [base, (base[0] - 1, base[1]), (base[0], base[1] - 2)]


def _recursion_outputs(tag, out, trace, B):
    """name -> tensor of the DEFINED part of one recursion's results (undefined entries zeroed by the run's own num_ims, which is
    compared as well)."""
    res = {f"{tag}.logits": out["logits"], f"{tag}.ctx_slide": out["ctx_slide"], f"{tag}.status": out["status"]}
    for l, rec in enumerate(trace):
        n = rec["num_ims"]
        N = rec["locs"].shape[1]
        valid = torch.arange(N, device=n.device)[None, :] < n[:, None]
        res[f"{tag}.L{l}.num_ims"] = n
        res[f"{tag}.L{l}.locs"] = torch.where(valid[:, :, None], rec["locs"], 0)
        res[f"{tag}.L{l}.parent_inds"] = torch.where(valid, rec["parent_inds"], 0)
        res[f"{tag}.L{l}.importance"] = rec["importance"].reshape(B, N)
        res[f"{tag}.L{l}.logits"], res[f"{tag}.L{l}.ctx_slide"] = rec["logits"], rec["ctx_slide"]
        if "keep_idx" in rec:
            kc = rec["keep_count"]
            kv = torch.arange(rec["keep_idx"].shape[1], device=n.device)[None, :] < kc[:, None]
            res[f"{tag}.L{l}.keep_count"], res[f"{tag}.L{l}.keep_idx"] = kc, torch.where(kv, rec["keep_idx"], 0)
    last = trace[-1]
    N = last["locs"].shape[1]
    valid = torch.arange(N, device=DEV)[None, :] < last["num_ims"][:, None]
    cp = out.get("ctx_patch")
    if cp is not None and cp.numel():
        cp = cp.reshape(B, N, -1)
        res[f"{tag}.ctx_patch"] = torch.where(valid[:, :, None], cp, 0.0)
    else:
        cp = None
    return res, cp, valid


def _hostile_words(t):
    """bool like t (fp32): the element is one of the hostile bit patterns."""
    return torch.isin(t.contiguous().view(I32), torch.tensor(P._signed(P.HOSTILE_F32, 32), dtype=I32, device=t.device))


# beyond the forward gate's configurations: wide heads (head_dim 128: csrc/attn_wide.hip, whose qkv rows must be finite)
EXTRA_CONFIGS = {"td256_h2": ({"model_config": {"trans_dim": 256, "trans_heads": 2}}, False, set())}


def _inference_run(cfg_name, pattern, **kw):
    """The forward gate's recursion of one configuration on a dense, a packed and an on-demand batch under ``pattern``."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch, OnDemandSlide
    from tests.test_gpu_chain_forward import FORWARD_CONFIGS, FORWARD_SIZES
    over, half, _ = FORWARD_CONFIGS[cfg_name] if cfg_name in FORWARD_CONFIGS else EXTRA_CONFIGS[cfg_name]
    top_k, base = FORWARD_SIZES.get(cfg_name, (16, (6, 7)))
    c, model, _ = build_model(DEV, 3, over, top_k_patches=[top_k] * 4)         # a fresh model per run: its weight images are packed in it
    skw = {"dtype": F16} if half else {}
    res, info = {}, {"ragged": [], "poison_left": 0, "padding_zero": True}
    with P.poisoned_empty(pattern, guard=True) as sites, torch.no_grad():
        slides = [DeviceSlide.synthetic(14, sid, b, p_bg=0.1, device=DEV, **skw) for sid, b in enumerate(_bases(base))]
        batches = {"dense": slides, "packed": DeviceSlideBatch([s.pack() for s in slides]), "on_demand": [OnDemandSlide.from_slide(s) for s in slides]}
        for tag, batch in batches.items():
            trace = []
            out = putils.recurse(model, batch, c.top_k_patches, 5, trace=trace, **kw)
            torch.cuda.synchronize()
            r, cp, valid = _recursion_outputs(tag, out, trace, 3)
            for l, rec in enumerate(trace):
                for key in ("attention", "attention_self", "rollout", "rollout_self"):
                    if key in rec:
                        r[f"{tag}.L{l}.{key}"] = rec[key]
            res.update(r)
            info["ragged"].append([bool((rec["num_ims"] < rec["locs"].shape[1]).any()) for rec in trace])
            info["padding_zero"] &= all(bool((rec["importance"].reshape(3, -1).view(I32)[~(torch.arange(rec["locs"].shape[1], device=DEV)[None, :]
                                                                                        < rec["num_ims"][:, None])] == 0).all()) for rec in trace)
            if pattern == "H" and cp is not None:
                info["poison_left"] += int(_hostile_words(cp)[~valid].sum())
    torch.cuda.synchronize()
    P.check_guards(f"{cfg_name} [{pattern}]")
    info["modules"] = sites.modules()
    return res, info


def _check_inference(cfg_name, **kw):
    infos = {}

    def fn(pattern):
        res, info = _inference_run(cfg_name, pattern, **kw)
        infos[pattern] = info
        assert all(all(r) for r in info["ragged"]), f"{cfg_name}: a level without a padded row: {info['ragged']}"
        assert info["padding_zero"], f"{cfg_name} [{pattern}]: importance of a padded entry is not +0.0"
        return res

    res = P.assert_independent(fn, cfg_name, runs=P.RUNS)
    for tag in ("dense", "packed", "on_demand"):
        assert int(res[f"{tag}.status"].item()) == 0, f"{cfg_name} {tag}: status word {int(res[f'{tag}.status'].item())}"
    mods = infos["H"]["modules"]
    assert {"paths_amd.ops", "paths_amd.utils"} <= mods, sorted(mods)
    print(f"[undefined] {cfg_name}: {len(res)} outputs bit-identical; hostile words left in padded ctx_patch rows: {infos['H']['poison_left']}")
    return infos


@pytest.mark.parametrize("cfg", ["shipped_k16", "fp16_grids", "td192", "nolstm", "td64_h1_hi36_nolstm", "hc64", "shipped_k64", "fp16_grids_k64",
                                 "td192_fp16_grids"])
def test_inference_does_not_depend_on_undefined_memory(dev, cfg):
    """Every configuration of the forward gate (tests/test_gpu_chain_forward.py:FORWARD_CONFIGS but the training forward): K = 16 on a
    6 x 7 base - K = 64 on 16 x 16 for the _k64 entries - three slides, five levels, on a dense, a packed and an on-demand batch, run
    under Z, Z, F and H with every torch.empty of the package poisoned between guard bands (slides, weight images, workspaces,
    operand images, per-level state).  The three slides' level-0 grids differ by a row / two columns so that every level, level 0
    included, has a padded row (asserted).  Z against Z: determinism; F and H against Z: logits, ctx_slide, the status word (0),
    every level's importance (padded entries exactly +0.0), num_ims, locs / parent_inds / kept indices on their valid entries, and
    the last level's ctx_patch on rows below num_ims.  Under H the hostile words are still there in a padded row of ctx_patch - the
    poison was real - and the recorded call sites include ops.py and utils.py."""
    from tests.test_gpu_chain_forward import FORWARD_CONFIGS
    assert set(FORWARD_CONFIGS) - {"training_forward"} == {"shipped_k16", "fp16_grids", "td192", "nolstm", "td64_h1_hi36_nolstm", "hc64",
                                                            "shipped_k64", "fp16_grids_k64", "td192_fp16_grids"}, "a new forward configuration belongs here too"
    infos = _check_inference(cfg)
    assert infos["H"]["poison_left"] > 0, "no hostile word survived in a padded row of ctx_patch: was the poison there?"


def test_wide_head_inference_does_not_depend_on_undefined_memory(dev):
    """trans_dim 256 with two heads of 128: the wide-head attention asks for FINITE rows behind a slide's last token (its products
    multiply them by exact zeros); the generic aggregator in front of it writes bp + PE into padded token rows, so it gets them."""
    _check_inference("td256_h2")


def test_attention_and_rollout_exports_do_not_depend_on_undefined_memory(dev):
    """The shipped configuration with the attention and rollout exports on: their outputs (0 on padding) and workspaces
    (paths_token0_attention_workspace / paths_attention_rollout_workspace floats, between guard bands) under the same four runs."""
    _check_inference("shipped_k16", attention=True, rollout=True)


# ================================================================================================
# 2. end to end: training
# ================================================================================================
def _training_run(over, dropout, pattern):
    from paths_amd import utils as putils
    from paths_amd.optim import HipAdamW
    from tests.test_gpu_backward import _train_setup
    torch.manual_seed(7)
    c, model, _, _, batch = _train_setup(DEV, top_k=16, base=(6, 7), n_slides=3, cfg_over=over)      # fresh weights, no cached image
    for proc in model.procs:
        proc.config.dropout = dropout
    model.train()
    with P.poisoned_empty(pattern, guard=True) as sites:
        opt = HipAdamW(model.parameters(), lr=1e-4)
        out = putils.recurse_train(model, batch["slide"], c.top_k_patches, 5)
        _, loss = putils.loss_from_logits(out["logits"], batch, "survival")
        loss.backward()
        torch.cuda.synchronize()
        res = {"loss": loss.detach().clone(), "status": out["status"].clone(), "logits": out["logits"].detach().clone()}
        for name, prm in model.named_parameters():
            if prm.grad is not None:
                res["grad." + name] = prm.grad.clone()
        opt.step()
        torch.cuda.synchronize()
        for name, prm in model.named_parameters():
            res["param." + name] = prm.detach().clone()
    P.check_guards(f"training [{pattern}]")
    return res, sites.modules()


def _check_training(label, over, dropout):
    mods = {}

    def fn(pattern):
        res, mods[pattern] = _training_run(over, dropout, pattern)
        return res

    res = P.assert_independent(fn, label, runs=P.RUNS)
    assert int(res["status"].item()) == 0
    grads = [k for k in res if k.startswith("grad.")]
    assert len(grads) > 50 and all(bool(torch.isfinite(res[k]).all()) for k in grads), "a gradient is not finite"
    assert {"paths_amd.backward", "paths_amd.ops", "paths_amd.utils"} <= mods["H"], sorted(mods["H"])
    print(f"[undefined] training {label}: loss {float(res['loss']):.6f}, {len(grads)} gradients and {len(res) - len(grads) - 3} parameters bit-identical")


@pytest.mark.parametrize("cfg", list(COVERAGE_CONFIGS))
def test_training_step_does_not_depend_on_undefined_memory(dev, cfg):
    """recurse_train, the loss, backward() and one HipAdamW step of every configuration of the backward gate
    (tests/test_gpu_row_backward.py:COVERAGE_CONFIGS) from the same initial weights under Z, Z, F and H, with every torch.empty of
    the package - saved activations, operand images, split-K and slab workspaces, gradient buffers - poisoned between guard bands:
    bit-identical loss, gradient of every live parameter and parameters after the step; every gradient finite; the recorded call
    sites include backward.py."""
    _check_training(cfg, COVERAGE_CONFIGS[cfg], 0.0)


def test_training_step_with_shipped_dropout_does_not_depend_on_undefined_memory(dev):
    """The same with the shipped dropout (0.05; test_training_with_shipped_dropout_config's configuration) and the same seed per run."""
    from paths_amd import ops
    if ops.GEMM_MODE == "f32":
        pytest.skip("dropout needs the split-operand attention kernel: PATHS_GEMM_MODE=f32 rejects it loudly (backward.py)")
    _check_training("shipped dropout 0.05", None, 0.05)
