"""The aggregator's forward kernels that no test had called on inputs of its own, one entry point at a time, against the float64
references of tests/chain_ref.py (decoder_layer_ref, attention_ref, token0_tail_ref): paths_token_layer_f32, paths_token_layer_h3,
paths_token_layer_ws_rows, paths_token0_tail and paths_attention_h3_any_img.

Conventions of tests/test_gpu_chain_forward.py: every output is pre-filled with the NaN sentinel, the entry point is called through
_lib.call, valid rows are compared with float64 under two conditions (the per-element bound chain_ref propagates, and
err <= 4 * err32 + ACT * n with err32 the error of the same formula in torch fp32 on the device and n the normalisation stages on the
output's path), padded rows against the kernel's stated contract, and everything beyond the documented extents must keep the sentinel.
Each test prints the measured maxima (run with -s); the maxima of the first run are recorded in the docstrings.

The per-element bound of an output behind the feed-forward sums worst cases through three LayerNorms and two products and is far
above any measured error (the printed ratios are ~1e-4); it binds for the in_proj outputs, the second condition binds for the rest."""
import functools
import math

import pytest
import torch

from tests import chain_ref as R
from tests.test_gpu_chain_forward import DEV, GUARD_ROWS, NAN_FILL, TAIL, _bits, _ffill, _untouched
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LOG2E = math.log2(math.e)
H = 4


@functools.lru_cache(maxsize=None)
def _layers(d):
    """Two random decoder layers + head (fp32, on the device) with ops.pack_level's keys: in_proj at 0.15, out_proj / linear1 at 0.1,
    linear2 at 0.05, biases and the LayerNorm offsets at 0.1, gains 1 +- 0.1."""
    g = torch.Generator().manual_seed(4000 + d)
    rnd = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(DEV)
    layers = []
    for _ in range(2):
        lay = {"wqkv": rnd(3 * d, d) * 0.15, "bqkv": rnd(3 * d) * 0.1, "wo": rnd(d, d) * 0.1, "bo": rnd(d) * 0.1, "cab": rnd(d) * 0.1,
               "w1": rnd(4 * d, d) * 0.1, "b1": rnd(4 * d) * 0.1, "w2": rnd(d, 4 * d) * 0.05, "b2": rnd(d) * 0.1, "eps": 1e-5}
        for n in ("ln1", "ln2", "ln3"):
            lay[n + "g"], lay[n + "b"] = 1 + rnd(d) * 0.1, rnd(d) * 0.1
        layers.append({k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in lay.items()})
    lvl = {"lnfg": 1 + rnd(d) * 0.1, "lnfb": rnd(d) * 0.1, "lnf_eps": 1e-5}
    return layers, lvl


def _f64(dct):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in dct.items()
            if not (isinstance(k, str) and "image" in k)}


class _Findings:
    """Collects every missed condition of a test so that one run shows them all; check() raises at the end."""

    def __init__(self):
        self.bad = []

    def report(self, label, name, got, ref64, tol, ref32, nact):
        """The two conditions of test_gpu_chain_forward._report for one output tensor."""
        if not bool(torch.isfinite(got).all()):
            self.bad.append(f"{label} {name}: non-finite values")
            return
        err = (got.double() - ref64).abs()
        ratio = float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())
        e, e32 = float(err.max()), float((ref32.double() - ref64).abs().max())
        bound2 = 4 * e32 + R.ACT * nact
        print(f"[agg] {label} {name}: max err {e:.3e} = {ratio:.2e} of its element bound, {e / bound2 if bound2 else float('inf'):.3f} of 4 * err32 ({e32:.3e}) + {nact} ACT")
        if ratio > 1.0:
            self.bad.append(f"{label} {name}: {ratio:.3f} of the per-element bound (max err {e:.3e})")
        if e > bound2:
            self.bad.append(f"{label} {name}: err {e:.3e} > 4 * {e32:.3e} + {nact} * ACT")

    def expect(self, ok, what):
        if not ok:
            self.bad.append(what)

    def check(self):
        assert not self.bad, "\n".join(self.bad)


# ================================================================================================
# paths_token_layer_f32 / paths_token_layer_h3 / paths_token_layer_ws_rows
# ================================================================================================
LAYER_SHAPES = {"65": (65, (64, 65, 1)), "130": (130, (130, 37, 129))}        # (T, valid tokens per slide): both straddle the 64-token tile
LAYER_KERNELS = {"f32": ("paths_token_layer_f32", 128), "h3": ("paths_token_layer_h3", 128), "ws_rows": ("paths_token_layer_ws_rows", 192)}
LAYER_MODES = {"qkv": (0, 1), "post": (1, 0), "both": (1, 1)}                 # (do_post, do_qkv)


@functools.lru_cache(maxsize=None)
def _layer_problem(d, T, lens):
    """x, attn in +-1 (attn: the attention's output enters the layer kernels as an input); references of all three modes for every row
    (the kernels are row-wise: with skip_padding 0 a padded row is computed like any other), float64 with bounds and fp32 torch."""
    B = len(lens)
    g = torch.Generator().manual_seed(31 * T + d)
    x = (torch.rand((B, T, d), generator=g) * 2 - 1).to(DEV)
    attn = (torch.rand((B, T, d), generator=g) * 2 - 1).to(DEV)
    layers, _ = _layers(d)
    pr = {"x": x, "attn": attn, "B": B, "T": T, "d": d, "num_ims": torch.tensor([n - 1 for n in lens], dtype=torch.int64, device=DEV)}
    for tag, cast in (("64", lambda t: t.double()), ("32", lambda t: t)):
        l0, l1 = ({k: (cast(v) if torch.is_tensor(v) else v) for k, v in lay.items() if "image" not in k} for lay in layers)
        xo, txo = R.decoder_post_ref(l0, cast(x), cast(attn), bounds=True)
        pr["x_out" + tag], pr["tol_x_out"] = xo, txo
        pr["qkv_only" + tag] = R.in_proj_ref(l1, cast(x), H)
        pr["qkv_post" + tag] = R.in_proj_ref(l1, xo, H, e_x=txo)
    return pr


def _layer_buffers(kernel, pr):
    B, T, d = pr["B"], pr["T"], pr["d"]
    b = {"x_out": _ffill(B * T + GUARD_ROWS, d)}
    if kernel == "ws_rows":
        b["qkv_rows"] = _ffill(B * T + GUARD_ROWS, 3 * d + 8)
    else:
        for n in "qkv":
            b[n] = _ffill(B * H * T * 32 + TAIL)
    return b


def _layer_call(kernel, pr, bufs, mode, skip, max_tokens=0, **change):
    from paths_amd import _lib, ops
    p = _lib.ptr
    B, T, d = pr["B"], pr["T"], pr["d"]
    post, nxt = _layers(d)[0]
    do_post, do_qkv = LAYER_MODES[mode]
    g = lambda lay, key, on: p(lay[key]) if on else None
    vecs = [g(post, k, do_post) for k in ("bo", "ln1g", "ln1b", "cab", "ln2g", "ln2b")]
    a = dict(x_in=p(pr["x"]), attn=p(pr["attn"]) if do_post else None, x_out=p(bufs["x_out"]) if do_post else None, num_ims=p(pr["num_ims"]),
             B=B, T=T, d=d, H=H, do_post=do_post, do_qkv=do_qkv, skip=skip, qscale=LOG2E / math.sqrt(32), eps=1e-5, max_tokens=max_tokens)
    a.update(change)
    tail = (a["num_ims"], a["B"], a["T"], a["d"])
    if kernel == "f32":
        _lib.call("paths_token_layer_f32", a["x_in"], a["attn"], a["x_out"], g(post, "wo", do_post), vecs[0], vecs[1], vecs[2], vecs[3], vecs[4], vecs[5],
                  g(post, "w1", do_post), g(post, "b1", do_post), g(post, "w2", do_post), g(post, "b2", do_post), g(post, "ln3g", do_post),
                  g(post, "ln3b", do_post), g(nxt, "wqkv", do_qkv), g(nxt, "bqkv", do_qkv), *(p(bufs[n]) if do_qkv else None for n in "qkv"),
                  *tail, a["H"], do_post, do_qkv, a["skip"], a["qscale"], a["eps"], a["max_tokens"], _lib.stream())
        return
    ip, sp, iq, sq = ops.tlayer_operands(post if do_post else None, nxt if do_qkv else None, "h3" if kernel == "h3" else "ws")
    biases = vecs + [g(post, k, do_post) for k in ("b1", "b2", "ln3g", "ln3b")] + [g(nxt, "bqkv", do_qkv)]
    if kernel == "h3":
        _lib.call("paths_token_layer_h3", a["x_in"], a["attn"], a["x_out"], p(ip), p(iq), *biases, sp[0], sp[1], sp[2], sq[0],
                  *(p(bufs[n]) if do_qkv else None for n in "qkv"), *tail, a["H"], do_post, do_qkv, a["skip"], a["qscale"], a["eps"], a["max_tokens"],
                  None, _lib.stream())
    else:
        _lib.call("paths_token_layer_ws_rows", a["x_in"], a["attn"], a["x_out"], p(ip), p(iq), *biases, sp[0], sp[1], sp[2], sq[0],
                  p(bufs["qkv_rows"]) if do_qkv else None, 3 * d + 8 if do_qkv else 0, *tail, do_post, do_qkv, a["skip"], a["eps"], _lib.stream())


def _layer_run(kernel, pr, mode, skip, max_tokens=0):
    bufs = _layer_buffers(kernel, pr)
    _layer_call(kernel, pr, bufs, mode, skip, max_tokens)
    torch.cuda.synchronize()
    return bufs


def _layer_views(kernel, pr, bufs, mode):
    """name -> [B, T, columns] view of what the mode writes, token-major (q, k, v of the f32 / h3 kernels: head-major [B, H, T, 32]
    permuted; of the row form: the three d-wide bands of qkv_rows)."""
    B, T, d = pr["B"], pr["T"], pr["d"]
    do_post, do_qkv = LAYER_MODES[mode]
    v = {}
    if do_post:
        v["x_out"] = bufs["x_out"][:B * T].view(B, T, d)
    if do_qkv:
        for i, n in enumerate("qkv"):
            if kernel == "ws_rows":
                v[n] = bufs["qkv_rows"][:B * T, i * d:(i + 1) * d].reshape(B, T, d)
            else:
                v[n] = bufs[n][:B * H * T * 32].view(B, H, T, 32).transpose(1, 2).reshape(B, T, d)
    return v


def _layer_guards(kernel, pr, bufs, mode, F, label):
    B, T, d = pr["B"], pr["T"], pr["d"]
    do_post, do_qkv = LAYER_MODES[mode]
    F.expect(_untouched(bufs["x_out"][B * T:]) and (do_post or _untouched(bufs["x_out"])), f"{label}: x_out beyond B * T rows (or written without do_post)")
    if kernel == "ws_rows":
        F.expect(_untouched(bufs["qkv_rows"][:, 3 * d:]) and _untouched(bufs["qkv_rows"][B * T:]) and (do_qkv or _untouched(bufs["qkv_rows"])),
                 f"{label}: qkv_rows band behind 3 d / rows beyond B * T")
    else:
        for n in "qkv":
            F.expect(_untouched(bufs[n][B * H * T * 32:]) and (do_qkv or _untouched(bufs[n])), f"{label}: {n} beyond [B, H, T, 32]")


@pytest.mark.parametrize("shape", sorted(LAYER_SHAPES))
@pytest.mark.parametrize("kernel", sorted(LAYER_KERNELS))
def test_token_layer_kernels_match_float64(dev, kernel, shape):
    """do_qkv only, do_post only and both, each with skip_padding 0 and 1, against decoder_post_ref / in_proj_ref on random fp32 x and attn.
    skip_padding 0: every row of every slide is compared (a row-wise kernel computes padded rows like any other).  skip_padding 1: the
    valid rows are bit-identical to the skip_padding 0 run and every other row is that value or still the sentinel - the kernels drop
    whole 64-token tiles behind a slide's last valid token and write partly valid tiles in full; the headers promise neither, so only
    "value or sentinel" is asserted - and both shapes leave at least one tile unwritten.  f32 / h3 write q, k, v head-major
    [B, H, T, 32] with q times qscale; the row form writes [q | k | v] token-major at ld_qkv = 3 d + 8 with q unscaled and leaves the
    band alone.  max_tokens = 1 (f32 / h3): row 0 of every slide is bit-identical to the full run and nothing else is written.
    Measured maxima on an MI355X (max |err|, fraction of the per-element bound, fraction of 4 err32 + n ACT):
      in_proj alone:   f32 q 2.7e-7 .34 .29  k 1.0e-6 .35 .25  v 9.4e-7 .36 .24   h3 q 1.5e-7 .23 .16  k 5.9e-7 .21 .14  v 6.5e-7 .21 .14
                       ws_rows q 1.2e-6 .25 .20  k 8.3e-7 .21 .13  v 9.7e-7 .23 .17
      chain (+ in_proj): x_out f32 1.4e-6 2e-4 .23, h3 1.2e-6 1e-4 .20, ws_rows 1.4e-6 7e-5 .20; q, k, v behind it <= 2.1e-6, 2e-5, .24
    (behind the feed-forward the element bound sums worst cases through three LayerNorms: the second condition binds there)."""
    T, lens = LAYER_SHAPES[shape]
    d = LAYER_KERNELS[kernel][1]
    pr = _layer_problem(d, T, lens)
    B = pr["B"]
    F = _Findings()
    qs = LOG2E / math.sqrt(32) if kernel != "ws_rows" else 1.0
    valid = torch.arange(T, device=DEV)[None, :] <= pr["num_ims"][:, None]                      # [B, T]
    heads = lambda t: t.transpose(1, 2).reshape(B, T, d)                                         # [B, H, T, hd] -> [B, T, d]
    for mode, (do_post, do_qkv) in LAYER_MODES.items():
        label = f"{kernel} T {T} {mode}"
        full = _layer_run(kernel, pr, mode, 0)
        views = _layer_views(kernel, pr, full, mode)
        if do_post:
            F.report(label, "x_out", views["x_out"], pr["x_out64"], pr["tol_x_out"], pr["x_out32"], R.LAYER_ACTIVATIONS["x_out"])
        if do_qkv:
            key = "qkv_post" if do_post else "qkv_only"
            r64, r32 = pr[key + "64"], pr[key + "32"]
            for n in "qkv":
                s = qs if n == "q" else 1.0
                ref = heads(r64[n]) * s
                tol = heads(r64["tol_" + n]) * s + R.U * ref.abs()
                F.report(label, n, views[n], ref, tol, heads(r32[n]) * s, R.LAYER_ACTIVATIONS[n if do_post else n + "_only"])
        _layer_guards(kernel, pr, full, mode, F, label)
        skipped = _layer_run(kernel, pr, mode, 1)
        n_fill = 0
        for name, v1 in _layer_views(kernel, pr, skipped, mode).items():
            a, b = _bits(views[name]), _bits(v1)
            same = a == b
            F.expect(bool(same[valid].all()), f"{label}: {name} of a valid row changed with skip_padding")
            F.expect(bool((same | (b == NAN_FILL))[~valid].all()), f"{label}: {name} of a padded row is neither the value nor the sentinel")
            n_fill += int((b == NAN_FILL)[~valid].sum())
        if kernel != "h3" or T > 128:            # (paths_token_layer_h3's workgroup is 128 tokens: at T = 65 it has one per slide)
            F.expect(n_fill > 0, f"{label}: the short slide was meant to leave a whole tile unwritten")
        _layer_guards(kernel, pr, skipped, mode, F, label + " skip_padding")
        if kernel != "ws_rows" and mode == "both":
            one = _layer_run(kernel, pr, mode, 0, max_tokens=1)
            for name, v1 in _layer_views(kernel, pr, one, mode).items():
                F.expect(torch.equal(_bits(v1[:, 0]), _bits(views[name][:, 0])), f"{label} max_tokens 1: {name} of row 0 differs from the full run")
                F.expect(_untouched(v1[:, 1:]), f"{label} max_tokens 1: {name} written behind row 0")
            _layer_guards(kernel, pr, one, mode, F, label + " max_tokens 1")
    F.check()


def test_token_layer_refusals_launch_nothing(dev):
    from paths_amd import _lib
    for kernel, d in (("f32", 128), ("h3", 128), ("ws_rows", 192)):
        pr = _layer_problem(d, 65, (64, 65, 1))

        def refused(what, mode="both", **change):
            bufs = _layer_buffers(kernel, pr)
            with pytest.raises(_lib.PathsHipError):
                _layer_call(kernel, pr, bufs, mode, 1, **change)
            torch.cuda.synchronize()
            assert all(_untouched(t) for t in bufs.values()), f"{kernel}: {what}"

        refused("a trans_dim the kernel is not built for", d=d + 64)
        refused("skip_padding without num_ims", num_ims=None)
        refused("no input rows", x_in=None)
        refused("do_post without the attention's output", mode="post", attn=None)
        if kernel != "ws_rows":
            refused("a head count other than 4", H=2)


# ================================================================================================
# paths_token0_tail
# ================================================================================================
TAIL_SHAPES = {"300": (300, (300, 37, 1)), "65": (65, (64, 65))}             # 300 keys: several of the 16 key splits hold keys; 37 / 1: most are empty


@functools.lru_cache(maxsize=None)
def _tail_problem(T, lens, head):
    """x in +-1; q, k, v = decoder_layer_ref's float64 in_proj of x rounded to fp32 (q times qscale first): inputs, so the test stands
    apart from the in_proj kernels.  The reference attends with exp2 of the pre-scaled q (qk_scale = ln 2)."""
    d, B = 128, len(lens)
    g = torch.Generator().manual_seed(77 * T + len(head))
    rnd = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(DEV)
    layers, lvl = _layers(d)
    lay = layers[1]
    depth = 2 if head == "concat" else 0
    pr = {"x": rnd(B, T, d), "B": B, "T": T, "depth": depth, "num_ims": torch.tensor([n - 1 for n in lens], dtype=torch.int64, device=DEV),
          "ctx_prev": rnd(B, d + 4) if head == "residual" else None, "ctx_all": rnd(B, depth, d) if depth else None,
          "wcls": (rnd(4, (depth + 1) * d) * 0.1).contiguous(), "bcls": rnd(4) * 0.1}
    r = R.in_proj_ref(_f64(_attn_layer(d)), pr["x"].double(), H)        # (an in_proj at 4 / sqrt(d): logits spread over a few units)
    qs = LOG2E / math.sqrt(32)
    pr["q"], pr["k"], pr["v"] = (r["q"] * qs).float().contiguous(), r["k"].float().contiguous(), r["v"].float().contiguous()
    for tag, cast in (("64", lambda t: t.double()), ("32", lambda t: t)):
        c = lambda t: None if t is None else cast(t)
        l1 = {k: (cast(v) if torch.is_tensor(v) else v) for k, v in lay.items() if "image" not in k}
        lv = {"lnfg": cast(lvl["lnfg"]), "lnfb": cast(lvl["lnfb"]), "lnf_eps": 1e-5, "wcls": cast(pr["wcls"]), "bcls": cast(pr["bcls"])}
        cp = None if pr["ctx_prev"] is None else cast(pr["ctx_prev"][:, :d])
        pr["ref" + tag] = R.token0_tail_ref(l1, lv, cast(pr["x"]), pr["num_ims"], H, cp, c(pr["ctx_all"]),
                                            qkv=(cast(pr["q"]), cast(pr["k"]), cast(pr["v"])), qk_scale=math.log(2.0))
    return pr


def _tail_call(pr, bufs, **change):
    from paths_amd import _lib
    p = _lib.ptr
    layers, lvl = _layers(128)
    w = layers[1]
    a = dict(cls_in=pr["wcls"].shape[1], T=pr["T"], d=128, H=H)
    a.update(change)
    _lib.call("paths_token0_tail", p(pr["x"]), p(pr["q"]), p(pr["k"]), p(pr["v"]), p(pr["num_ims"]), p(w["wo"]), p(w["bo"]), p(w["ln1g"]), p(w["ln1b"]),
              p(w["cab"]), p(w["ln2g"]), p(w["ln2b"]), p(w["w1"]), p(w["b1"]), p(w["w2"]), p(w["b2"]), p(w["ln3g"]), p(w["ln3b"]),
              p(lvl["lnfg"]), p(lvl["lnfb"]), p(pr["ctx_prev"]), 128 + 4 if pr["ctx_prev"] is not None else 0, p(pr["ctx_all"]), pr["depth"],
              p(pr["wcls"]), p(pr["bcls"]), 4, a["cls_in"], p(bufs["ctx_out"]), p(bufs["logits"]), p(bufs["ws"]), pr["B"], a["T"], a["d"], a["H"],
              1e-5, 1e-5, _lib.stream())


def _tail_buffers(pr):
    B = pr["B"]
    return {"ctx_out": _ffill(B * 128 + TAIL), "logits": _ffill(B * 4 + TAIL), "ws": _ffill(B * H * 16 * 36 + TAIL)}


@pytest.mark.parametrize("head", ["residual", "concat"])
@pytest.mark.parametrize("shape", sorted(TAIL_SHAPES))
def test_token0_tail_matches_float64(dev, shape, head):
    """The last layer at token 0 from fp32 q, k, v [B, H, T, 32] (q pre-scaled), decoder.norm, the residual (ctx_prev at stride d + 4)
    or concat (depth 2) context and the classifier against token0_tail_ref; ws_partials starts as NaN (the kernel must write every
    partial it reads) and is not written behind its B * H * 16 * 36 floats.
    Measured maxima on an MI355X (max |err|, fraction of the per-element bound, fraction of 4 err32 + 4 ACT): ctx_out 6.2e-7 6e-7 .16,
    logits 4.6e-7 1e-8 .14 (the element bound passes four LayerNorms: the second condition binds)."""
    T, lens = TAIL_SHAPES[shape]
    pr = _tail_problem(T, lens, head)
    B = pr["B"]
    bufs = _tail_buffers(pr)
    _tail_call(pr, bufs)
    torch.cuda.synchronize()
    F = _Findings()
    (c64, l64, tc, tl), (c32, l32, _, _) = pr["ref64"], pr["ref32"]
    label = f"token0_tail T {T} {head}"
    F.report(label, "ctx_out", bufs["ctx_out"][:B * 128].view(B, 128), c64, tc, c32, R.TAIL_ACTIVATIONS["ctx_out"])
    F.report(label, "logits", bufs["logits"][:B * 4].view(B, 4), l64, tl, l32, R.TAIL_ACTIVATIONS["logits"])
    F.expect(_untouched(bufs["ctx_out"][B * 128:]) and _untouched(bufs["logits"][B * 4:]) and _untouched(bufs["ws"][B * H * 16 * 36:]),
             f"{label}: written beyond ctx_out / logits / ws_partials")
    F.check()


def test_token0_tail_refusals_launch_nothing(dev):
    from paths_amd import _lib
    pr = _tail_problem(65, (64, 65), "concat")
    for what, change in (("cls_in that is not (depth + 1) d", {"cls_in": 128}), ("a trans_dim other than 128", {"d": 192}), ("a head count other than 4", {"H": 2})):
        bufs = _tail_buffers(pr)
        with pytest.raises(_lib.PathsHipError):
            _tail_call(pr, bufs, **change)
        torch.cuda.synchronize()
        assert all(_untouched(t) for t in bufs.values()), what


# ================================================================================================
# paths_attention_h3_any_img
# ================================================================================================
@functools.lru_cache(maxsize=None)
def _attn_layer(d):
    """_layers' first layer with an in_proj at 4 / sqrt(d): attention logits spread over a few units, so a wrong q or k row moves the
    softmax visibly."""
    g = torch.Generator().manual_seed(4100 + d)
    lay = {k: v for k, v in _layers(d)[0][0].items() if "image" not in k}
    lay["wqkv"] = ((torch.rand((3 * d, d), generator=g) * 2 - 1) * (4 / math.sqrt(d))).to(DEV).contiguous()
    return lay


ATTN_IMG_CASES = {"hd48-65": (192, 65, (64, 65, 1)), "hd48-300": (192, 300, (300, 37, 129)), "hd32-130": (128, 130, (130, 37, 129))}


@pytest.mark.parametrize("case", sorted(ATTN_IMG_CASES))
def test_attention_h3_any_img_matches_float64(dev, case):
    """Operand images written by paths_token_layer_ws (do_qkv only: d = 192 / 4 heads = head_dim 48, q scaled there; d = 128 = head_dim
    32, the producer the header names) into a sentinel-filled workspace, then paths_attention_h3_any_img: o against float64
    in_proj + attention on every valid query row, under attention_ref's bound on top of in_proj_ref's and under 4 * err32 + 1 ACT
    (err32 from the same chain in torch fp32 on the device; the one activation stage is the softmax's exponential).
    Padded query rows: the header promises nothing for them (the kernel skips 128-query blocks behind a slide's last valid token and
    computes the rest of a partly valid block from whatever its image rows hold), so they are not looked at; nothing is written
    behind o [B, T, d] or behind paths_attention_h3_any_workspace bytes.
    Measured maxima on an MI355X (max |err|, fraction of the per-element bound, fraction of 4 err32 + 1 ACT): head_dim 48 2.2e-6 .017
    .22, head_dim 32 2.4e-6 .003 .22."""
    from paths_amd import _lib, ops
    d, T, lens = ATTN_IMG_CASES[case]
    B, hd = len(lens), d // H
    g = torch.Generator().manual_seed(5 * T + d)
    x = (torch.rand((B, T, d), generator=g) * 2 - 1).to(DEV)
    lay = _attn_layer(d)
    num_ims = torch.tensor([n - 1 for n in lens], dtype=torch.int64, device=DEV)
    nbytes = int(_lib.load().paths_attention_h3_any_workspace(B, T, H, hd))
    assert d != 128 or nbytes == int(_lib.load().paths_attention_x6_workspace(B, T, H, hd, 2))       # (one layout at head_dim 32)
    ws = _ffill(nbytes // 4 + TAIL)
    qscale = LOG2E / math.sqrt(hd)
    ops.token_layer_ws(x.view(B * T, d), None, None, None, lay, ws, num_ims, B, T, d, H, qscale)
    o = _ffill(B * T * d + TAIL)
    _lib.call("paths_attention_h3_any_img", o.data_ptr(), num_ims.data_ptr(), B, T, H, hd, ws.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    r64 = R.in_proj_ref(_f64(lay), x.double(), H)
    o64, tol = R.attention_ref(r64["q"], r64["k"], r64["v"], num_ims, bounds=True, errs=(r64["tol_q"], r64["tol_k"], r64["tol_v"]))
    r32 = R.in_proj_ref({k: v for k, v in lay.items() if "image" not in k}, x, H)
    o32 = R.attention_ref(r32["q"], r32["k"], r32["v"], num_ims)
    valid = torch.arange(T, device=DEV)[None, :] <= num_ims[:, None]
    got = o[:B * T * d].view(B, T, d)
    F = _Findings()
    F.report(f"attention_h3_any_img {case}", "o", got[valid], o64[valid], tol[valid], o32[valid], R.ATTN_ACTIVATIONS["o"])
    F.expect(_untouched(o[B * T * d:]), f"{case}: o written behind [B, T, d]")
    F.expect(_untouched(ws[nbytes // 4:]), f"{case}: workspace written behind paths_attention_h3_any_workspace bytes")
    F.check()
