"""The special token's attention export (csrc/attn_token0.hip: paths_token0_attention) against float64 restatements: the kernel on
identical fp32 inputs, the drop-in PATHSProcessor.process(return_attention=True) on the goldens' inputs and the device recursion
(utils.recurse(attention=True)) against the oracle's own token sequences; and the export leaves every other output bit-identical."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.helpers import build_model
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ATT_TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    from paths_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


SMALL = {"num_levels": 3, "top_k_patches": [16, 16]}           # the smoke() case


# ------------------------------------------------------------------------------------------------
# float64 restatements
# ------------------------------------------------------------------------------------------------
def ref_attention(x, num_ims, w_in, b_in, nhead, special_last):
    """nn.MultiheadAttention's weights of the special token in float64 (full K projection, bias included): x [B, T, d] ->
    patch [B, H, T-1] (0 on padding), self [B, H]."""
    x = np.asarray(x, np.float64)
    w_in, b_in = np.asarray(w_in, np.float64), np.asarray(b_in, np.float64)
    B, T, d = x.shape
    hd = d // nhead
    patch = np.zeros((B, nhead, T - 1))
    self_ = np.zeros((B, nhead))
    for b in range(B):
        n = int(min(max(int(num_ims[b]), 0), T - 1))
        rows = x[b, : n + 1]
        xs = rows[n] if special_last else rows[0]
        q = w_in[:d] @ xs + b_in[:d]
        k = rows @ w_in[d:2 * d].T + b_in[d:2 * d]                          # [n + 1, d]
        for h in range(nhead):
            s = k[:, h * hd:(h + 1) * hd] @ q[h * hd:(h + 1) * hd] / math.sqrt(hd)
            p = np.exp(s - s.max())
            p /= p.sum()
            if special_last:
                patch[b, h, :n], self_[b, h] = p[:n], p[n]
            else:
                patch[b, h, :n], self_[b, h] = p[1:], p[0]
    return patch, self_


def decoder_attention64(p, prefix, S, num_ims, nhead, layers, eps=1e-5):
    """The oracle's post-LN decoder stack (oracle/paths_oracle.py:decoder_stack) in float64 on S [B, T, d] (special token first),
    returning the special token's attention of every layer: ([B, L, H, T-1], [B, L, H])."""
    S = S.double()
    B, T, d = S.shape
    hd = d // nhead
    key_pad = torch.arange(T)[None, :] >= (num_ims + 1)[:, None]
    att, att_self = [], []
    g = lambda name: p[prefix + name].double()
    ln = lambda v, w, bb: torch.nn.functional.layer_norm(v, (d,), w, bb, eps)
    for l in range(layers):
        q_ = f"decoder.layers.{l}."
        qkv = S @ g(q_ + "self_attn.in_proj_weight").T + g(q_ + "self_attn.in_proj_bias")
        q, k, v = (t.reshape(B, T, nhead, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        sc = sc.masked_fill(key_pad[:, None, None, :], float("-inf"))
        a = torch.softmax(sc, dim=-1)                                       # [B, H, T, T]
        att.append(torch.where(key_pad[:, None, 1:], 0.0, a[:, :, 0, 1:]))
        att_self.append(a[:, :, 0, 0])
        o = (a @ v).transpose(1, 2).reshape(B, T, d) @ g(q_ + "self_attn.out_proj.weight").T + g(q_ + "self_attn.out_proj.bias")
        S = ln(S + o, g(q_ + "norm1.weight"), g(q_ + "norm1.bias"))
        S = ln(S + g(q_ + "multihead_attn.out_proj.bias"), g(q_ + "norm2.weight"), g(q_ + "norm2.bias"))
        ff = torch.relu(S @ g(q_ + "linear1.weight").T + g(q_ + "linear1.bias")) @ g(q_ + "linear2.weight").T + g(q_ + "linear2.bias")
        S = ln(S + ff, g(q_ + "norm3.weight"), g(q_ + "norm3.bias"))
    return torch.stack(att, 1), torch.stack(att_self, 1)


def oracle_level_attention(params, depth, xs, num_ims, nhead, layers):
    pre = f"procs.{depth}.global_agg."
    B = xs.shape[0]
    S = torch.cat((params[pre + "special_token"].view(1, 1, -1).repeat(B, 1, 1), xs), dim=1)
    return decoder_attention64(params, pre + "transformer.", S, num_ims, nhead, layers)


# ------------------------------------------------------------------------------------------------
# 1. the kernel
# ------------------------------------------------------------------------------------------------
def run_kernel(dev, x, num_ims, w_in, b_in, nhead, special_last):
    from paths_amd import _lib
    B, T, d = x.shape
    N = T - 1
    patch = torch.full((B, nhead, N), float("nan"), device=dev)
    self_ = torch.full((B, nhead), float("nan"), device=dev)
    ws = torch.empty((int(_lib.load().paths_token0_attention_workspace(B, T, d, nhead)),), device=dev)
    _lib.call("paths_token0_attention", _lib.ptr(x), _lib.ptr(num_ims), _lib.ptr(w_in), _lib.ptr(b_in), _lib.ptr(patch) if N else None,
              nhead * N, _lib.ptr(self_), nhead, _lib.ptr(ws), B, T, d, nhead, special_last, _lib.stream())
    torch.cuda.synchronize()
    return patch.cpu(), self_.cpu()


GEOMS = [(128, 4), (192, 4), (160, 4), (96, 4), (320, 4), (64, 2), (1536, 4), (1536, 24)]
CASES = [(d, h, T) for d, h in GEOMS for T in (1, 2, 65, 300, 2049)] + [(1536, 4, 8193)]


@pytest.mark.parametrize("d,nhead,T", CASES)
def test_kernel_vs_float64(dev, d, nhead, T):
    gen = torch.Generator().manual_seed(d * 100003 + nhead * 101 + T)
    B = 4
    x = torch.randn((B, T, d), generator=gen)
    w_in = torch.randn((3 * d, d), generator=gen) * (1.5 / math.sqrt(d))
    b_in = torch.randn((3 * d,), generator=gen) * 0.5
    num_ims = torch.tensor([T - 1, 0, (T - 1) // 2, max(T - 3, 0)], dtype=torch.int64)
    tol = 1e-5 if d == 1536 else 2e-6
    for special_last in (0, 1):
        xp = x.clone()
        for b in range(B):                         # padding rows hold NaN: the kernel must never read them
            xp[b, int(num_ims[b]) + 1:] = float("nan")
        xd, nd, wd, bd = xp.to(dev), num_ims.to(dev), w_in.to(dev), b_in.to(dev)
        patch, self_ = run_kernel(dev, xd, nd, wd, bd, nhead, special_last)
        rp, rs = ref_attention(xp.numpy(), num_ims.numpy(), w_in.numpy(), b_in.numpy(), nhead, special_last)
        assert torch.isfinite(patch).all() and torch.isfinite(self_).all()
        assert np.abs(patch.numpy() - rp).max(initial=0.0) <= tol and np.abs(self_.numpy() - rs).max() <= tol
        for b in range(B):
            assert (patch[b, :, int(num_ims[b]):] == 0).all()                      # padding exactly 0
        tot = patch.double().sum(-1) + self_.double()
        assert (tot - 1).abs().max() <= 1e-5
        assert (self_[1] == 1).all()                                               # num_ims = 0: all weight on itself
        p2, s2 = run_kernel(dev, xd, nd, wd, bd, nhead, special_last)              # deterministic
        assert torch.equal(patch, p2) and torch.equal(self_, s2)


def test_kernel_clamps_num_ims(dev):
    """num_ims outside [0, T-1] is clamped on the device (no read past the slide's rows)."""
    gen = torch.Generator().manual_seed(7)
    B, T, d, nh = 2, 65, 128, 4
    x = torch.randn((B, T, d), generator=gen)
    w_in = torch.randn((3 * d, d), generator=gen) / math.sqrt(d)
    b_in = torch.zeros((3 * d,))
    got = run_kernel(dev, x.to(dev), torch.tensor([1000, -5], device=dev), w_in.to(dev), b_in.to(dev), nh, 0)
    want = run_kernel(dev, x.to(dev), torch.tensor([T - 1, 0], device=dev), w_in.to(dev), b_in.to(dev), nh, 0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------
# 2. drop-in PATHSProcessor.process(return_attention=True)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1_level0_b2_k256", "g2_level2_b2_k256", "g12_td192_level1", "g15_td160_h4_hd40_level1"])
def test_drop_in_attention_vs_float64(dev, name):
    from oracle import paths_oracle as orc
    from paths_amd.data_utils.patch_batch import PatchBatch
    g, info = load_golden(name)
    cfg, model, params = build_model(dev, info["wseed"], info["cfg_over"])
    ocfg = H.oracle_config(info["cfg_over"])
    inp = H.single_level_inputs(info, ocfg)
    pb = PatchBatch(**{k: torch.from_numpy(v).to(dev) for k, v in inp.items()})
    depth = info["depth"]
    with torch.no_grad():
        plain = {k: v.cpu() for k, v in model(depth, pb).items()}
        out = {k: v.cpu() for k, v in model(depth, pb, return_attention=True).items()}
    assert set(plain) == {"logits", "ctx_slide", "ctx_patch", "importance"}
    assert set(out) == set(plain) | {"attention", "attention_self"}
    for k in plain:
        assert torch.equal(plain[k], out[k]), k
    mc = cfg.model_config
    B, N = inp["fts"].shape[:2]
    assert out["attention"].shape == (B, mc.trans_layers, mc.trans_heads, N) and out["attention_self"].shape == (B, mc.trans_layers, mc.trans_heads)
    probe = {}
    ti = {k: torch.from_numpy(v) for k, v in inp.items()}
    orc.process_level(params, ocfg, depth, ti["fts"], ti["locs"], ti["num_ims"], ti["ctx_slide"], ti["ctx_patch"], probe=probe)
    ra, rs = oracle_level_attention(params, depth, probe["xs"], ti["num_ims"], mc.trans_heads, mc.trans_layers)
    assert (out["attention"].double() - ra).abs().max() <= ATT_TOL
    assert (out["attention_self"].double() - rs).abs().max() <= ATT_TOL
    for b, n in enumerate(info["num_ims"]):
        assert (out["attention"][b, :, :, n:] == 0).all()
    with pytest.raises(NotImplementedError):
        model(depth, pb, return_attention=True)                # grad enabled: not a training path


# ------------------------------------------------------------------------------------------------
# 3. the device recursion
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [SMALL, dict(SMALL, model_config={"trans_dim": 192})])
def test_recursion_attention_vs_float64(dev, monkeypatch, over):
    """The smoke() case (3 levels, B = 2, 8 x 8 base grid, top-k 16), default geometry and trans_dim 192, against float64 attention
    of the oracle's own token sequences; rows matched by location (kept order may differ at exact ties)."""
    from oracle import paths_oracle as orc
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    cfg, model, params = build_model(dev, 5, over)
    ocfg = H.oracle_config(over)
    slides = [DeviceSlide.synthetic(21, s, (8, 8), num_levels=3, device=dev) for s in range(2)]
    probes = []
    orig = orc.process_level

    def spy(p, c, depth, fts, locs, num_ims, ctx_slide, ctx_patch, probe=None):
        pr = {}
        res = orig(p, c, depth, fts, locs, num_ims, ctx_slide, ctx_patch, probe=pr)
        probes.append((depth, pr["xs"], num_ims.clone(), locs.clone()))
        return res

    monkeypatch.setattr(orc, "process_level", spy)
    trace = []
    with torch.no_grad():
        putils.recurse(model, slides, cfg.top_k_patches, 3, trace=trace, attention=True)
        orc.inference_end2end(params, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], None, [])
    mc = cfg.model_config
    assert len(probes) == 3
    for depth, xs, nim, locs in probes:
        ra, rs = oracle_level_attention(params, depth, xs, nim, mc.trans_heads, mc.trans_layers)
        rec = trace[depth]
        att, att_self = rec["attention"].cpu().double(), rec["attention_self"].cpu().double()
        glocs = rec["locs"].cpu()
        for b in range(2):
            n = int(nim[b])
            assert int(rec["num_ims"][b]) == n
            where = {tuple(r): i for i, r in enumerate(glocs[b, :n].tolist())}
            idx = torch.tensor([where[tuple(r)] for r in locs[b, :n].tolist()], dtype=torch.long)
            assert (att[b, :, :, idx] - ra[b, :, :, :n]).abs().max() <= ATT_TOL
            assert (att_self[b] - rs[b]).abs().max() <= ATT_TOL
            assert (att[b, :, :, n:] == 0).all()


def _headline(dev):
    from paths_amd.data_utils.slide import DeviceSlide
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[512] * 4)
    slides = [DeviceSlide.synthetic(1234, sid, (32, 64), device=dev) for sid in [10003, 10004, 10005, 10006, 10007, 10008, 10011, 10014]]
    return cfg, model, slides


def test_headline_recursion_attention_changes_nothing_else(dev):
    """K = 2048 x 8 slides x 5 levels (the benchmark's shape): with attention=True every trace field and output is bit-identical to
    attention=False, and each exported row is a probability distribution; without the flag the export is never launched."""
    from paths_amd import utils as putils
    from tests.helpers import spy_calls
    cfg, model, slides = _headline(dev)
    tr0, tr1 = [], []
    with torch.no_grad():
        with spy_calls() as calls:
            out0 = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=tr0)
        assert "paths_token0_attention" not in calls
        with spy_calls() as calls:
            out1 = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=tr1, attention=True)
        assert calls.count("paths_token0_attention") == 5 * cfg.model_config.trans_layers
    torch.cuda.synchronize()
    nim = tr0[-1]["num_ims"].cpu()
    for k in out0:
        if k == "ctx_patch":           # (padding rows of the state are never written by the recursion: compare the slides' rows)
            for b in range(len(slides)):
                assert torch.equal(out0[k][b, : int(nim[b])], out1[k][b, : int(nim[b])]), k
            continue
        assert torch.equal(out0[k], out1[k]), k
    for r0, r1 in zip(tr0, tr1):
        assert set(r1) == set(r0) | {"attention", "attention_self"}
        rows = {"locs": r0["num_ims"], "parent_inds": r0["num_ims"], "keep_idx": r0.get("keep_count")}
        for k in r0:
            if k in rows:              # (defined entries only: rows past a slide's count are scratch)
                for b in range(len(slides)):
                    c = int(rows[k][b])
                    assert torch.equal(r0[k][b, :c], r1[k][b, :c]), k
                continue
            assert torch.equal(r0[k], r1[k]), k
        tot = r1["attention"].double().sum(-1) + r1["attention_self"].double()
        assert (tot - 1).abs().max() <= 1e-5
        n = r1["num_ims"].cpu()
        att = r1["attention"].cpu()
        for b in range(len(slides)):
            assert (att[b, :, :, int(n[b]):] == 0).all() and (att[b, :, :, : int(n[b])] >= 0).all()


def test_recursion_attention_token_orders_agree(dev, monkeypatch):
    """The default form (FUSE_QKV 2: tokens in the fused finish's order, the special token last) and the reference-order form
    (FUSE_QKV 0) export the same attention."""
    import paths_amd.ops as ops
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    from tests.helpers import spy_calls
    cfg, model, _ = build_model(dev, 5, SMALL)
    slides = [DeviceSlide.synthetic(21, s, (8, 8), num_levels=3, device=dev) for s in range(2)]
    traces = {}
    for mode in (2, 0):
        monkeypatch.setattr(ops, "FUSE_QKV", mode)
        tr = []
        with torch.no_grad(), spy_calls() as calls:
            putils.recurse(model, slides, cfg.top_k_patches, 3, trace=tr, attention=True)
        assert ("paths_importance_qkv_x6" in calls) == (mode == 2)
        traces[mode] = tr
    for a, b in zip(traces[2], traces[0]):
        assert torch.equal(a["locs"], b["locs"]) and torch.equal(a["num_ims"], b["num_ims"])
        assert (a["attention"] - b["attention"]).abs().max() <= 1e-6
        assert (a["attention_self"] - b["attention_self"]).abs().max() <= 1e-6
