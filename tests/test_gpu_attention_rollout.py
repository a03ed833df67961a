"""The special token's attention rollout (csrc/attn_rollout.hip) against float64 restatements (tests/rollout_ref.py): prepare + step on
identical fp32 inputs, the drop-in PATHSProcessor.process(return_rollout=True) and the device recursion (utils.recurse(rollout=True))
against the oracle's own token sequences; and the rollout leaves every other output bit-identical."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.helpers import build_model
from tests import rollout_ref as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ROLL_TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    from paths_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


SMALL = {"num_levels": 3, "top_k_patches": [16, 16]}           # the smoke() case


# ------------------------------------------------------------------------------------------------
# 1. the kernels: prepare + step on identical fp32 inputs
# ------------------------------------------------------------------------------------------------
def run_step(dev, x, num_ims, w_in, b_in, nhead, special_last, r_in, outputs=False):
    """prepare(x) then one step of r_in [B, T] (canonical rows): r_out [B, T], or with ``outputs`` the rollout pair ([B, T-1], [B])."""
    from paths_amd import _lib
    B, T, d = x.shape
    ws = torch.full((int(_lib.load().paths_attention_rollout_workspace(B, T, d, nhead)),), float("nan"), device=dev)
    st = _lib.stream()
    _lib.call("paths_attention_rollout_prepare", _lib.ptr(x), _lib.ptr(num_ims), _lib.ptr(w_in), _lib.ptr(b_in), _lib.ptr(ws), B, T, d,
              nhead, special_last, st)
    if outputs:
        roll = torch.full((B, T - 1), float("nan"), device=dev)
        self_ = torch.full((B,), float("nan"), device=dev)
        _lib.call("paths_attention_rollout_step", _lib.ptr(ws), _lib.ptr(num_ims), _lib.ptr(r_in), None, _lib.ptr(roll) if T > 1 else None,
                  T - 1, _lib.ptr(self_), B, T, d, nhead, st)
        torch.cuda.synchronize()
        return roll.cpu(), self_.cpu()
    r_out = torch.full((B, T), float("nan"), device=dev)
    _lib.call("paths_attention_rollout_step", _lib.ptr(ws), _lib.ptr(num_ims), _lib.ptr(r_in), _lib.ptr(r_out), None, 0, None, B, T, d,
              nhead, st)
    torch.cuda.synchronize()
    return r_out.cpu()


GEOMS = [(128, 4), (192, 4), (160, 4), (96, 4), (320, 4), (64, 2), (1536, 4), (1536, 24), (128, 8)]
CASES = [(d, h, T) for d, h in GEOMS for T in (1, 2, 65, 300, 2049)] + [(1536, 4, 8193)]


def _inputs(d, nhead, T, B=4):
    gen = torch.Generator().manual_seed(d * 100003 + nhead * 101 + T)
    x = torch.randn((B, T, d), generator=gen)
    w_in = torch.randn((3 * d, d), generator=gen) * (1.5 / math.sqrt(d))
    b_in = torch.randn((3 * d,), generator=gen) * 0.5
    num_ims = torch.tensor([T - 1, 0, (T - 1) // 2, max(T - 3, 0)][:B], dtype=torch.int64)
    r_in = torch.rand((B, T), generator=gen)
    for b in range(B):
        r_in[b, int(num_ims[b]) + 1:] = 0.0
    return x, w_in, b_in, num_ims, r_in


@pytest.mark.parametrize("d,nhead,T", CASES)
def test_kernel_step_vs_float64(dev, d, nhead, T):
    x, w_in, b_in, num_ims, r_in = _inputs(d, nhead, T)
    B = x.shape[0]
    tol = 1e-5 if d == 1536 else 2e-6
    for special_last in (0, 1):
        xp = x.clone()
        for b in range(B):                         # padding rows hold NaN: the kernels must never read them
            xp[b, int(num_ims[b]) + 1:] = float("nan")
        xd, nd, wd, bd, rd = xp.to(dev), num_ims.to(dev), w_in.to(dev), b_in.to(dev), r_in.to(dev)
        got = run_step(dev, xd, nd, wd, bd, nhead, special_last, rd)
        want = R.step64(xp, num_ims, w_in, b_in, nhead, special_last, r_in)
        assert torch.isfinite(got).all()
        assert (got.double() - want).abs().max() <= tol
        for b in range(B):
            assert (got[b, int(num_ims[b]) + 1:] == 0).all()                       # rows past num_ims exactly 0
        # mass is kept: every row of P sums to 1, so sum(r_out) = sum(r_in)
        assert (got.double().sum(1) - r_in.double().sum(1)).abs().max() <= 1e-5 * max(1.0, float(r_in.sum(1).max()))
        again = run_step(dev, xd, nd, wd, bd, nhead, special_last, rd)             # deterministic
        assert torch.equal(got, again)
        roll, self_ = run_step(dev, xd, nd, wd, bd, nhead, special_last, rd, outputs=True)
        assert torch.equal(self_, got[:, 0]) and torch.equal(roll, got[:, 1:])      # output form: patch j = canonical row 1 + j


def test_kernel_clamps_num_ims(dev):
    """num_ims outside [0, T-1] is clamped on the device (no read past the slide's rows)."""
    x, w_in, b_in, _, r_in = _inputs(128, 4, 65, B=2)
    args = (x.to(dev), None, w_in.to(dev), b_in.to(dev), 4, 0)
    r_in[1, 1:] = 0.0
    got = run_step(dev, args[0], torch.tensor([1000, -5], device=dev), *args[2:], r_in.to(dev))
    want = run_step(dev, args[0], torch.tensor([64, 0], device=dev), *args[2:], r_in.to(dev))
    assert torch.equal(got, want) and torch.isfinite(got).all()
    assert float(got[1, 0]) == float(r_in[1, 0])                 # one token: A = [[1]]


def test_kernel_seed(dev):
    """seed: r = 0.5 e_s + 0.5 mean_h(a) from paths_token0_attention's layout (a slot of [B, L, H, N] / [B, L, H])."""
    from paths_amd import _lib
    B, L, nh, T = 3, 2, 4, 70
    N = T - 1
    num_ims = torch.tensor([N, 5, 0])
    gen = torch.Generator().manual_seed(5)
    patch = torch.rand((B, L, nh, N), generator=gen)
    self_ = torch.rand((B, L, nh), generator=gen)
    pd, sd, nd = patch.to(dev), self_.to(dev), num_ims.to(dev)
    r = torch.full((B, T), float("nan"), device=dev)
    roll = torch.full((B, N), float("nan"), device=dev)
    rs = torch.full((B,), float("nan"), device=dev)
    _lib.call("paths_attention_rollout_seed", pd.data_ptr() + 4 * nh * N, L * nh * N, sd.data_ptr() + 4 * nh, L * nh, _lib.ptr(nd), _lib.ptr(r),
              None, 0, None, B, T, nh, _lib.stream())
    _lib.call("paths_attention_rollout_seed", pd.data_ptr() + 4 * nh * N, L * nh * N, sd.data_ptr() + 4 * nh, L * nh, _lib.ptr(nd), None,
              _lib.ptr(roll), N, _lib.ptr(rs), B, T, nh, _lib.stream())
    torch.cuda.synchronize()
    r, roll, rs = r.cpu(), roll.cpu(), rs.cpu()
    want = torch.zeros((B, T), dtype=torch.float64)
    for b in range(B):
        n = int(num_ims[b])
        want[b, 0] = 0.5 + 0.5 * self_[b, 1].double().mean()
        want[b, 1:n + 1] = 0.5 * patch[b, 1, :, :n].double().mean(0)
    assert (r.double() - want).abs().max() <= 1e-7
    assert torch.equal(roll, r[:, 1:]) and torch.equal(rs, r[:, 0])


# ------------------------------------------------------------------------------------------------
# 2. drop-in PATHSProcessor.process(return_rollout=True)
# ------------------------------------------------------------------------------------------------
def _drop_in(dev, info, cfg, model, params):
    from oracle import paths_oracle as orc
    from paths_amd.data_utils.patch_batch import PatchBatch
    ocfg = H.oracle_config(info["cfg_over"])
    inp = H.single_level_inputs(info, ocfg)
    pb = PatchBatch(**{k: torch.from_numpy(v).to(dev) for k, v in inp.items()})
    depth = info["depth"]
    with torch.no_grad():
        plain = {k: v.cpu() for k, v in model(depth, pb).items()}
        out = {k: v.cpu() for k, v in model(depth, pb, return_rollout=True).items()}
        both = {k: v.cpu() for k, v in model(depth, pb, return_rollout=True, return_attention=True).items()}
    assert set(plain) == {"logits", "ctx_slide", "ctx_patch", "importance"}
    assert set(out) == set(plain) | {"rollout", "rollout_self"}
    assert set(both) == set(out) | {"attention", "attention_self"}
    for k in plain:
        assert torch.equal(plain[k], out[k]) and torch.equal(plain[k], both[k]), k
    assert torch.equal(out["rollout"], both["rollout"]) and torch.equal(out["rollout_self"], both["rollout_self"])
    mc = cfg.model_config
    B, N = inp["fts"].shape[:2]
    assert out["rollout"].shape == (B, N) and out["rollout_self"].shape == (B,)
    probe = {}
    ti = {k: torch.from_numpy(v) for k, v in inp.items()}
    orc.process_level(params, ocfg, depth, ti["fts"], ti["locs"], ti["num_ims"], ti["ctx_slide"], ti["ctx_patch"], probe=probe)
    rr, rs = R.oracle_level_rollout(params, depth, probe["xs"], ti["num_ims"], mc.trans_heads, mc.trans_layers)
    assert (out["rollout"].double() - rr).abs().max() <= ROLL_TOL
    assert (out["rollout_self"].double() - rs).abs().max() <= ROLL_TOL
    for b in range(B):
        assert (out["rollout"][b, int(ti["num_ims"][b]):] == 0).all()
    with pytest.raises(NotImplementedError):
        model(depth, pb, return_rollout=True)                  # grad enabled: not a training path


@pytest.mark.parametrize("name", ["g1_level0_b2_k256", "g2_level2_b2_k256", "g12_td192_level1", "g15_td160_h4_hd40_level1",
                                  "g12_td64_h2_l3_level1"])
def test_drop_in_rollout_vs_float64(dev, name):
    g, info = load_golden(name)
    cfg, model, params = build_model(dev, info["wseed"], info["cfg_over"])
    _drop_in(dev, info, cfg, model, params)


def test_drop_in_rollout_one_layer(dev):
    """trans_layers = 1: the rollout is 0.5 e_s + 0.5 mean_h of the only layer's token-0 attention (no full-matrix step)."""
    g, info = load_golden("g1_level0_b2_k256")
    info = dict(info)
    over = dict(info["cfg_over"] or {})
    over["model_config"] = dict(over.get("model_config", {}), trans_layers=1)
    info["cfg_over"] = over
    cfg, model, params = build_model(dev, info["wseed"], over)
    assert cfg.model_config.trans_layers == 1
    _drop_in(dev, info, cfg, model, params)


# ------------------------------------------------------------------------------------------------
# 3. the device recursion
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [SMALL, dict(SMALL, model_config={"trans_dim": 192})])
def test_recursion_rollout_vs_float64(dev, monkeypatch, over):
    """The smoke() case (3 levels, B = 2, 8 x 8 base grid, top-k 16), default geometry and trans_dim 192, against the float64 rollout
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
        putils.recurse(model, slides, cfg.top_k_patches, 3, trace=trace, rollout=True)
        orc.inference_end2end(params, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], None, [])
    mc = cfg.model_config
    assert len(probes) == 3
    for depth, xs, nim, locs in probes:
        rr, rs = R.oracle_level_rollout(params, depth, xs, nim, mc.trans_heads, mc.trans_layers)
        rec = trace[depth]
        assert "attention" not in rec
        roll, roll_self = rec["rollout"].cpu().double(), rec["rollout_self"].cpu().double()
        glocs = rec["locs"].cpu()
        for b in range(2):
            n = int(nim[b])
            assert int(rec["num_ims"][b]) == n
            where = {tuple(r): i for i, r in enumerate(glocs[b, :n].tolist())}
            idx = torch.tensor([where[tuple(r)] for r in locs[b, :n].tolist()], dtype=torch.long)
            assert (roll[b, idx] - rr[b, :n]).abs().max() <= ROLL_TOL
            assert abs(float(roll_self[b]) - float(rs[b])) <= ROLL_TOL
            assert (roll[b, n:] == 0).all()


def _headline(dev):
    from paths_amd.data_utils.slide import DeviceSlide
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[512] * 4)
    slides = [DeviceSlide.synthetic(1234, sid, (32, 64), device=dev) for sid in [10003, 10004, 10005, 10006, 10007, 10008, 10011, 10014]]
    return cfg, model, slides


ROLLOUT_CALLS = ("paths_attention_rollout_prepare", "paths_attention_rollout_seed", "paths_attention_rollout_step")


def _same_records(r0, r1, nslides):
    rows = {"locs": r0["num_ims"], "parent_inds": r0["num_ims"], "keep_idx": r0.get("keep_count")}
    for k in r0:
        if k in rows:                  # (defined entries only: rows past a slide's count are scratch)
            for b in range(nslides):
                c = int(rows[k][b])
                assert torch.equal(r0[k][b, :c], r1[k][b, :c]), k
            continue
        assert torch.equal(r0[k], r1[k]), k


def test_headline_recursion_rollout_changes_nothing_else(dev):
    """K = 2048 x 8 slides x 5 levels (the benchmark's shape): with rollout=True every trace field and output is bit-identical to a run
    without it and to a run with attention=True; each rollout row is a distribution; without the flag no rollout kernel is launched."""
    from paths_amd import utils as putils
    from tests.helpers import spy_calls
    cfg, model, slides = _headline(dev)
    L = cfg.model_config.trans_layers
    tr0, tr1, tr2 = [], [], []
    with torch.no_grad():
        with spy_calls() as calls:
            out0 = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=tr0)
        assert not any(c in calls for c in ROLLOUT_CALLS)
        with spy_calls() as calls:
            out2 = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=tr2, attention=True)
        assert not any(c in calls for c in ROLLOUT_CALLS)
        with spy_calls() as calls:
            out1 = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=tr1, rollout=True)
        assert calls.count("paths_attention_rollout_prepare") == 5 * (L - 1)
        assert calls.count("paths_attention_rollout_step") == 5 * (L - 1)
        assert calls.count("paths_attention_rollout_seed") == 5
        tr3 = []
        out3 = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=tr3, rollout=True, attention=True)
    torch.cuda.synchronize()
    nim = tr0[-1]["num_ims"].cpu()
    for other in (out1, out2, out3):
        for k in out0:
            if k == "ctx_patch":       # (padding rows of the state are never written by the recursion: compare the slides' rows)
                for b in range(len(slides)):
                    assert torch.equal(out0[k][b, : int(nim[b])], other[k][b, : int(nim[b])]), k
                continue
            assert torch.equal(out0[k], other[k]), k
    for r0, r1, r2, r3 in zip(tr0, tr1, tr2, tr3):
        assert set(r1) == set(r0) | {"rollout", "rollout_self"}
        assert set(r3) == set(r2) | {"rollout", "rollout_self"}
        _same_records(r0, {k: r1[k] for k in r0}, len(slides))
        _same_records(r2, {k: r3[k] for k in r2}, len(slides))
        assert torch.equal(r1["rollout"], r3["rollout"]) and torch.equal(r1["rollout_self"], r3["rollout_self"])
        roll, roll_self, n = r1["rollout"].cpu(), r1["rollout_self"].cpu(), r1["num_ims"].cpu()
        assert ((roll.double().sum(-1) + roll_self.double()) - 1).abs().max() <= 1e-5
        assert (roll >= 0).all() and (roll_self >= 0).all()
        for b in range(len(slides)):
            assert (roll[b, int(n[b]):] == 0).all()


def test_recursion_rollout_token_orders_agree(dev, monkeypatch):
    """The default form (FUSE_QKV 2: tokens in the fused finish's order, the special token last) and the reference-order form
    (FUSE_QKV 0) give the same rollout."""
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
            putils.recurse(model, slides, cfg.top_k_patches, 3, trace=tr, rollout=True)
        assert ("paths_importance_qkv_x6" in calls) == (mode == 2)
        traces[mode] = tr
    for a, b in zip(traces[2], traces[0]):
        assert torch.equal(a["locs"], b["locs"]) and torch.equal(a["num_ims"], b["num_ims"])
        assert (a["rollout"] - b["rollout"]).abs().max() <= 1e-6
        assert (a["rollout_self"] - b["rollout_self"]).abs().max() <= 1e-6


def test_headline_rollout_values_match_serial_and_standalone(dev, monkeypatch):
    """At the headline shape the rollout's VALUES (not only its sums and signs) are checked: two warm recursions with the aggregator
    on its own stream, overlapping the selection chain, must equal bit for bit a recursion with the aggregator serialised behind it;
    and that serialised rollout must equal prepare + seed + step run standalone on the same layer inputs.  Corrupted Q / K would
    leave every row of P summing to 1, so only a value comparison catches it."""
    import paths_amd.ops as ops
    from paths_amd import _lib
    from paths_amd import utils as putils
    cfg, model, slides = _headline(dev)
    mc = cfg.model_config
    L, nh = mc.trans_layers, mc.trans_heads
    assert L == 2

    def run(**kw):
        tr = []
        with torch.no_grad():
            putils.recurse(model, slides, cfg.top_k_patches, 5, trace=tr, rollout=True, **kw)
        torch.cuda.synchronize()
        return tr

    run()                                                     # warm: packs, images, allocator (later runs overlap fully)
    overlapped = [run(), run()]
    captured = []
    orig = ops._Rollout.layer

    def spy(self, l, x, special_last):
        if l == 0:
            captured.append((x.detach().clone(), self.num_ims.clone(), self.lvl_pack["layers"][0], special_last))
        return orig(self, l, x, special_last)

    monkeypatch.setattr(putils, "OVERLAP_AGGREGATOR", False)
    monkeypatch.setattr(ops._Rollout, "layer", spy)
    serial = run(attention=True)
    assert len(captured) == 5
    for lvl in range(5):
        for tr in overlapped:
            assert torch.equal(tr[lvl]["rollout"], serial[lvl]["rollout"]), lvl
            assert torch.equal(tr[lvl]["rollout_self"], serial[lvl]["rollout_self"]), lvl
        x, num_ims, lay, sl = captured[lvl]
        B, T, d = x.shape
        N = T - 1
        ws = torch.empty((int(_lib.load().paths_attention_rollout_workspace(B, T, d, nh)),), device=dev)
        r = torch.empty((B, T), device=dev)
        roll, roll_self = torch.empty((B, N), device=dev), torch.empty((B,), device=dev)
        att, att_self = serial[lvl]["attention"], serial[lvl]["attention_self"]
        st = _lib.stream()
        _lib.call("paths_attention_rollout_prepare", _lib.ptr(x), _lib.ptr(num_ims), _lib.ptr(lay["w_in"]), _lib.ptr(lay["b_in"]), _lib.ptr(ws),
                  B, T, d, nh, sl, st)
        _lib.call("paths_attention_rollout_seed", att.data_ptr() + 4 * (L - 1) * nh * N, L * nh * N, att_self.data_ptr() + 4 * (L - 1) * nh,
                  L * nh, _lib.ptr(num_ims), _lib.ptr(r), None, 0, None, B, T, nh, st)
        _lib.call("paths_attention_rollout_step", _lib.ptr(ws), _lib.ptr(num_ims), _lib.ptr(r), None, _lib.ptr(roll), N, _lib.ptr(roll_self),
                  B, T, d, nh, st)
        torch.cuda.synchronize()
        assert torch.equal(roll, serial[lvl]["rollout"]) and torch.equal(roll_self, serial[lvl]["rollout_self"]), lvl
