"""CPU side of the gradient-weighted attention relevance (paths_amd/saliency.py:attention_relevance): the float64
restatement (tests/relevance_ref.py) against torch's own autograd and against Chefer's update rule, the argument checks, and the
header / binding / source list / host-side validation of the two entry points."""
import ctypes
import math
import os
import types

import pytest
import torch

from tests import relevance_ref as R


def _operands(seed, B=3, H=3, T=9, hd=16):
    gen = torch.Generator().manual_seed(seed)
    q, k = (torch.randn((B, H, T, hd), generator=gen, dtype=torch.float64) * 1.5 for _ in range(2))
    v = torch.randn((B, H, T, hd), generator=gen, dtype=torch.float64)
    d_o = torch.randn((B, T, H * hd), generator=gen, dtype=torch.float64)
    r_in = torch.rand((B, T), generator=gen, dtype=torch.float64)
    num_ims = torch.tensor([T - 1, 0, 4][:B])
    return q, k, v, d_o, r_in, num_ims, math.log2(math.e) / math.sqrt(hd)


def _autograd_attention(q, k, v, d_o, n1, qscale):
    """(A, dL/dA) [H, n1, n1] of L = sum(dO * softmax(Q K^T) V) by torch autograd over the first n1 rows of one slide."""
    H, _, hd = q.shape
    a = torch.softmax(R.LN2 * qscale * (q[:, :n1] @ k[:, :n1].transpose(-1, -2)), dim=-1).requires_grad_()
    o = (a @ v[:, :n1]).transpose(0, 1).reshape(n1, H * hd)
    (o * d_o[:n1]).sum().backward()
    return a.detach(), a.grad


def test_step64_uses_the_gradient_autograd_gives():
    q, k, v, d_o, r_in, num_ims, qscale = _operands(1)
    got = R.step64(q, k, v, d_o, num_ims, qscale, r_in)
    env = R.step64(q, k, v, d_o, num_ims, qscale, r_in, absval=True)
    for b in range(q.shape[0]):
        n1 = int(num_ims[b]) + 1
        a, g = _autograd_attention(q[b], k[b], v[b], d_o[b], n1, qscale)
        want = r_in[b, :n1] + (r_in[b, :n1] @ (a * g).clamp_min(0).mean(0) if n1 > 1 else 0.0)
        assert (got[b, :n1] - want).abs().max() <= 1e-13
        assert (got[b, n1:] == 0).all()
        assert (env[b, :n1] >= got[b, :n1] - 1e-15).all()                 # |x| >= x^+
    assert torch.equal(got[1, :1], r_in[1, :1])                           # a slide without patches keeps its r


def test_lse64_is_the_log2_statistic_of_the_same_scores():
    q, k, _, _, _, num_ims, qscale = _operands(2)
    lse = R.lse64(q, k, num_ims, qscale)
    for b in range(q.shape[0]):
        n1 = int(num_ims[b]) + 1
        s = qscale * (q[b, :, :n1] @ k[b, :, :n1].transpose(-1, -2))
        assert (torch.exp2(s - lse[b, :, :n1, None]).sum(-1) - 1).abs().max() <= 1e-13
        assert torch.isnan(lse[b, :, n1:]).all()


def test_products_of_I_plus_Abar_are_chefers_update():
    """r = e_s^T (I + Abar_{L-1}) ... (I + Abar_0) three ways: Chefer's R <- R + Abar R from R = I read at row 0
    (relevance_from_attention), the explicit row-vector products, and seed64 followed by step64 from the last layer down."""
    B, H, T, hd, L = 3, 2, 7, 16, 3
    ops = [_operands(10 + l, B, H, T, hd) for l in range(L)]
    num_ims, qscale = ops[0][5], ops[0][6]
    att, grad = [], []
    for q, k, v, d_o, *_ in ops:
        a = torch.zeros((B, H, T, T), dtype=torch.float64)
        g = torch.zeros_like(a)
        for b in range(B):
            n1 = int(num_ims[b]) + 1
            a[b, :, :n1, :n1], g[b, :, :n1, :n1] = _autograd_attention(q[b], k[b], v[b], d_o[b], n1, qscale)
        att.append(a), grad.append(g)
    # the last layer is read at token 0 only: its output gradient lives on row 0
    grad[-1][:, :, 1:] = 0.0
    rel, rel_self = R.relevance_from_attention(att, grad, num_ims, T)
    q, k, v, d_o, *_ = ops[-1]
    r = R.seed64(q, k, v, d_o[:, 0], num_ims, qscale)
    for l in range(L - 2, -1, -1):
        q, k, v, d_o, *_ = ops[l]
        r = R.step64(q, k, v, d_o, num_ims, qscale, r)
    for b in range(B):
        n1 = int(num_ims[b]) + 1
        row = torch.zeros(n1, dtype=torch.float64)
        row[0] = 1.0
        if n1 > 1:
            for l in range(L - 1, -1, -1):
                row = row @ (torch.eye(n1, dtype=torch.float64) + (att[l][b, :, :n1, :n1] * grad[l][b, :, :n1, :n1]).clamp_min(0).mean(0))
        for other in (torch.cat((rel_self[b:b + 1], rel[b, :n1 - 1])), r[b, :n1]):
            assert (other - row).abs().max() <= 1e-12 * float(row.abs().max())
        assert (rel[b, n1 - 1:] == 0).all() and (r[b, n1:] == 0).all() and rel_self[b] >= 1
    assert rel_self[1] == 1                                               # num_ims = 0
    none_rel, none_self = R.relevance_from_attention(att, [None] * L, num_ims, T)   # no path to the target: r = e_s
    assert not none_rel.any() and (none_self == 1).all()


# ------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    from paths_amd import saliency
    from paths_amd.data_utils import slide as S
    model = types.SimpleNamespace(use_lstm=True)
    fn = saliency.attention_relevance
    with pytest.raises(NotImplementedError, match="lstm=false"):
        fn(types.SimpleNamespace(use_lstm=False), [], [2], 2)
    od = [S.OnDemandSlide([(2, 2)], lambda l, c: torch.zeros(len(c), 8), 8, "cpu")]
    with pytest.raises(NotImplementedError, match="on-demand"):
        fn(model, od, [2], 2)
    with pytest.raises(ValueError, match="unknown target"):
        fn(model, [], [2], 2, target="hazard")
    with pytest.raises(ValueError, match="integer"):
        fn(model, [], [2], 2, target="logit:x")
    wide = types.SimpleNamespace(use_lstm=True, procs=[types.SimpleNamespace(config=types.SimpleNamespace(trans_dim=512, trans_heads=4))])
    with pytest.raises(NotImplementedError, match="head_dim"):
        fn(wide, [], [2], 1)


def test_fp8_variants_are_refused(monkeypatch):
    from paths_amd import backward as bw, ops
    assert bw.relevance_unsupported(32) is None and bw.relevance_unsupported(64) is None
    assert "head_dim" in bw.relevance_unsupported(96)
    monkeypatch.setattr(ops, "AGG_FP8", True)
    assert "fp8" in bw.relevance_unsupported(32)


def test_hook_is_off_outside_the_context_manager():
    from paths_amd import backward as bw
    assert bw.RELEVANCE_SINK is None
    sink = []
    with bw.attention_relevance(sink):
        assert bw.RELEVANCE_SINK is sink
        with pytest.raises(RuntimeError):
            with bw.attention_relevance([]):
                raise RuntimeError("inside")
        assert bw.RELEVANCE_SINK is sink
    assert bw.RELEVANCE_SINK is None and sink == []


# ------------------------------------------------------------------------------------------------
# the C surface
# ------------------------------------------------------------------------------------------------
ENTRY_POINTS = (("paths_attention_relevance_seed", 22), ("paths_attention_relevance_step", 21))


def test_header_declares_the_entry_points_and_the_binding_matches():
    from paths_amd import _lib
    for name, nargs in ENTRY_POINTS:
        assert name in _lib.DECLARATIONS, f"{name} is not declared in include/paths_hip.h"
        res, args = _lib.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == len(_lib.SIGNATURES[name]) == nargs
    assert _lib.ABI_VERSION == 3                                      # no existing signature changed
    import __graft_entry__ as g
    assert "attn_relevance.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "attn_relevance.hip"))


def test_build_compiles_the_new_file_and_exports_the_entry_points():
    import __graft_entry__ as g
    from paths_amd import _lib
    g.build()
    lib = _lib.load()
    assert lib.paths_abi_version() == 3
    for name, _ in ENTRY_POINTS:
        assert hasattr(lib, name)
    if os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        assert os.path.getmtime(os.path.join(g.OBJDIR, "attn_relevance.o")) >= os.path.getmtime(os.path.join(g.CSRC, "attn_relevance.hip"))


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)
    B, H, T, hd = 2, 4, 65, 32
    hm = (H * T * hd, T * hd, hd)

    def seed(q=A, k=A, v=A, s=hm, da0=A, da0_ld=H * hd, lse0=A, ni=A, r=A, rel=None, rel_ld=0, rel_self=None, B=B, T=T, H=H, hd=hd):
        return lib.paths_attention_relevance_seed(q, k, v, *s, 1.0, da0, da0_ld, lse0, H, 1, ni, r, rel, rel_ld, rel_self, B, T, H, hd, None)

    def step(q=A, k=A, v=A, s=hm, d_o=A, ld_o=H * hd, lse=A, ni=A, r_in=A, r_out=2 * A, rel=None, rel_ld=0, rel_self=None, B=B, T=T, H=H,
             hd=hd):
        return lib.paths_attention_relevance_step(q, k, v, *s, 1.0, d_o, ld_o, lse, ni, r_in, r_out, rel, rel_ld, rel_self, B, T, H, hd, None)

    for fn in (seed, step):
        assert fn(q=None) == -1 and b"null" in lib.paths_last_error()
        assert fn(ni=None) == -1 and b"null" in lib.paths_last_error()
        assert fn(B=0) == -1 and b"bad shape" in lib.paths_last_error()
        assert fn(T=0) == -1 and b"bad shape" in lib.paths_last_error()
        for bad in (8, 40, 96, 128):
            assert fn(hd=bad) == -1 and b"head_dim" in lib.paths_last_error()
        assert fn(k=A + 4) == -1 and b"aligned" in lib.paths_last_error()
        assert fn(s=(H * T * hd, T * hd, hd + 2)) == -1 and b"strides" in lib.paths_last_error()
        assert fn(s=(H * T * hd, T * hd, 16)) == -1 and b"strides" in lib.paths_last_error()
    assert seed(da0_ld=H * hd - 4) == -1 and b"da0" in lib.paths_last_error()
    assert seed(r=None) == -1 and b"null" in lib.paths_last_error()                       # neither r nor the outputs
    assert seed(r=None, rel=A, rel_ld=T - 2, rel_self=A) == -1 and b"strides" in lib.paths_last_error()
    assert step(ld_o=H * hd - 4) == -1 and b"d_o" in lib.paths_last_error()
    assert step(r_out=None) == -1 and b"null" in lib.paths_last_error()
    assert step(r_out=A) == -1 and b"r_out must not be r_in" in lib.paths_last_error()
    assert step(r_out=None, rel=A, rel_ld=T - 2, rel_self=A) == -1 and b"stride" in lib.paths_last_error()
    with pytest.raises(_lib.PathsHipError, match=r"paths_attention_relevance_step failed \(-1\)"):
        _lib.call("paths_attention_relevance_step", None, None, None, 0, 0, 0, 1.0, None, 0, None, None, None, None, None, 0, None, 1, 1, 1, 32,
                  None)


# ------------------------------------------------------------------------------------------------
# the raster
# ------------------------------------------------------------------------------------------------
def test_relevance_map_two_level_hierarchy():
    import numpy as np
    from paths_amd.heatmap import hierarchy_from_trace, relevance_map
    trace = [{"num_ims": torch.tensor([2]), "locs": torch.tensor([[[0, 0], [256, 0], [0, 0]]]), "importance": torch.zeros(1, 3),
              "parent_inds": torch.zeros(1, 3, dtype=torch.long), "keep_idx": torch.tensor([[1]]), "keep_count": torch.tensor([1]),
              "attention_relevance": torch.tensor([[0.25, 0.5, 0.0]]), "attention_relevance_self": torch.tensor([1.5])},
             {"num_ims": torch.tensor([1]), "locs": torch.tensor([[[768, 256]]]), "importance": torch.zeros(1, 1),
              "parent_inds": torch.zeros(1, 1, dtype=torch.long), "attention_relevance": torch.tensor([[2.0]]),
              "attention_relevance_self": torch.tensor([1.0])}]
    levels = hierarchy_from_trace(trace, 0)
    assert levels[0]["attention_relevance"].tolist() == [0.25, 0.5] and levels[0]["attention_relevance_self"] == 1.5
    m0, m1 = relevance_map(levels, (2, 1))
    assert m0.shape == m1.shape == (4, 2)
    assert np.array_equal(m0, np.array([[0.25, 0.25], [0.25, 0.25], [0.5, 0.5], [0.5, 0.5]]))
    want = np.zeros((4, 2))
    want[3, 1] = 2.0
    assert np.array_equal(m1, want)
    with pytest.raises(KeyError, match="attention relevance"):
        relevance_map([{k: v for k, v in lv.items() if not k.startswith("attention_relevance")} for lv in levels], (2, 1))
