"""CPU side of the gradient x input attributions (paths_amd/saliency.py): target parsing against float64, the float64 row reference
(tests/saliency_ref.py), the rasters of paths_amd.heatmap.saliency_map, the lstm=false rejection, the backward's weight-gradient
switch and the host-side argument checks of paths_saliency_rows (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import saliency_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_targets_parse_and_risk_matches_float64():
    from paths_amd.saliency import parse_target, risk_score
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(5, 4, generator=g) * 3
    want = S.risk_score(logits.numpy())
    got = parse_target("risk")(logits)
    assert got.shape == (5,) and parse_target("risk") is risk_score
    # four sigmoids, three products and four adds in fp32 on values in [0, 1]: a few units of roundoff of the largest possible sum (4)
    assert np.abs(got.double().numpy() - want).max() <= 16 * S.U * 4
    assert np.abs(risk_score(logits.double()).numpy() - want).max() <= 1e-14
    # by hand, one row: hazards h -> -(s1 + s1 s2 + ...) with s_k = 1 - h_k
    h = 1 / (1 + np.exp(-logits[0].double().numpy()))
    s = 1 - h
    assert abs(want[0] + (s[0] + s[0] * s[1] + s[0] * s[1] * s[2] + s[0] * s[1] * s[2] * s[3])) <= 1e-15
    assert torch.equal(parse_target("logit:1")(logits), logits[:, 1])
    assert torch.equal(parse_target("logit:-1")(logits), logits[:, 3])
    fn = lambda lg: lg.sum(1)
    assert parse_target(fn) is fn
    for bad in ("hazard", "logit:", "logit:x", "logit", 3):
        with pytest.raises(ValueError):
            parse_target(bad)
    with pytest.raises(ValueError):
        parse_target("logit:4")(logits)
    # the risk is differentiable where the pass needs it to be
    lg = logits.clone().requires_grad_(True)
    risk_score(lg).sum().backward()
    assert lg.grad is not None and bool((lg.grad > 0).all())          # a larger hazard anywhere = a higher risk


def test_row_reference_by_hand():
    dx = np.array([[[3.0, -4.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [5.0, 5.0, 5.0, 5.0]]])
    x = np.array([[[2.0, 1.0, 7.0, 7.0], [1.0, -2.0, 3.0, -4.0], [1.0, 1.0, 1.0, 1.0]]])
    gxi, gnorm, absdot = S.saliency_rows(dx, x, np.array([2]))
    np.testing.assert_array_equal(gxi, [[2.0, -2.0, 0.0]])
    np.testing.assert_array_equal(gnorm, [[5.0, 2.0, 0.0]])
    np.testing.assert_array_equal(absdot, [[10.0, 10.0, 0.0]])
    assert S.gamma(128) == 128 * S.U / (1 - 128 * S.U)


def _two_levels():
    # level 0: 2 x 1 grid, both patches visited; level 1 (4 x 2 grid): two children of patch (0, 0) and one of patch (1, 0)
    lv0 = {"locs": np.array([[0, 0], [256, 0]]), "importance": np.array([0.5, 0.25], np.float32),
           "grad_x_input": np.array([-0.375, 0.125], np.float32), "grad_norm": np.array([2.0, 0.5], np.float32)}
    lv1 = {"locs": np.array([[0, 1], [1, 0], [3, 1]]) * 256, "importance": np.array([0.1, 0.2, 0.3], np.float32),
           "grad_x_input": np.array([0.25, -0.0625, 0.1875], np.float32), "grad_norm": np.array([1.0, 3.0, 0.25], np.float32)}
    return [lv0, lv1]


def test_saliency_map_two_level_hierarchy():
    from paths_amd.heatmap import saliency_map
    m0, m1 = saliency_map(_two_levels(), (2, 1))
    assert m0.shape == m1.shape == (4, 2)
    want0 = np.zeros((4, 2))
    want0[0:2, :], want0[2:4, :] = -0.375, 0.125                     # a level-0 patch covers 2 x 2 finest cells; signs survive
    np.testing.assert_array_equal(m0, want0)
    want1 = np.zeros((4, 2))
    want1[0, 1], want1[1, 0], want1[3, 1] = 0.25, -0.0625, 0.1875
    np.testing.assert_array_equal(m1, want1)                         # 0 where level 1 did not visit; no fold into level 0
    n0, n1 = saliency_map(_two_levels(), (2, 1), kind="grad_norm")
    wantn = np.zeros((4, 2))
    wantn[0, 1], wantn[1, 0], wantn[3, 1] = 1.0, 3.0, 0.25
    np.testing.assert_array_equal(n1, wantn)
    assert n0[0, 0] == 2.0 and n0[3, 1] == 0.5
    with pytest.raises(KeyError):
        saliency_map([{k: v for k, v in lv.items() if not k.startswith("grad_")} for lv in _two_levels()], (2, 1))
    with pytest.raises(KeyError):
        saliency_map([{k: v for k, v in lv.items() if k != "grad_norm"} for lv in _two_levels()], (2, 1), kind="grad_norm")
    with pytest.raises(ValueError):
        saliency_map(_two_levels(), (2, 1), kind="importance")


def test_hierarchy_from_trace_carries_the_attributions():
    from paths_amd.heatmap import hierarchy_from_trace
    N = 4
    gxi = torch.tensor([[0.25, -0.125, 0.0625, 0.0], [-0.5, 0.0, 0.0, 0.0]])
    gn = torch.tensor([[1.0, 2.0, 3.0, 0.0], [4.0, 0.0, 0.0, 0.0]])
    tr = [{"num_ims": torch.tensor([3, 1]), "locs": torch.zeros((2, N, 2), dtype=torch.int64), "importance": torch.rand(2, N),
           "parent_inds": torch.zeros((2, N), dtype=torch.int64), "grad_x_input": gxi, "grad_norm": gn,
           "grad": torch.zeros((2, N, 8))}]
    lv = hierarchy_from_trace(tr, 0)[0]
    np.testing.assert_array_equal(lv["grad_x_input"], gxi[0, :3].numpy())
    np.testing.assert_array_equal(lv["grad_norm"], gn[0, :3].numpy())
    lv1 = hierarchy_from_trace(tr, 1)[0]
    np.testing.assert_array_equal(lv1["grad_x_input"], np.array([-0.5], np.float32))
    plain = hierarchy_from_trace([{k: v for k, v in tr[0].items() if not k.startswith("grad")}], 1)[0]
    assert "grad_x_input" not in plain and "grad_norm" not in plain


def test_lstm_false_is_rejected_by_name():
    from paths_amd.config import Config
    from paths_amd.saliency import input_gradients
    cfg = Config.load(os.path.join(ROOT, "tests", "golden", "sample"), test_mode=True)
    cfg.model_config.lstm = False
    torch.manual_seed(0)
    model = cfg.get_model()
    assert not model.use_lstm
    with pytest.raises(NotImplementedError, match="lstm=false"):
        input_gradients(model, [], cfg.top_k_patches, cfg.num_levels)
    assert model.training                                            # (rejected before the mode switch)


def test_weight_gradient_switch_nests_and_restores():
    from paths_amd import backward as bw
    assert bw.WEIGHT_GRADS is True
    ran = []
    with bw.no_weight_grads():
        assert bw.WEIGHT_GRADS is False
        with bw.no_weight_grads():
            assert bw.WEIGHT_GRADS is False
        assert bw.WEIGHT_GRADS is False
        bw.after_reductions(lambda: ran.append(1))                   # a touch-up of a weight gradient: dropped
        out = torch.empty((0,))
        assert bw.gemm_tn(None, 0, None, 0, out, 0, 0, 0) is None     # returns before it looks at an operand
        assert bw.colsum(0, 0, 0, 4, out=out) is out
    assert bw.WEIGHT_GRADS is True and not ran
    with pytest.raises(RuntimeError):
        with bw.no_weight_grads():
            raise RuntimeError("x")
    assert bw.WEIGHT_GRADS is True
    bw.after_reductions(lambda: ran.append(1))
    assert ran == [1]


def test_header_declares_the_symbol_and_the_binding_matches():
    from paths_amd import _lib
    assert "paths_saliency_rows" in _lib.DECLARATIONS, "paths_saliency_rows is not declared in include/paths_hip.h"
    res, args = _lib.DECLARATIONS["paths_saliency_rows"]
    assert res is ctypes.c_int and len(args) == len(_lib.SIGNATURES["paths_saliency_rows"]) == 11
    assert _lib.ABI_VERSION == 3


def test_saliency_rows_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    assert lib.paths_abi_version() == 3
    A = 4096                                    # (a 16-byte aligned non-null address: never dereferenced, every call below is rejected)
    call = lambda dx, ldd, x, ldx, ni, N, D, B, o1, o2: lib.paths_saliency_rows(dx, ldd, x, ldx, ni, N, D, B, o1, o2, None)
    assert call(None, 128, A, 128, A, 4, 128, 2, A, A) == -1 and b"null" in lib.paths_last_error()
    assert call(A, 128, A, 128, A, 4, 128, 2, A, None) == -1 and b"null" in lib.paths_last_error()
    assert call(A, 128, A, 128, A, 4, 64, 2, A, A) == -1 and b"multiple of 128" in lib.paths_last_error()
    assert call(A, 128, A, 128, A, 4, 0, 2, A, A) == -1 and b"multiple of 128" in lib.paths_last_error()
    assert call(A, 128, A, 128, A, 0, 128, 2, A, A) == -1 and b"positive" in lib.paths_last_error()
    assert call(A, 128, A, 128, A, 4, 128, 0, A, A) == -1 and b"positive" in lib.paths_last_error()
    assert call(A, 128, A, 126, A, 4, 128, 2, A, A) == -1 and b"strides" in lib.paths_last_error()
    assert call(A, 130, A, 128, A, 4, 128, 2, A, A) == -1 and b"strides" in lib.paths_last_error()
    assert call(A + 4, 128, A, 128, A, 4, 128, 2, A, A) == -1 and b"aligned" in lib.paths_last_error()
    with pytest.raises(_lib.PathsHipError, match=r"paths_saliency_rows failed \(-1\)"):
        _lib.call("paths_saliency_rows", None, 128, None, 128, None, 4, 128, 2, None, None, None)
