"""CPU side of the attributions along the frozen path (paths_amd/saliency.py: integrated_gradients / smooth_grad): the
restated Gaussian generator's statistics, the quadrature rules, the oracle-along-a-recorded-path reference (tests/path_ref.py) and
its completeness, the argument checks, the header / binding of the two entry points and their host-side argument validation."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import path_ref as R

KEYS = ((1, 0), (2, 0), (0x1234, 7), (99, 3), (5, 5), (123456789, 42))        # (key_lo, key_hi)
IG_STEPS = 8         # fixed by test_reference_completeness_fixes_the_steps; tests/test_gpu_path_attributions.py uses it


# ------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------
def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_generator_statistics():
    """n = 64 x 128 draws (64 rows of D = 128) per key; bounds in standard errors of the statistic under the null (conditions set
    beforehand, not measurements): |mean| <= 4 / sqrt(n), |var - 1| <= 4 sqrt(2 / n), lag-1 / 2 / 128 autocorrelation
    <= 4 / sqrt(n - lag), correlation between consecutive keys <= 4 / sqrt(n), Kolmogorov-Smirnov distance <= 1.95 / sqrt(n)."""
    n = 64 * 128
    e = np.arange(n, dtype=np.uint64)
    zs = [R.gauss(lo, hi, e) for lo, hi in KEYS]
    worst = dict(mean=0.0, var=0.0, lag1=0.0, lag2=0.0, lag128=0.0, cross=0.0, ks=0.0)
    for z in zs:
        assert np.abs(z).max() <= 5.89
        worst["mean"] = max(worst["mean"], abs(z.mean()) * np.sqrt(n))
        worst["var"] = max(worst["var"], abs(z.var() - 1.0) / np.sqrt(2.0 / n))
        for lag in (1, 2, 128):
            worst[f"lag{lag}"] = max(worst[f"lag{lag}"], abs(_corr(z[:-lag], z[lag:])) * np.sqrt(n - lag))
        zsort = np.sort(z)
        cdf = R.normal_cdf(zsort)
        ks = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))
        worst["ks"] = max(worst["ks"], ks * np.sqrt(n))
    for a, b in zip(zs[:-1], zs[1:]):
        worst["cross"] = max(worst["cross"], abs(_corr(a, b)) * np.sqrt(n))
    print("worst, in standard errors:", {k: round(float(v), 3) for k, v in worst.items()})
    for k in ("mean", "var", "lag1", "lag2", "lag128", "cross"):
        assert worst[k] <= 4.0, (k, worst[k])
    assert worst["ks"] <= 1.95, worst["ks"]


def test_generator_by_hand_and_extremes():
    """One pair restated with python integers; the draw depends on (key, element) only; the extreme hashes stay finite."""
    from paths_amd.saliency import _fmix32
    lo, hi, e = 0x1234, 7, 2 * 77
    def h(i):
        return _fmix32(((i & 0xFFFFFFFF) * 0x9E3779B1 + lo) ^ _fmix32((i >> 32) * 0x85EBCA77 + hi))
    assert int(R.drop_hash(np.uint64(e), lo, hi)) == h(e) and int(R.drop_hash(np.uint64(e + 1), lo, hi)) == h(e + 1)
    big = (5 << 32) + 10
    assert int(R.drop_hash(np.uint64(big), lo, hi)) == h(big)
    u1, u2 = ((h(e) >> 8) + 0.5) / 2 ** 24, (h(e + 1) >> 8) / 2 ** 24
    rad = np.sqrt(-2 * np.log(u1))
    z = R.gauss(lo, hi, np.array([e, e + 1], np.uint64))
    np.testing.assert_allclose(z, [rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)], rtol=1e-14)
    assert np.sqrt(-2 * np.log(0.5 / 2 ** 24)) <= 5.89                       # the largest radius any hash can give
    np.testing.assert_array_equal(R.gauss(lo, hi, np.arange(64, dtype=np.uint64))[10:20], R.gauss(lo, hi, np.arange(10, 20, dtype=np.uint64)))


def test_noise_keys_are_distinct_and_64_bit():
    from paths_amd.saliency import noise_key
    ks = {noise_key(s, l, n, b) for s in (0, 1, 1 << 40) for l in range(5) for n in range(16) for b in range(8)}
    assert len(ks) == 3 * 5 * 16 * 8 and all(0 <= k < 1 << 64 for k in ks)
    assert len({k & 0xFFFFFFFF for k in ks}) > 1900 and len({k >> 32 for k in ks}) > 1900
    assert noise_key(3, 1, 2, 0) == noise_key(3, 1, 2, 0)


# ------------------------------------------------------------------------------------------------
# quadrature
# ------------------------------------------------------------------------------------------------
def test_quadrature_rules():
    from paths_amd.saliency import quadrature
    for rule in ("gausslegendre", "midpoint"):
        for steps in (1, 3, 8, 32):
            a, w = quadrature(rule, steps)
            assert a.shape == w.shape == (steps,) and a.dtype == w.dtype == np.float64
            assert abs(w.sum() - 1.0) <= 1e-14 and (a > 0).all() and (a < 1).all() and (w > 0).all()
    a, w = quadrature("midpoint", 4)
    np.testing.assert_array_equal(a, [0.125, 0.375, 0.625, 0.875])
    np.testing.assert_array_equal(w, [0.25] * 4)
    # degree 5 in alpha, exact at 3 nodes: int_0^1 (3 a^5 - 2 a^4 + a^2 - 7 a + 0.5) da
    a, w = quadrature("gausslegendre", 3)
    poly = lambda t: 3 * t ** 5 - 2 * t ** 4 + t ** 2 - 7 * t + 0.5
    assert abs((w * poly(a)).sum() - (3 / 6 - 2 / 5 + 1 / 3 - 7 / 2 + 0.5)) <= 1e-14
    a, w = quadrature("midpoint", 3)
    assert abs((w * poly(a)).sum() - (3 / 6 - 2 / 5 + 1 / 3 - 7 / 2 + 0.5)) > 1e-3      # (the midpoint rule is not)


# ------------------------------------------------------------------------------------------------
# the row contracts by hand
# ------------------------------------------------------------------------------------------------
def test_row_references_by_hand():
    x = np.array([[[1.0, -2.0, 3.0, 4.0], [9.0, 9.0, 9.0, 9.0]]])
    base = np.array([1.0, 0.0, 1.0, 0.0])
    out, det, rms = R.path_points(x, base, [0.5, 1.0], [0.0, 0.0], None, np.array([1]))
    np.testing.assert_array_equal(out[0, 0], [1.0, -1.0, 2.0, 2.0])
    np.testing.assert_array_equal(out[1, 0], x[0, 0])
    assert not out[:, 1].any() and rms[0, 0] == np.sqrt(30 / 4) and rms[0, 1] == 0
    np.testing.assert_array_equal(det[0, 0], [1.0, 1.0, 2.0, 2.0])
    out, _, _ = R.path_points(np.ones((1, 1, 4)), None, [0.0], [1.0], [(7 << 32) | 0x1234], np.array([1]))
    np.testing.assert_array_equal(out[0, 0], R.gauss(0x1234, 7, np.arange(4, dtype=np.uint64)))
    dx = np.array([[[1.0, 1.0, 0.0, 2.0], [5.0, 5.0, 5.0, 5.0]], [[0.0, 1.0, 1.0, 0.0], [5.0, 5.0, 5.0, 5.0]]])
    gxi, sq, adx, ag, aq = R.path_accumulate(dx, x, base, [2.0, -1.0], np.array([1]))
    # member 0: (0, -2, 0, 8) -> 6, squares 6;  member 1: (0, -2, 2, 0) -> 0, squares 2
    np.testing.assert_array_equal(gxi, [[12.0, 0.0]])
    np.testing.assert_array_equal(sq, [[12.0 - 2.0, 0.0]])
    np.testing.assert_array_equal(adx[0, 0], [2.0, 1.0, -1.0, 4.0])
    np.testing.assert_array_equal(ag, [[2 * 10.0 + 4.0, 0.0]])
    np.testing.assert_array_equal(aq, [[14.0, 0.0]])
    assert not adx[0, 1].any()


# ------------------------------------------------------------------------------------------------
# the reference along the recorded path, and its completeness
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """The small setting of tests/test_gpu_saliency._setup: 3 synthetic slides, base (6, 7), top-16, 5 levels, weights of seed 3."""
    from oracle import paths_oracle as orc
    from paths_amd import synthetic as syn
    ocfg = H.oracle_config(None, top_k_patches=[16] * 4)
    params = H.oracle_params(ocfg, 3)
    grids = [orc.LazyGrids(syn.SyntheticSlide(14, sid, (6, 7), 1024, 5, 0.1)) for sid in range(3)]
    otrace = []
    with torch.no_grad():
        orc.inference_end2end(params, ocfg, grids, None, otrace)
    return ocfg, params, grids, otrace


def test_frozen_path_reproduces_the_oracle(small):
    ocfg, params, grids, otrace = small
    ref = R.frozen_path(params, ocfg, grids, otrace, None, "risk")
    assert torch.equal(ref["logits"], otrace[-1]["logits"])                      # bit for bit
    assert all(g.shape == rec["locs"].shape[:2] + (1024,) for g, rec in zip(ref["grads"], otrace))
    assert all(float(g.abs().sum()) > 0 for g in ref["grads"])
    for g, rec in zip(ref["grads"], otrace):                                     # padded rows carry no gradient
        pad = torch.arange(g.shape[1])[None, :] >= rec["num_ims"][:, None]
        assert float(g[pad].abs().sum()) == 0.0
    assert not any(any(rec["fallback"]) for rec in otrace)
    # alpha = 0: all-zero rows everywhere would be background to the free recursion; the frozen path does not look
    zero = R.frozen_path(params, ocfg, grids, otrace, [torch.zeros_like(x) for x in R.recorded_rows(grids, otrace)], "risk")
    assert torch.isfinite(zero["target"]).all() and not torch.equal(zero["target"], ref["target"])


def test_reference_completeness_fixes_the_steps(small):
    """Gauss-Legendre in float64 over the fp32 reference gradients: the smallest of 8 / 16 / 32 steps at which the reference's own
    completeness gap is at most 1 % of |F(X) - F(0)| for every slide is what the GPU test uses (IG_STEPS).
    Measured: steps = 8 gives gaps of 0.18 %, 0.15 % and 0.08 % of |F(X) - F(0)| for the three slides."""
    from paths_amd.saliency import quadrature
    ocfg, params, grids, otrace = small
    rows = R.recorded_rows(grids, otrace)
    f1 = R.frozen_path(params, ocfg, grids, otrace, rows, "risk")["target"].double()
    f0 = R.frozen_path(params, ocfg, grids, otrace, [torch.zeros_like(x) for x in rows], "risk")["target"].double()
    chosen = None
    for steps in (8, 16, 32):
        a, w = quadrature("gausslegendre", steps)
        total = torch.zeros(3, dtype=torch.float64)
        for al, wt in zip(a, w):
            g = R.frozen_path(params, ocfg, grids, otrace, [(x.double() * al).float() for x in rows], "risk")["grads"]
            total += wt * sum((gl.double() * x.double()).sum(dim=(1, 2)) for gl, x in zip(g, rows))
        gap = (total - (f1 - f0)).abs() / (f1 - f0).abs()
        print(f"steps {steps}: completeness gap / |F(X) - F(0)| = {gap.tolist()}")
        if bool((gap <= 0.01).all()):
            chosen = steps
            break
    assert chosen == IG_STEPS


# ------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    from paths_amd import saliency
    from paths_amd.data_utils import slide as S
    model = types.SimpleNamespace(use_lstm=True)
    nolstm = types.SimpleNamespace(use_lstm=False)
    for fn in (saliency.integrated_gradients, saliency.smooth_grad):
        with pytest.raises(NotImplementedError, match="lstm=false"):
            fn(nolstm, [], [2], 2)
        od = [S.OnDemandSlide([(2, 2)], lambda l, c: torch.zeros(len(c), 8), 8, "cpu")]
        with pytest.raises(NotImplementedError, match="on-demand"):
            fn(model, od, [2], 2)
        with pytest.raises(ValueError, match="unknown target"):
            fn(model, [], [2], 2, target="hazard")
    for steps in (0, -3):
        with pytest.raises(ValueError, match="steps"):
            saliency.integrated_gradients(model, [], [2], 2, steps=steps)
    with pytest.raises(ValueError, match="rule"):
        saliency.integrated_gradients(model, [], [2], 2, rule="simpson")
    for bad in (torch.zeros(2, 3), torch.zeros(()), [0.0] * 8):
        with pytest.raises(ValueError, match="baseline"):
            saliency.integrated_gradients(model, [], [2], 2, baseline=bad)
    with pytest.raises(ValueError, match="samples"):
        saliency.smooth_grad(model, [], [2], 2, samples=0)
    with pytest.raises(ValueError, match="sigma"):
        saliency.smooth_grad(model, [], [2], 2, sigma=-0.1)


def test_heatmap_passes_the_new_keys_through():
    from paths_amd.heatmap import hierarchy_from_trace, saliency_map
    N = 3
    vals = {k: torch.tensor([[0.5, -0.25, 9.0]]) * (i + 1) for i, k in enumerate(("integrated_gradients", "smooth_grad_x_input", "smooth_grad_sq"))}
    tr = [dict(vals, num_ims=torch.tensor([2]), locs=torch.tensor([[[0, 0], [256, 0], [0, 0]]]), importance=torch.rand(1, N),
               parent_inds=torch.zeros((1, N), dtype=torch.int64))]
    lv = hierarchy_from_trace(tr, 0)
    for i, k in enumerate(vals):
        np.testing.assert_array_equal(lv[0][k], np.array([0.5, -0.25], np.float32) * (i + 1))
        (m,) = saliency_map(lv, (2, 1), kind=k)
        np.testing.assert_array_equal(m, np.array([[0.5], [-0.25]]) * (i + 1))
    with pytest.raises(KeyError):
        saliency_map(lv, (2, 1), kind="grad_norm")
    with pytest.raises(ValueError):
        saliency_map(lv, (2, 1), kind="importance")


# ------------------------------------------------------------------------------------------------
# the C surface
# ------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_binding_matches():
    from paths_amd import _lib
    for name, nargs in (("paths_path_points", 13), ("paths_path_accumulate", 16)):
        assert name in _lib.DECLARATIONS, f"{name} is not declared in include/paths_hip.h"
        res, args = _lib.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == len(_lib.SIGNATURES[name]) == nargs
    assert _lib.ABI_VERSION == 3                                      # no existing signature changed
    import __graft_entry__ as g
    assert "path_rows.hip" in g.SOURCES


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    A = 4096                                    # (a 16-byte aligned non-null address: never dereferenced, every call below is rejected)
    pts = lambda x, ldx, base, al, sg, keys, ni, N, D, B, C, out: lib.paths_path_points(x, ldx, base, al, sg, keys, ni, N, D, B, C, out, None)
    assert pts(None, 128, None, A, A, None, A, 4, 128, 2, 1, A) == -1 and b"null" in lib.paths_last_error()
    assert pts(A, 128, None, A, A, None, A, 4, 128, 2, 1, None) == -1 and b"null" in lib.paths_last_error()
    assert pts(A, 128, None, A, A, None, A, 4, 64, 2, 1, A) == -1 and b"multiple of 128" in lib.paths_last_error()
    assert pts(A, 128, None, A, A, None, A, 4, 128, 2, 0, A) == -1 and b"positive" in lib.paths_last_error()
    assert pts(A, 128, None, A, A, None, A, 0, 128, 2, 1, A) == -1 and b"positive" in lib.paths_last_error()
    assert pts(A, 126, None, A, A, None, A, 4, 128, 2, 1, A) == -1 and b"stride" in lib.paths_last_error()
    assert pts(A, 128, A + 4, A, A, None, A, 4, 128, 2, 1, A) == -1 and b"aligned" in lib.paths_last_error()
    acc = lambda dx, ldd, x, ldx, base, w, ni, N, D, B, C, init, g, q, a: lib.paths_path_accumulate(dx, ldd, x, ldx, base, w, ni, N, D, B, C,
                                                                                                    init, g, q, a, None)
    assert acc(None, 128, A, 128, None, A, A, 4, 128, 2, 1, 1, A, A, None) == -1 and b"null" in lib.paths_last_error()
    assert acc(A, 128, A, 128, None, A, A, 4, 128, 2, 1, 1, A, None, None) == -1 and b"null" in lib.paths_last_error()
    assert acc(A, 128, A, 128, None, A, A, 4, 0, 2, 1, 1, A, A, None) == -1 and b"multiple of 128" in lib.paths_last_error()
    assert acc(A, 128, A, 128, None, A, A, 4, 128, 0, 1, 1, A, A, None) == -1 and b"positive" in lib.paths_last_error()
    assert acc(A, 130, A, 128, None, A, A, 4, 128, 2, 1, 1, A, A, None) == -1 and b"strides" in lib.paths_last_error()
    assert acc(A, 128, A, 128, None, A, A, 4, 128, 2, 1, 1, A, A, A + 8) == -1 and b"aligned" in lib.paths_last_error()
    with pytest.raises(_lib.PathsHipError, match=r"paths_path_points failed \(-1\)"):
        _lib.call("paths_path_points", None, 128, None, None, None, None, None, 4, 128, 2, 1, None, None)
