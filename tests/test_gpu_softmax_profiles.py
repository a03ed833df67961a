"""The forward attention kernels' running softmax on structured score rows (tests/softmax_profiles.py), through the C ABI, against
float64 (tests/attn_ref.py and the restatements the exports already have).

Every forward kernel keeps a running (m, l, O) per query across 64-key steps; csrc/attn_x6.hip defers the rescale, takes exp2
optimistically against a maximum that starts at 0 and revises (re-basing the next step's scores, which are in flight), the 32x32
kernels do the same, and the key-split forms (the wave-pair kernel's and attn_h3_any's small block, attn_token0.hip, the tails,
attn_rollout.hip) merge partials whose neutral elements differ.  Which path a row takes depends on where along the keys its large
scores fall; the profiles put them there (every step rising, a slow ramp under the deferral threshold, a cliff, a spike in the
masked last step, spikes at consecutive steps, equal spikes in different splits, offsets of +-320, a huge masked key), with rows
that rise, fall and stay flat in one 16-query tile.  tests/test_cpu_softmax_profiles.py shows that the inputs' products are exact
and which steps must revise.

Entry points: paths_attention_f32, paths_attention_x6 (three planes; two planes under PATHS_ATTN_M32 = 0, 1, 3; the pair kernel's
key-split block), paths_attention_x6_dropout (p = 0.1, two and three planes: the deferred non-optimistic step), paths_attention_any,
_any_train, _h3_any (head_dim 16 / 32 / 48 / 64: the one-wave loop and, up to 48, the 4-wave merge), _wide_fwd (two passes: the
control), _token0_any, _token0_fwd, paths_token0_tail, paths_token0_tail_ws, paths_token0_attention, paths_attention_rollout_prepare
(+ one step).  Where a kernel picks a branch by shape, the launcher's condition is asserted on the shapes used.

Checks: every valid row finite and within the bar of float64, lse within its bar; padded rows as the entry points' own tests ask.
Bars: the entry point's bar in its random-input test (2e-6 x6 / f32 / token0, 5e-6 any / h3_any, O_BAR relative for the training
forwards, LSE_BAR), or - where fp32 itself cannot do better on a profile: token-major scores of magnitude 320 after the rounding of
g / qscale, an lse near 320 - 4x the error of the same formula in plain float32 torch on the CPU on the same inputs
(softmax_profiles.formula_f32; the largest over the slides of the profile), whichever is larger.  Never from the kernel under test.

Not covered here: the e4m3 variants (csrc/attn_fp8.hip: their error is the format's and has measured-bar tests) and the backward
kernels (they recompute exp2(s - lse) from a saved lse and keep no running state; tests/test_gpu_attention_backward.py gives them a
sharp and a near-uniform head).
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import chain_ref as R
from tests import rollout_ref
from tests import softmax_profiles as SP
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LN2 = SP.LN2
X6_BAR = 2e-6              # absolute, test_attention_x6_matches_fp64 / test_attention_32x32_kernels_match_fp64
ANY_BAR = 5e-6             # absolute, test_attention_h3_any_matches_fp64
T0_BAR = 2e-6              # absolute, the token-0 forms (same test) and the exports' probabilities
LSE_BAR = 1e-4             # log2 units
O_BAR = 1e-5               # training forwards: relative to max|o| of the slide (tests/test_gpu_attention_backward.py)
DROP_KEY = 0x5EED_0A77_E5D0_0B1D

# BAR: per entry point the worst error measured on one MI355X over the three bundles (and head dims), the profile it fell on, the
# float32 yardstick of that profile (largest error of softmax_profiles.formula_f32 against float64 over the slides, in the metric of
# the bar) and the bar that held there, max(base, 4 x yardstick); from the "[softmax]" lines of a run with -s.
#   entry point                      o: worst    yardstick  bar      profile        lse: worst  yardstick  bar      profile
#   f32                              7.8e-7      4.8e-7     2.0e-6   twin_spikes    1.6e-5      1.6e-5     1.0e-4   offset_up
#   x6 planes 3                      4.2e-7      4.8e-7     2.0e-6   twin_spikes    1.6e-5      1.6e-5     1.0e-4   offset_up
#   x6 planes 2, M32 = 0             5.4e-7      2.8e-7     2.0e-6   late_spike     1.6e-5      1.6e-5     1.0e-4   offset_up
#   x6 planes 2, M32 = 1             5.8e-7      4.8e-7     2.0e-6   twin_spikes    1.6e-5      1.6e-5     1.0e-4   offset_down
#   x6 planes 2, M32 = 3             5.8e-7      4.8e-7     2.0e-6   twin_spikes    1.6e-5      1.6e-5     1.0e-4   offset_down
#   x6 pair kernel, key-split        6.7e-7      5.1e-7     2.0e-6   twin_spikes    1.6e-5      1.6e-5     1.0e-4   offset_down
#   x6_dropout planes 2 (rel)        5.2e-7      5.8e-7     1.0e-5   twin_spikes    1.6e-5      1.6e-5     1.0e-4   offset_up
#   x6_dropout planes 3 (rel)        6.4e-7      5.8e-7     1.0e-5   twin_spikes    1.6e-5      1.6e-5     1.0e-4   offset_up
#   any                              4.8e-5      4.8e-5     1.9e-4   offset_down (head_dim 64; closest to a bar: 2.6e-6 of 1.0e-5, stairs_down at 16)
#   any_train (rel)                  4.9e-5      4.9e-5     1.9e-4   offset_down    2.3e-4      2.3e-4     9.1e-4   late_spike_200 (head_dim 64)
#   h3_any                           1.6e-5      9.1e-6     3.7e-5   offset_up  (head_dim 32, the two-key slide; 5.8e-6 at head_dim 48)
#   token0_any                       5.0e-6      2.8e-6     1.1e-5   offset_up  (head_dim 48, the two-key slide)
#   wide_fwd (rel)                   1.2e-6      1.8e-5     7.2e-5   twin_spikes    2.9e-5      3.6e-5     1.4e-4   offset_up
#   token0_fwd (rel)                 2.2e-7      2.0e-7     1.0e-5   masked_max     7.1e-6      7.1e-6     1.0e-4   offset_up
#   token0_attention, special first  7.0e-7      2.8e-7     2.0e-6   offset_down
#   token0_attention, special last   2.9e-6      9.1e-7     3.6e-6   offset_down
#   rollout prepare + step           4.9e-6      1.0e-5     4.1e-5   spikes (special last); closest to a bar: 2.4e-6 of 1.5e-5, steps (special first)
#   token0_tail        ctx_out 7.2e-7 = 0.18 of 4 err32 + 4 ACT (err32 8.2e-7), 1.9e-6 of its element bound; logits 2.8e-7, 0.14
#   token0_tail_ws     ctx_out 1.9e-6 = 0.30 of 4 err32 + 4 ACT (err32 1.7e-6), 1.3e-4 of its element bound; logits 3.6e-7, 0.12
#                      (distributed and single-chain form alike)
# The token-major entries owe their yardsticks to the rounding of qscale q and of the sums: at scores of +-320 one ulp is 3e-5 log2
# units (paths_attention_any and _any_train land on the float32 formula's own error to three digits).  The two-key slide of offset_up is where h3_any and token0_any come closest: a dot product summed at magnitude 80 rounds
# six to eight times at 7.6e-6, which the same sum in float32 NumPy in the kernel's order reproduces to three digits (5.02e-6).

GEOMS = SP.GEOMS


def _L():
    from paths_amd import _lib
    return _lib


class Problem:
    """Inputs of one (bundle, geometry, head_dim, layout) with their float64 reference and float32 yardstick."""

    def __init__(self, bname, geom, hd, layout):
        self.names = SP.BUNDLES[bname]
        self.T, self.lens = GEOMS[geom]
        self.B, self.H, self.hd, self.d = len(self.lens), len(self.names), hd, len(self.names) * hd
        self.layout = layout
        q, k, v = SP.make_inputs(self.names, self.lens, self.T, hd)
        self.qscale = SP.qscale32(hd)
        if layout == "head":
            self.score_mul, self.qmul = LN2, 1.0
        else:
            q, self.qkv = SP.token_major(q, k, v, hd)
            self.score_mul, self.qmul = self.qscale * LN2, self.qscale
        self.q, self.k, self.v = q, k, v
        self.o64, self.lse64 = SP.reference(q, k, v, self.lens, self.score_mul)
        self.o32, self.lse32 = SP.formula_f32(q, k, v, self.lens, self.qmul)
        self.num_ims = torch.tensor([n - 1 for n in self.lens], dtype=torch.int64)

    def to(self, device, *names):
        return [getattr(self, n).to(device) for n in names]

    def heads(self, o_tok):
        """[B, T, H hd] (device) -> [B, H, T, hd] (CPU)"""
        return o_tok.view(self.B, self.T, self.H, self.hd).permute(0, 2, 1, 3).cpu()


@functools.lru_cache(maxsize=None)
def problem(bname, geom="base", hd=32, layout="head"):
    return Problem(bname, geom, hd, layout)


class Findings:
    """Every missed condition of a test, so that one run shows them all."""

    def __init__(self, label):
        self.label, self.bad = label, []

    def compare(self, pr, o, lse, base, rel=False, rows=None, o64=None, o32=None):
        """o [B, H, T, hd] (CPU) against pr.o64 over the first `rows` valid queries of every slide (None: all): finite, and per (slide,
        head) max|o - o64| (rel: over max|o64| of the slide) <= max(base, 4 x yardstick of the head's profile).  The yardstick is
        the same error of the float32 formula, the largest over the slides: a slide of one or two keys (or one query) is a single
        sample of a rounding error, not a measure of what fp32 can do on the profile.  lse likewise with LSE_BAR."""
        o64 = pr.o64 if o64 is None else o64
        o32 = pr.o32 if o32 is None else o32
        span = [(b, n, min(n, rows) if rows else n) for b, n in enumerate(pr.lens)]
        scale = [float(o64[b, :, :r].abs().max()) if rel else 1.0 for b, _, r in span]
        for h, name in enumerate(pr.names):
            yard = max(float((o32[b, h, :r].double() - o64[b, h, :r]).abs().max()) / scale[b] for b, _, r in span)
            yard_l = max(float((pr.lse32[b, h, :r].double() - pr.lse64[b, h, :r]).abs().max()) for b, _, r in span)
            bar, lbar = max(base, 4 * yard), max(LSE_BAR, 4 * yard_l)
            worst, worst_l = 0.0, 0.0
            for b, n, r in span:
                got = o[b, h, :r]
                if not bool(torch.isfinite(got).all()):
                    self.bad.append(f"{self.label} {name} slide {b} (len {n}): non-finite o")
                    continue
                e = float((got.double() - o64[b, h, :r]).abs().max()) / scale[b]
                worst = max(worst, e)
                if not e <= bar:
                    self.bad.append(f"{self.label} {name} slide {b} (len {n}): o err {e:.3e} > bar {bar:.3e} (float32 formula {yard:.3e})")
                if lse is None:
                    continue
                gl = lse[b, h, :r]
                if not bool(torch.isfinite(gl).all()):
                    self.bad.append(f"{self.label} {name} slide {b} (len {n}): non-finite lse")
                    continue
                el = float((gl.double() - pr.lse64[b, h, :r]).abs().max())
                worst_l = max(worst_l, el)
                if not el <= lbar:
                    self.bad.append(f"{self.label} {name} slide {b} (len {n}): lse err {el:.3e} > bar {lbar:.3e} (float32 formula {yard_l:.3e})")
            line = f"[softmax] {self.label} {name}: o {worst:.2e} (f32 {yard:.2e}, bar {bar:.1e})"
            if lse is not None:
                line += f" lse {worst_l:.2e} (f32 {yard_l:.2e}, bar {lbar:.1e})"
            print(line)

    def expect(self, ok, what):
        if not ok:
            self.bad.append(what)

    def check(self):
        assert not self.bad, self.label + ":\n" + "\n".join(self.bad)


def nan_like(device, *shape):
    return torch.full(shape, float("nan"), device=device)


# ================================================================================================
# head-major kernels: paths_attention_f32 / _x6 / _x6_dropout
# ================================================================================================
def x6_branch(planes, m32, drop_p, npairs, nq, cus=256):
    """The kernel attention_split (csrc/attn_x6.hip) launches: 'x6' = attn_x6_kernel (16x16x32; optimistic softmax at two planes without
    dropout, the deferred step otherwise), 'm32' = attn_m32_kernel, 'pair' = attn_m32p_kernel."""
    if drop_p > 0:
        return "x6"
    if planes == 2 and (m32 == 3 or (m32 == 2 and npairs * ((nq + 255) // 256) >= cus * 5 // 8)):
        return "pair"
    if planes == 2 and m32 == 1:
        return "m32"
    return "x6"


def run_x6(dev, pr, planes, m32, monkeypatch, drop_p=0.0):
    L = _L()
    p, st = L.ptr, L.stream()
    B, T, H, hd = pr.B, pr.T, pr.H, pr.hd
    q, k, v, num_ims = pr.to(dev, "q", "k", "v", "num_ims")
    ws = torch.empty((int(L.load().paths_attention_x6_workspace(B, T, H, hd, planes)),), device=dev, dtype=torch.uint8)
    o, lse = nan_like(dev, B, T, H * hd), nan_like(dev, B, H, T)
    monkeypatch.setenv("PATHS_ATTN_M32", str(m32))
    if drop_p > 0:
        L.call("paths_attention_x6_dropout", p(q), p(k), p(v), p(o), p(lse), p(num_ims), B, T, H, hd, 0, p(ws), planes, DROP_KEY, drop_p, st)
    else:
        L.call("paths_attention_x6", p(q), p(k), p(v), p(o), p(lse), p(num_ims), B, T, H, hd, 0, p(ws), planes, 0, st)
    torch.cuda.synchronize()
    return pr.heads(o), lse.cpu()


@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_attention_f32_on_profiles(dev, bname):
    """csrc/attn_f32.hip: the plain online softmax on the f32-input MFMA."""
    L = _L()
    p, st = L.ptr, L.stream()
    pr = problem(bname)
    B, T, H, hd = pr.B, pr.T, pr.H, pr.hd
    q, k, v, num_ims = pr.to(dev, "q", "k", "v", "num_ims")
    o, lse = nan_like(dev, B, T, H * hd), nan_like(dev, B, H, T)
    L.call("paths_attention_f32", p(q), p(k), p(v), p(o), p(lse), p(num_ims), B, T, H, hd, 0, st)
    torch.cuda.synchronize()
    F = Findings(f"f32 {bname}")
    F.compare(pr, pr.heads(o), lse.cpu(), X6_BAR)
    F.check()


@pytest.mark.parametrize("planes,m32,kernel", [(3, 0, "x6"), (2, 0, "x6"), (2, 1, "m32"), (2, 3, "pair")],
                         ids=["planes3", "planes2-m32_0", "planes2-m32_1", "planes2-m32_3"])
@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_attention_x6_on_profiles(dev, bname, planes, m32, kernel, monkeypatch):
    """paths_attention_x6: three planes (the deferred step: rescale only when a lane's maximum rises by more than 8), two planes on the
    16x16x32 kernel (m starts at 0, optimistic exp2, revision with the in-flight scores re-based), on the 32x32x16 kernel and on
    the wave pair (four-step ring, loader waves)."""
    pr = problem(bname)
    assert x6_branch(planes, m32, 0.0, pr.B * pr.H, pr.T) == kernel
    # no block of these slides takes the pair kernel's key-split path unless it has one key step (lengths 2 and 1)
    assert all(n - 256 * ((n - 1) // 256) > 32 or n <= 64 for n in pr.lens)
    o, lse = run_x6(dev, pr, planes, m32, monkeypatch)
    F = Findings(f"x6 planes {planes} M32={m32} {bname}")
    F.compare(pr, o, lse, X6_BAR)
    F.check()


@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_pair_kernel_key_split_on_profiles(dev, bname, monkeypatch):
    """The wave-pair kernel's small block: at most 32 queries, key steps kt = wave, wave + 12, .. per wave, the first step of each wave
    with a correction of either sign, partials merged through LDS with -1e30 as the neutral maximum (csrc/attn_x6.hip: `small`)."""
    pr = problem(bname, "split")
    assert x6_branch(2, 3, 0.0, pr.B * pr.H, pr.T) == "pair"
    tails = [(n, n - 256 * ((n - 1) // 256), (n + 63) // 64) for n in pr.lens]          # (len, queries of the last block, key steps)
    assert all(0 < left <= 32 for _, left, _ in tails)                                  # every slide ends in a key-split block
    assert any(steps > 12 for _, _, steps in tails) and any(steps < 12 for _, _, steps in tails)   # a wave with two steps; waves with none
    o, lse = run_x6(dev, pr, 2, 3, monkeypatch)
    F = Findings(f"x6 pair key-split {bname}")
    F.compare(pr, o, lse, X6_BAR)
    F.check()


def drop_mask(dev, pr, p):
    from tests.test_gpu_attention_backward import drop_mask as dm
    return dm(dev, pr.B, pr.H, pr.T, DROP_KEY, p, pr.T).cpu()


@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_attention_x6_dropout_on_profiles(dev, bname, planes, monkeypatch):
    """paths_attention_x6_dropout at p = 0.1: the deferred (not optimistic) step on fp16 and on bf16 planes, m from -inf; lse is the
    un-dropped softmax's.  The training forwards' bar: O_BAR relative to max|o| of the slide."""
    pr = problem(bname)
    assert x6_branch(planes, 2, 0.1, pr.B * pr.H, pr.T) == "x6"
    mask = drop_mask(dev, pr, 0.1)
    o64, _ = SP.reference(pr.q, pr.k, pr.v, pr.lens, pr.score_mul, mask)
    o32, _ = SP.formula_f32(pr.q, pr.k, pr.v, pr.lens, pr.qmul, mask)
    o, lse = run_x6(dev, pr, planes, 2, monkeypatch, drop_p=0.1)
    F = Findings(f"x6_dropout planes {planes} {bname}")
    F.compare(pr, o, lse, O_BAR, rel=True, o64=o64, o32=o32)
    F.check()


# ================================================================================================
# token-major kernels: paths_attention_any / _any_train / _h3_any / _wide_fwd / _token0_any; paths_attention_token0_fwd
# ================================================================================================
@pytest.mark.parametrize("hd", [16, 32, 48, 64])
@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_attention_any_h3_any_token0_any_on_profiles(dev, bname, hd):
    """paths_attention_any, _any_train (+ lse), _h3_any and _token0_any on the token-major in_proj output.  attn_h3_any.hip: a block
    with at most 32 queries left (len - 128 k <= 32) and head_dim <= 48 splits the key steps over its four waves and merges with
    -inf as the neutral maximum; every other block runs the one-wave loop."""
    L = _L()
    p, st = L.ptr, L.stream()
    pr = problem(bname, "base", hd, "token")
    B, T, H, d = pr.B, pr.T, pr.H, pr.d
    qkv, num_ims = pr.to(dev, "qkv", "num_ims")
    left = [n - 128 * ((n - 1) // 128) for n in pr.lens]
    merged = [n for n, lf in zip(pr.lens, left) if lf <= 32 and hd <= 48]
    if hd <= 48:
        assert any(n > 256 for n in merged) and any(lf > 32 for lf in left)      # both forms run; a merge over seven key steps (385)
    else:
        assert not merged
    F = Findings(f"any hd {hd} {bname}")
    o = nan_like(dev, B, T, d)
    L.call("paths_attention_any", p(qkv), 3 * d, p(o), p(num_ims), B, T, H, hd, pr.qscale, 0, st)
    torch.cuda.synchronize()
    F.compare(pr, pr.heads(o), None, ANY_BAR)
    F.label = f"any_train hd {hd} {bname}"
    o, lse = nan_like(dev, B, T, d), nan_like(dev, B, H, T)
    L.call("paths_attention_any_train", p(qkv), 3 * d, p(o), p(lse), p(num_ims), B, T, H, hd, pr.qscale, 0, 0, 0.0, st)
    torch.cuda.synchronize()
    F.compare(pr, pr.heads(o), lse.cpu(), O_BAR, rel=True)
    F.label = f"h3_any hd {hd} {bname}"
    o = nan_like(dev, B, T, d)
    ws = torch.empty((int(L.load().paths_attention_h3_any_workspace(B, T, H, hd)),), device=dev, dtype=torch.uint8)
    L.call("paths_attention_h3_any", p(qkv), 3 * d, p(o), p(num_ims), B, T, H, hd, pr.qscale, p(ws), st)
    torch.cuda.synchronize()
    F.compare(pr, pr.heads(o), None, ANY_BAR)
    F.label = f"token0_any hd {hd} {bname}"
    a0 = nan_like(dev, B, d)
    ws0 = torch.empty((int(L.load().paths_attention_token0_workspace(B, T, H)),), device=dev)
    L.call("paths_attention_token0_any", p(qkv), 3 * d, p(num_ims), p(a0), p(ws0), B, T, H, hd, pr.qscale, st)
    torch.cuda.synchronize()
    o0 = nan_like("cpu", B, H, T, hd)
    o0[:, :, 0] = a0.view(B, H, hd).cpu()
    F.compare(pr, o0, None, T0_BAR, rows=1)
    F.check()


@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_attention_wide_fwd_on_profiles(dev, bname):
    """paths_attention_wide_fwd (head_dim 96): scores in scratch, two passes, no running state - the control.  (It used to normalise
    with exp2(qscale S - lse): on late_spike_200 / masked_max_200, a maximum of 200 .. 400, the rounding of lse moved every P by
    1.06e-5 of max|o| against the bar of 1e-5 and a float32 formula at 7e-8; the forward now divides by the sum it took.)"""
    L = _L()
    p, st = L.ptr, L.stream()
    pr = problem(bname, "base", 96, "token")
    B, T, H, hd, d = pr.B, pr.T, pr.H, pr.hd, pr.d
    qkv, num_ims = pr.to(dev, "qkv", "num_ims")
    o, lse = nan_like(dev, B, T, d), nan_like(dev, B, H, T)
    ws = torch.empty((int(L.load().paths_attention_wide_workspace(T, hd)),), device=dev)
    L.call("paths_attention_wide_fwd", p(qkv), 3 * d, p(o), p(lse), p(num_ims), B, T, H, hd, pr.qscale, 0, 0, 0.0, p(ws), st)
    torch.cuda.synchronize()
    F = Findings(f"wide_fwd {bname}")
    F.compare(pr, pr.heads(o), lse.cpu(), O_BAR, rel=True)
    F.check()


@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_attention_token0_fwd_on_profiles(dev, bname):
    """paths_attention_token0_fwd (head-major, training): four key splits of 128 keys at these shapes (pick_splits), merged with -inf
    as the neutral maximum; a0 within O_BAR of the slide's max|o|, lse0 within LSE_BAR."""
    L = _L()
    p, st = L.ptr, L.stream()
    pr = problem(bname)
    B, T, H, hd, d = pr.B, pr.T, pr.H, pr.hd, pr.d
    q, k, v, num_ims = pr.to(dev, "q", "k", "v", "num_ims")
    a0, lse0 = nan_like(dev, B, d), nan_like(dev, B, H)
    ws = torch.empty((int(L.load().paths_attention_token0_workspace(B, T, H)),), device=dev)
    L.call("paths_attention_token0_fwd", p(q), p(k), p(v), p(num_ims), p(a0), p(lse0), p(ws), B, T, H, hd, 0, 0.0, st)
    torch.cuda.synchronize()
    o0, l0 = nan_like("cpu", B, H, T, hd), nan_like("cpu", B, H, T)
    o0[:, :, 0], l0[:, :, 0] = a0.view(B, H, hd).cpu(), lse0.cpu()
    F = Findings(f"token0_fwd {bname}")
    F.compare(pr, o0, l0, O_BAR, rel=True, rows=1)
    F.check()


# ================================================================================================
# fused single-query attention: paths_token0_tail (q, k, v) and paths_token0_tail_ws (in_proj folded into the query)
# ================================================================================================
def report2(F, name, got, ref64, tol, ref32, nact):
    """The two conditions of tests/test_gpu_chain_forward.py for an output behind the row chain: the per-element bound chain_ref
    propagates, and err <= 4 err32 + ACT n (err32: the same formula in float32 torch)."""
    if not bool(torch.isfinite(got).all()):
        F.bad.append(f"{name}: non-finite values")
        return
    err = (got.double() - ref64).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())
    e, e32 = float(err.max()), float((ref32.double() - ref64).abs().max())
    bound2 = 4 * e32 + R.ACT * nact
    print(f"[softmax] {F.label} {name}: {e:.2e} = {ratio:.2e} of its element bound, {e / bound2:.2f} of 4 x f32 ({e32:.2e}) + {nact} ACT")
    F.expect(ratio <= 1.0, f"{name}: {ratio:.3f} of the per-element bound (max err {e:.3e})")
    F.expect(e <= bound2, f"{name}: err {e:.3e} > 4 * {e32:.3e} + {nact} * ACT")


@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_token0_tail_on_profiles(dev, bname):
    """paths_token0_tail (csrc/tlayer_f32.hip): 16 key partitions of 64 keys at these lengths, per-lane online softmax, wave merge, then
    the partitions' merge (-inf neutral); ctx_out and logits behind the row chain against chain_ref.token0_tail_ref on the same
    q, k, v.  The attention's own error reaches ctx_out through out_proj (weights of 0.1) and three LayerNorms of gain ~1."""
    from tests.test_gpu_aggregator_forward import _f64, _layers, _tail_buffers, _tail_call
    pr = problem(bname)
    B, T, d = pr.B, pr.T, 128
    assert pr.d == d and pr.hd == 32
    layers, lvl = _layers(d)
    g = torch.Generator().manual_seed(4242)
    rnd = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(dev)
    q, k, v, num_ims = pr.to(dev, "q", "k", "v", "num_ims")
    tp = {"x": rnd(B, T, d), "B": B, "T": T, "depth": 0, "num_ims": num_ims, "ctx_prev": rnd(B, d + 4), "ctx_all": None,
          "wcls": (rnd(4, d) * 0.1).contiguous(), "bcls": rnd(4) * 0.1, "q": q, "k": k, "v": v}
    refs = {}
    for tag, cast in (("64", lambda t: t.double()), ("32", lambda t: t)):
        l1 = {kk: (cast(vv) if torch.is_tensor(vv) else vv) for kk, vv in layers[1].items() if "image" not in kk}
        lv = {"lnfg": cast(lvl["lnfg"]), "lnfb": cast(lvl["lnfb"]), "lnf_eps": 1e-5, "wcls": cast(tp["wcls"]), "bcls": cast(tp["bcls"])}
        refs[tag] = R.token0_tail_ref(l1, lv, cast(tp["x"]), num_ims, pr.H, cast(tp["ctx_prev"][:, :d]), None,
                                      qkv=(cast(q), cast(k), cast(v)), qk_scale=LN2)
    bufs = _tail_buffers(tp)
    _tail_call(tp, bufs)
    torch.cuda.synchronize()
    (c64, l64, tc, tl), (c32, l32, _, _) = refs["64"], refs["32"]
    F = Findings(f"token0_tail {bname}")
    report2(F, "ctx_out", bufs["ctx_out"][:B * d].view(B, d), c64, tc, c32, R.TAIL_ACTIVATIONS["ctx_out"])
    report2(F, "logits", bufs["logits"][:B * 4].view(B, 4), l64, tl, l32, R.TAIL_ACTIVATIONS["logits"])
    F.check()


def carrier_rows(pr, dev):
    """x [B, T, 128] and an in_proj (wqkv [384, 128], bqkv [384]) whose q and k carry the problem's profile: column h of x holds head
    h's key carrier f, column 4 + h the query carrier g / qscale, columns 8 + 30 h .. + 29 the head's 30 noise dimensions (shared by
    q and k: q_i . k_j = g f + x_i . x_j over them); Wq / Wk pick those columns (rows of 0 / 1, zero bias), so q and k are exact.  Wv
    is random with zeros in the eight carrier columns (v stays O(1))."""
    assert pr.layout == "token" and pr.hd == 32 and pr.H == 4
    B, T, d = pr.B, pr.T, 128
    x = torch.zeros((B, T, d))
    wqkv = torch.zeros((3 * d, d))
    for h in range(4):
        x[:, :, h] = pr.k[:, h, :, 0]
        x[:, :, 4 + h] = pr.q[:, h, :, 0]
        x[:, :, 8 + 30 * h:38 + 30 * h] = pr.k[:, h, :, 1:31]
        wqkv[32 * h, 4 + h] = 1.0
        wqkv[d + 32 * h, h] = 1.0
        for e in range(30):
            wqkv[32 * h + 1 + e, 8 + 30 * h + e] = 1.0
            wqkv[d + 32 * h + 1 + e, 8 + 30 * h + e] = 1.0
    g = torch.Generator().manual_seed(99)
    wv = (torch.rand((d, d), generator=g) * 2 - 1) * 0.15
    wv[:, :8] = 0.0
    wqkv[2 * d:] = wv
    bqkv = torch.zeros(3 * d)
    bqkv[2 * d:] = (torch.rand(d, generator=g) * 2 - 1) * 0.1
    return x.to(dev), wqkv.to(dev), bqkv.to(dev)


@pytest.mark.parametrize("form,special_last", [("distributed", 0), ("distributed", 1), ("chain", 0)])
@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_token0_tail_ws_on_profiles(dev, bname, form, special_last):
    """paths_token0_tail_ws (csrc/token0_ws.hip): K / V projections folded into the query, (token split, head) workgroups publish
    (max, sum, z) partials of 128 tokens that are merged - by every workgroup of the slide in the distributed form (the nine slides:
    four splits each), by the last arriver in the single-chain form (the same slides six times over: 216 workgroups do not fit the
    distributed form's 192).  The in_proj is chosen so that the folded query and the rows carry the profile (carrier_rows); ctx_out
    and logits against chain_ref.token0_tail_ref on the same x and weights.  special_last: the query is the slide's last valid row."""
    from paths_amd import ops
    from tests.test_gpu_aggregator_forward import _layers
    L = _L()
    pr = problem(bname, "base", 32, "token")
    T, d, H = pr.T, 128, 4
    x, wqkv, bqkv = carrier_rows(pr, dev)
    num_ims = pr.num_ims.to(dev)
    if form == "chain":
        x, num_ims = x.repeat(6, 1, 1), num_ims.repeat(6)
    B = x.shape[0]
    assert bool(L.load().paths_token0_ws_supported(B, T, d, H))
    # which form the launcher takes shows in the scratch it asks for (csrc/token0_ws.hip: dist_splits, chain_splits)
    floats = int(L.load().paths_token0_ws_partials_d(B, T, d))
    assert floats == (B * (H * 4 * (4 + d + d) + d) if form == "distributed" else B * H * 4 * (4 + d)), (form, floats)
    layers, lvl = _layers(d)
    lay = {kk: vv for kk, vv in layers[1].items() if "image" not in kk}
    lay["wqkv"], lay["bqkv"] = wqkv, bqkv
    g = torch.Generator().manual_seed(4343)
    rnd = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(dev)
    ctx_prev, wcls, bcls = rnd(B, d), (rnd(4, d) * 0.1).contiguous(), rnd(4) * 0.1
    refs = {}
    for tag, cast in (("64", lambda t: t.double()), ("32", lambda t: t)):
        l1 = {kk: (cast(vv) if torch.is_tensor(vv) else vv) for kk, vv in lay.items()}
        lv = {"lnfg": cast(lvl["lnfg"]), "lnfb": cast(lvl["lnfb"]), "lnf_eps": 1e-5, "wcls": cast(wcls), "bcls": cast(bcls)}
        refs[tag] = R.token0_tail_ref(l1, lv, cast(x), num_ims, H, cast(ctx_prev), None, special_last=bool(special_last))
    pack = {"layers": [dict(lay)], "lnfg": lvl["lnfg"], "lnfb": lvl["lnfb"], "lnf_eps": 1e-5, "wcls": wcls, "bcls": bcls}
    ctx_out, logits = nan_like(dev, B, d), nan_like(dev, B, 4)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.token0_tail_ws(pack, x, num_ims, (ctx_prev, None, 0, ctx_out, logits), status, B, T, d, H, pr.qscale, special_last)
    torch.cuda.synchronize()
    (c64, l64, tc, tl), (c32, l32, _, _) = refs["64"], refs["32"]
    F = Findings(f"token0_tail_ws {form} special_last {special_last} {bname}")
    F.expect(int(status.item()) == 0, f"status {int(status.item())}")
    report2(F, "ctx_out", ctx_out, c64, tc, c32, R.TAIL_ACTIVATIONS["ctx_out"])
    report2(F, "logits", logits, l64, tl, l32, R.TAIL_ACTIVATIONS["logits"])
    F.check()


# ================================================================================================
# exports with a running state of their own: paths_token0_attention, paths_attention_rollout_prepare (+ step)
# ================================================================================================
def layer_attention32(x, num_ims, w_in, b_in, nhead):
    """rollout_ref.layer_attention64 in float32 (CPU): per slide the [H, n + 1, n + 1] softmax attention over its valid rows."""
    B, T, d = x.shape
    hd = d // nhead
    out = []
    for b in range(B):
        n = int(num_ims[b])
        rows = x[b, :n + 1]
        q = rows @ w_in[:d].T + b_in[:d]
        k = rows @ w_in[d:2 * d].T + b_in[d:2 * d]
        q, k = (t.reshape(n + 1, nhead, hd).transpose(0, 1) for t in (q, k))
        out.append(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1))
    return out


@pytest.mark.parametrize("special_last", [0, 1])
@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_token0_attention_on_profiles(dev, bname, special_last):
    """paths_token0_attention: the special token's probabilities over key splits merged in a fixed order, from x and the true in_proj;
    against the float64 restatement of tests/test_gpu_token0_attention.py at its bar (2e-6 absolute on a probability), padding
    exactly 0, rows summing to 1."""
    from tests.test_gpu_token0_attention import ref_attention, run_kernel
    pr = problem(bname, "base", 32, "token")
    B, T, H = pr.B, pr.T, 4
    x, wqkv, bqkv = carrier_rows(pr, dev)
    num_ims = pr.num_ims
    patch, self_ = run_kernel(dev, x, num_ims.to(dev), wqkv, bqkv, H, special_last)
    xc, wc, bc = x.cpu(), wqkv.cpu(), bqkv.cpu()
    rp, rs = ref_attention(xc.numpy(), num_ims.numpy(), wc.numpy(), bc.numpy(), H, special_last)
    xs = rollout_ref.canonical_rows(xc, num_ims, special_last)
    a32 = layer_attention32(xs, num_ims, wc, bc, H)
    F = Findings(f"token0_attention special_last {special_last} {bname}")
    F.expect(bool(torch.isfinite(patch).all() and torch.isfinite(self_).all()), "non-finite probabilities")
    for h, name in enumerate(pr.names):
        errs, yards = [], []
        for b, n in enumerate(pr.lens):
            got = np.concatenate(([float(self_[b, h])], patch[b, h, :n - 1].numpy().astype(np.float64)))
            ref = np.concatenate(([rs[b, h]], rp[b, h, :n - 1]))
            errs.append(float(np.abs(got - ref).max()))
            yards.append(float(np.abs(a32[b][h, 0].double().numpy() - ref).max()))
            F.expect(bool((patch[b, h, n - 1:] == 0).all()), f"{name} slide {b}: padding not exactly 0")
        bar = max(T0_BAR, 4 * max(yards))                      # (the yardstick of the profile: the largest over its slides)
        for b, (n, e) in enumerate(zip(pr.lens, errs)):
            F.expect(e <= bar, f"{name} slide {b} (len {n}): err {e:.3e} > bar {bar:.3e} (float32 formula {max(yards):.3e})")
        print(f"[softmax] {F.label} {name}: p {max(errs):.2e} (f32 {max(yards):.2e}, bar {bar:.1e})")
    tot = patch.double().sum(-1) + self_.double()
    F.expect(float((tot - 1).abs().max()) <= 1e-5, "rows do not sum to 1")
    F.check()


@pytest.mark.parametrize("special_last", [0, 1])
@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_rollout_prepare_on_profiles(dev, bname, special_last):
    """paths_attention_rollout_prepare: the (m, l) of EVERY query row over 64-key tiles (per-lane online state, then a merge over the four
    lane groups with -inf neutral), read through one paths_attention_rollout_step of a random r_in; against rollout_ref.step64 at
    the bar of tests/test_gpu_attention_rollout.py (2e-6), rows past num_ims exactly 0, mass kept."""
    from tests.test_gpu_attention_rollout import run_step
    pr = problem(bname, "base", 32, "token")
    B, T, H = pr.B, pr.T, 4
    x, wqkv, bqkv = carrier_rows(pr, dev)
    num_ims = pr.num_ims
    g = torch.Generator().manual_seed(77)
    r_in = torch.rand((B, T), generator=g)
    for b, n in enumerate(pr.lens):
        r_in[b, n:] = 0.0
    got = run_step(dev, x, num_ims.to(dev), wqkv, bqkv, H, special_last, r_in.to(dev))
    xc, wc, bc = x.cpu(), wqkv.cpu(), bqkv.cpu()
    want = rollout_ref.step64(xc, num_ims, wc, bc, H, special_last, r_in)
    a32 = layer_attention32(rollout_ref.canonical_rows(xc, num_ims, special_last), num_ims, wc, bc, H)
    F = Findings(f"rollout special_last {special_last} {bname}")
    F.expect(bool(torch.isfinite(got).all()), "non-finite rollout")
    errs, yards = [], []
    for b, n in enumerate(pr.lens):
        y32 = 0.5 * r_in[b, :n] + 0.5 * (r_in[b, :n] @ a32[b].mean(0))
        errs.append(float((got[b, :n].double() - want[b, :n]).abs().max()))
        yards.append(float((y32.double() - want[b, :n]).abs().max()))
        F.expect(bool((got[b, n:] == 0).all()), f"slide {b}: rows past num_ims not exactly 0")
    bar = max(T0_BAR, 4 * max(yards))                          # (r_out mixes the four heads' profiles: one yardstick per case)
    for b, (n, e) in enumerate(zip(pr.lens, errs)):
        F.expect(e <= bar, f"slide {b} (len {n}): err {e:.3e} > bar {bar:.3e} (float32 formula {max(yards):.3e})")
    print(f"[softmax] {F.label}: r_out {max(errs):.2e} (f32 {max(yards):.2e}, bar {bar:.1e})")
    F.expect(float((got.double().sum(1) - r_in.double().sum(1)).abs().max()) <= 1e-5 * max(1.0, float(r_in.sum(1).max())), "mass not kept")
    F.check()
