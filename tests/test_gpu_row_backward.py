"""The row-wise backward kernels, the slab reductions and the gradients passed between levels, each called directly through the C ABI
and checked against the float64 references of tests/rows_ref.py at ragged shapes: slides with 0, 1, N - 1 and N patches, widths
that are not multiples of the kernels' strides, splits that leave slabs empty, saturated gates and ill-conditioned LayerNorm rows.

Per case:
  accuracy      element-wise outputs: max|g - ref| / max|ref| per slide (LayerNorm: per row family) and per output; sums (dgamma,
                dbeta, colsum(dx), colsum, slab partials, da): |g - ref| / sum|terms|, so a cancelling sum is judged by its
                conditioning and not by how small its result is;
  padding       padded rows come back zero while their inputs hold large finite garbage - and, in the *_ignores_what_padded_rows_hold
                tests, bit-identical outputs when they hold NaN / Inf instead (hostile_rows) - and what the contract leaves alone keeps a
                sentinel (the other kernel's columns of dG, the h half of d_state_prev, rows of parents that were not kept);
  determinism   two launches give bit-identical outputs (no atomics here: a difference is a race);
  sensitivity   the same outputs measured against a wrong reference (the longest slide's num_ims cut by one, r / m planes swapped,
                LayerNorm variance over d - 1, a sum missing its last row or slab) miss the bar by at least 10x.
The gradients between levels are at most four fp32 adds in block order: they are compared for bit equality.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H
from tests import rows_ref as R
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = -7.25
GARBAGE = 3.0e4          # large finite values in the rows the kernels must not use

# Bars, at most 4x the worst value measured on one MI355X over this file's cases (in the comment).
BAR = {
    "lstm_a": 5.6e-7,        # worst 1.44e-7 (dpre_o, N = 2049, D = 1536)
    "lstm_b": 4e-7,          # worst 9.98e-8 (dgates, N = 2049, Hc = 96)
    "imp_elem": 2.1e-7,      # worst 5.46e-8 (dP, any, Hi = 96, d = 192)
    "imp_dot": 2.8e-7,       # worst 7.24e-8 (dah, any, Hi = 36, d = 64); da, dhid, dah against the conditioning of g . P
    "imp_rows_dot": 4e-7,    # worst 1.01e-7 (dh, any, Hi = 36, D = 132, N = 2049)
    "ln_fwd": 3.6e-6,        # worst 9.19e-7 (xhat, d = 2044); absolute on xhat, relative on rstd and y
    "ln_bwd": 5.6e-7,        # worst 1.43e-7 (dx, d = 192, 4097 rows)
    "ln_sum": 5.4e-7,        # worst 1.35e-7 (slab sums of dy xhat, d = 1536, rows_per_block 7); dgamma / dbeta / colsum(dx) <= 1.24e-7
    "ln_chain": 6.4e-7,      # worst 1.67e-7 (dx, d = 1540)
    "colsum": 7.2e-7,        # worst 1.86e-7 (slab partials, N = 1792, scalar kernel)
}
ILL_RATIO = 4.0          # ill-conditioned LayerNorm rows: kernel error within 4x of fp32 torch's on the same inputs


def _lib():
    from paths_amd import _lib as L
    return L


def P(t):
    return None if t is None else t.data_ptr()


def sync():
    torch.cuda.synchronize()


def elem_err(got, ref, groups):
    """max over groups of max|g - ref| / max|ref| over the group's rows; groups: list of row index tensors / slices of dim 0.
    A group whose reference is exactly zero is measured against the largest reference value overall."""
    scale = float(ref.abs().max()) or 1.0
    worst = 0.0
    for gi in groups:
        r, g = ref[gi], got[gi]
        if r.numel() == 0:
            continue
        den = float(r.abs().max()) or scale
        worst = max(worst, float((g.double() - r).abs().max()) / den)
    return worst


def sum_err(got, ref, terms):
    """max |g - ref| / sum|terms| over the elements; where the terms are all zero the result must be exactly zero."""
    diff = (got.double() - ref).abs()
    zero = terms == 0
    if bool((diff[zero] != 0).any()):
        return math.inf
    return float((diff[~zero] / terms[~zero]).max()) if bool((~zero).any()) else 0.0


def slide_groups(num_ims, N):
    return [slice(b * N, b * N + int(n)) for b, n in enumerate(num_ims) if int(n) > 0]


def longest(num_ims):
    return max(range(len(num_ims)), key=lambda b: int(num_ims[b]))


def cut_one(num_ims):
    """num_ims with the longest slide's count cut by one"""
    n = list(num_ims)
    n[longest(n)] -= 1
    return n


def saturate(g, x, lo, hi, frac=0.1):
    """x with a fraction of its entries replaced by values at and next to the saturation points lo and hi (exact and 1 ulp inside)"""
    eps = torch.finfo(torch.float32).eps
    vals = torch.tensor([lo, hi, lo + abs(lo) * eps + (eps if lo == 0 else 0), hi - abs(hi) * eps / 2, 1e-30 + lo], device=x.device)
    pick = torch.rand(x.shape, device=x.device, generator=g) < frac
    idx = torch.randint(0, len(vals), x.shape, device=x.device, generator=g)
    return torch.where(pick, vals[idx], x)


def rnd(g, *shape, lo=-1.0, hi=1.0):
    return torch.rand(*shape, device="cuda", generator=g) * (hi - lo) + lo


def garbage_rows(x, valid):
    """x with the padded rows (dim 0) replaced by large finite values"""
    gar = GARBAGE * torch.sign(torch.randn_like(x)) * (1 + torch.rand_like(x))
    return torch.where(valid.view(-1, *([1] * (x.dim() - 1))), x, gar)


def hostile_rows(x, valid):
    """x with the padded rows (dim 0) replaced by the hostile pattern of tests/poison.py: NaN, +Inf, -Inf and 3e38 in a cycle.  Finite
    garbage passes whether a kernel masks with a select or with a multiplication; this passes only with a select."""
    from tests import poison
    bad = poison.fill_(torch.zeros_like(x).contiguous(), "H")
    return torch.where(valid.view(-1, *([1] * (x.dim() - 1))), x, bad)


def gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


# ---------------------------------------------------------------------------------------------------------------------------------
# the padded rows of every input: finite garbage and the hostile pattern give the same bits
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(label, a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x is None:
            assert y is None
            continue
        assert torch.isfinite(y).all(), f"{label}: output {i} is not finite with NaN / Inf in the padded rows"
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{label}: output {i} depends on what the padded rows hold"


@pytest.mark.parametrize("N,D,Hc", [(7, 1024, 32), (160, 1536, 96)])
def test_lstm_bwd_ignores_what_padded_rows_hold(dev, N, D, Hc):
    """paths_lstm_bwd_a / _b with d_state_out and a strided c0 / dc0: dy, o, tc, f|r|m, dc1, d_state_out and state_prev rows behind a
    slide's last patch hold large finite values, then NaN / Inf.  Every output (padded rows exactly zero) is bit-identical."""
    L = _lib()
    st = L.stream()
    g = gen(dev, N + D + Hc)
    num_ims = [N - 1, 0, N, 1]
    B = len(num_ims)
    M, Dp, G = B * N, D + Hc, 3 * Hc + D
    nims = torch.tensor(num_ims, device=dev, dtype=torch.int64)
    valid = R.valid_rows(nims, N)
    clean = {"dy": rnd(g, M, D), "o": rnd(g, M, D, lo=0.0), "tc": rnd(g, M, D), "frm": rnd(g, M, 3 * Hc), "dc1_h": rnd(g, M, Hc),
             "dso": rnd(g, M, Dp), "sp": rnd(g, M, Dp)}

    def run(rows):
        t = {k: rows(v, valid).contiguous() for k, v in clean.items()}
        dG, dpre_h, dsp = (torch.full(s, SENTINEL, device=dev) for s in ((M, G), (M, D), (M, Dp)))
        L.call("paths_lstm_bwd_a", P(t["dy"]), D, P(t["dso"]), Dp, P(t["o"]), P(t["tc"]), P(nims), N, M, D, P(dG) + 4 * 3 * Hc, G, P(dpre_h), st)
        L.call("paths_lstm_bwd_b", P(t["dc1_h"]), P(t["dso"]) + 4 * D, Dp, P(t["frm"]), P(t["sp"]) + 4 * D, Dp, P(nims), N, M, Hc, P(dG), G,
               P(dsp) + 4 * D, Dp, st)
        sync()
        return dG, dpre_h, dsp[:, D:].contiguous()

    fin, hos = run(garbage_rows), run(hostile_rows)
    _same(f"lstm_bwd N={N}", fin, hos)
    assert not hos[0][~valid].any() and not hos[1][~valid].any() and not hos[2][~valid].any()


@pytest.mark.parametrize("Hi,d,extra,imp_mul,N", [(128, 128, 0, 1, 160), (128, 128, 0, 0, 7), (36, 64, 0, 1, 160), (96, 192, 32, 0, 7)])
def test_importance_bwd_ignores_what_padded_rows_hold(dev, Hi, d, extra, imp_mul, N):
    """paths_importance_bwd / _any: the dtok rows of padded patches and of the special token, as in test_importance_bwd_vs_fp64 (pproj
    and hid are saved activations, finite in every row; alpha is 0 in padded rows by the forward's mask)."""
    L = _lib()
    st = L.stream()
    g = gen(dev, Hi + d + N)
    num_ims = [N - 1, 0, N, 1]
    M, nims, valid, hid, alpha, w2 = _imp_inputs(g, dev, num_ims, N, Hi, d)
    B = len(num_ims)
    fast = (Hi, d, extra) == (128, 128, 0)
    U = (Hi + d + 31) // 32 * 32 + extra
    tv = torch.cat((torch.zeros(B, 1, dtype=torch.bool, device=dev), valid.view(B, N)), 1).reshape(-1)      # row 0 of dtok: the special token's, not read
    dtok0, pproj0 = rnd(g, B * (N + 1), d), rnd(g, M, d)

    def run(rows):
        dtok, pproj, h = rows(dtok0, tv).contiguous(), pproj0, hid
        du, da, dah = (torch.full(s, SENTINEL, device=dev) for s in ((M, U), (M,), (M, Hi)))
        if fast:
            L.call("paths_importance_bwd", P(dtok), P(pproj), P(h), P(alpha), P(w2), P(nims), N, M, imp_mul, P(du), P(da), P(dah), st)
        else:
            L.call("paths_importance_bwd_any", P(dtok), P(pproj), P(h), P(alpha), P(w2), P(nims), N, M, imp_mul, Hi, d, U, P(du), P(da), P(dah), st)
        sync()
        return du, da, dah

    fin, hos = run(garbage_rows), run(hostile_rows)
    _same(f"importance_bwd Hi={Hi} d={d}", fin, hos)
    assert not hos[0][~valid].any() and not hos[1][~valid].any() and not hos[2][~valid].any()


@pytest.mark.parametrize("Hi,D,N", [(128, 1024, 160), (128, 1028, 7), (36, 132, 160), (200, 1024, 1)])
def test_importance_rows_bwd_ignores_what_padded_rows_hold(dev, Hi, D, N):
    """paths_importance_rows_bwd / _any: the dZ and X rows of padded patches, as in test_importance_rows_bwd_vs_fp64 - the kernel reads
    every row's dot product and must SELECT zero for a padded row, not multiply by it."""
    L = _lib()
    st = L.stream()
    g = gen(dev, Hi + D + N)
    num_ims = [N - 1, 0, N, 1]
    M, nims, valid, hid, alpha, w2 = _imp_inputs(g, dev, num_ims, N, Hi, D)
    dz0, x0 = rnd(g, M, D), rnd(g, M, D)

    def run(rows):
        dz, x, h = rows(dz0, valid).contiguous(), rows(x0, valid).contiguous(), hid
        dh, da, dah = (torch.full(s, SENTINEL, device=dev) for s in ((M, Hi), (M,), (M, Hi)))
        if Hi == 128:
            L.call("paths_importance_rows_bwd", P(dz), P(x), D, P(h), P(alpha), P(w2), P(nims), N, M, P(dh), P(da), P(dah), st)
        else:
            L.call("paths_importance_rows_bwd_any", P(dz), P(x), D, P(h), P(alpha), P(w2), P(nims), N, M, Hi, P(dh), P(da), P(dah), st)
        sync()
        return dh, da, dah

    fin, hos = run(garbage_rows), run(hostile_rows)
    _same(f"importance_rows_bwd Hi={Hi} D={D}", fin, hos)
    assert not hos[0][~valid].any() and not hos[1][~valid].any() and not hos[2][~valid].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# LSTM phases a and b, run into one [M, 3 Hc + D] dG as production does
# ---------------------------------------------------------------------------------------------------------------------------------
# N, D, Hc, d_state_out given, c0 form, dc0 form
LSTM_CASES = [(1, 1024, 32, False, "null", "null"), (7, 1536, 96, True, "strided", "strided"), (160, 1024, 256, True, "contig", "contig"),
              (2049, 1024, 256, False, "strided", "strided"), (2049, 1536, 96, True, "contig", "null"), (7, 1024, 256, True, "null", "contig"),
              (160, 1536, 32, False, "contig", "strided")]


@pytest.mark.parametrize("N,D,Hc,ext,c0_form,dc0_form", LSTM_CASES,
                         ids=[f"N{n}-D{d}-Hc{h}-{'ext' if e else 'noext'}-c0{c}-dc0{dc}" for n, d, h, e, c, dc in LSTM_CASES])
def test_lstm_bwd_vs_fp64(dev, N, D, Hc, ext, c0_form, dc0_form):
    L = _lib()
    st = L.stream()
    g = gen(dev, N * 31 + D + Hc)
    num_ims = [N - 1, 0, N, 1]
    B = len(num_ims)
    M, Dp, G = B * N, D + Hc, 3 * Hc + D
    nims = torch.tensor(num_ims, device=dev, dtype=torch.int64)
    valid = R.valid_rows(nims, N)
    dy = garbage_rows(rnd(g, M, D), valid)
    o = garbage_rows(saturate(g, rnd(g, M, D, lo=0.0), 0.0, 1.0), valid)
    tc = garbage_rows(saturate(g, rnd(g, M, D), -1.0, 1.0), valid)
    f, r = (saturate(g, rnd(g, M, Hc, lo=0.0), 0.0, 1.0) for _ in range(2))
    m = saturate(g, rnd(g, M, Hc), -1.0, 1.0)
    frm = garbage_rows(R.pack_gates(f, r, m).contiguous(), valid)
    dc1_h = garbage_rows(rnd(g, M, Hc), valid)
    d_state_out = garbage_rows(rnd(g, M, Dp), valid).view(B, N, Dp) if ext else None
    state_prev = garbage_rows(rnd(g, M, Dp), valid) if c0_form == "strided" else None
    c0 = {"null": None, "strided": None if state_prev is None else state_prev[:, D:], "contig": garbage_rows(rnd(g, M, Hc), valid)}[c0_form]
    c0_ptr, ldc0 = {"null": (None, 0), "strided": (P(state_prev) + 4 * D if state_prev is not None else None, Dp), "contig": (P(c0), Hc)}[c0_form]

    def run(a=True, b=True):
        dG = torch.full((M, G), SENTINEL, device=dev)
        dpre_h = torch.full((M, D), SENTINEL, device=dev)
        dsp = torch.full((M, Dp), SENTINEL, device=dev) if dc0_form == "strided" else None
        dc0 = torch.full((M, Hc), SENTINEL, device=dev) if dc0_form == "contig" else None
        dc0_ptr, lddc0 = {"null": (None, 0), "strided": (P(dsp) + 4 * D if dsp is not None else None, Dp), "contig": (P(dc0), Hc)}[dc0_form]
        if a:
            L.call("paths_lstm_bwd_a", P(dy), D, P(d_state_out), Dp, P(o), P(tc), P(nims), N, M, D, P(dG) + 4 * 3 * Hc, G, P(dpre_h), st)
        if b:
            L.call("paths_lstm_bwd_b", P(dc1_h), P(d_state_out) + 4 * D if ext else None, Dp, P(frm), c0_ptr, ldc0, P(nims), N, M, Hc,
                   P(dG), G, dc0_ptr, lddc0, st)
        sync()
        return dG, dpre_h, dsp, dc0

    dG, dpre_h, dsp, dc0 = run()
    dG2, dpre_h2, dsp2, dc02 = run()
    assert torch.equal(dG, dG2) and torch.equal(dpre_h, dpre_h2), "two launches differ"
    assert (dsp is None or torch.equal(dsp, dsp2)) and (dc0 is None or torch.equal(dc0, dc02))
    # each kernel alone leaves the other's columns of dG as it found them, and writes the same values it writes in the pair
    ga, _, _, _ = run(b=False)
    gb, _, dspb, _ = run(a=False)
    assert (ga[:, :3 * Hc] == SENTINEL).all() and (gb[:, 3 * Hc:] == SENTINEL).all()
    assert torch.equal(ga[:, 3 * Hc:], dG[:, 3 * Hc:]) and torch.equal(gb[:, :3 * Hc], dG[:, :3 * Hc])
    if dsp is not None:                                       # the h half of d_state_prev is not lstm_bwd_b's
        assert (dsp[:, :D] == SENTINEL).all()
    got_dc0 = dsp[:, D:] if dsp is not None else dc0
    assert torch.isfinite(dG).all() and torch.isfinite(dpre_h).all()
    # padded rows: zeros despite the garbage in every input row
    assert not dG[~valid].any() and not dpre_h[~valid].any()
    if got_dc0 is not None:
        assert not got_dc0[~valid].any()
    # accuracy
    ext_h = d_state_out.view(M, Dp)[:, :D] if ext else None
    ext_c = d_state_out.view(M, Dp)[:, D:] if ext else None
    ref_o, ref_h = R.lstm_bwd_a_ref(dy, ext_h, o, tc, valid)
    ref_g, ref_dc0 = R.lstm_bwd_b_ref(dc1_h, ext_c, frm, c0, valid)
    groups = slide_groups(num_ims, N)
    ea = {"dpre_o": elem_err(dG[:, 3 * Hc:], ref_o, groups), "dpre_h": elem_err(dpre_h, ref_h, groups)}
    eb = {"dgates": elem_err(dG[:, :3 * Hc], ref_g, groups)}
    if got_dc0 is not None:
        eb["dc0"] = elem_err(got_dc0, ref_dc0, groups)
    print(f"[lstm] N={N} D={D} Hc={Hc}: " + " ".join(f"{k}={v:.2e}" for k, v in {**ea, **eb}.items()))
    assert max(ea.values()) < BAR["lstm_a"], ea
    assert max(eb.values()) < BAR["lstm_b"], eb
    # sensitivity: the longest slide cut by one patch, and r / m read from each other's planes
    b = longest(num_ims)
    sl = [slice(b * N, (b + 1) * N)]
    v1 = R.valid_rows(torch.tensor(cut_one(num_ims)), N).to(dev)
    wo, wh = R.lstm_bwd_a_ref(dy, ext_h, o, tc, v1)
    wg, _ = R.lstm_bwd_b_ref(dc1_h, ext_c, frm, c0, v1)
    sg, _ = R.lstm_bwd_b_ref(dc1_h, ext_c, frm, c0, valid, swap_rm=True)
    den = lambda ref: float(ref[sl[0]].abs().max())                   # noqa: E731
    miss = {"a: len - 1": float((dG[sl[0], 3 * Hc:].double() - wo[sl[0]]).abs().max()) / den(ref_o),
            "b: len - 1": float((dG[sl[0], :3 * Hc].double() - wg[sl[0]]).abs().max()) / den(ref_g),
            "b: r <-> m": elem_err(dG[:, :3 * Hc], sg, groups)}
    print("[lstm]   against wrong references: " + " ".join(f"{k}={v:.2e}" for k, v in miss.items()))
    assert miss["a: len - 1"] >= 10 * BAR["lstm_a"] and miss["b: len - 1"] >= 10 * BAR["lstm_b"] and miss["b: r <-> m"] >= 10 * BAR["lstm_b"], miss


# ---------------------------------------------------------------------------------------------------------------------------------
# importance MLP + scaling + proj_in, LSTM form (dtok) and lstm = false form (dZ rows)
# ---------------------------------------------------------------------------------------------------------------------------------
def _imp_inputs(g, dev, num_ims, N, Hi, width):
    M = len(num_ims) * N
    nims = torch.tensor(num_ims, device=dev, dtype=torch.int64)
    valid = R.valid_rows(nims, N)
    hid = torch.relu(rnd(g, M, Hi))                              # about half exact zeros (the relu mask)
    alpha = torch.where(valid, saturate(g, torch.sigmoid(2 * rnd(g, M)), 0.0, 1.0), 0.0)   # padded rows: alpha == 0 by the mask
    alpha[longest(num_ims) * N + max(num_ims) - 1] = 0.3           # the row the sensitivity check cuts: not saturated
    w2 = rnd(g, Hi)
    return M, nims, valid, hid, alpha, w2


# (Hi, d, ldu extra columns beyond round-up-to-32, imp_mul, N); (128, 128) with ldu 256 runs the fast kernel
IMP_CASES = [(128, 128, 0, 1, 160), (128, 128, 0, 0, 7), (128, 128, 0, 1, 2049),
             (36, 64, 0, 1, 160), (64, 64, 32, 0, 7), (96, 192, 0, 1, 7), (128, 192, 32, 1, 160), (64, 384, 0, 1, 2049),
             (128, 96, 32, 1, 7), (128, 160, 0, 0, 160), (128, 320, 32, 1, 160), (128, 1536, 0, 1, 160), (200, 192, 32, 1, 160),
             (36, 64, 32, 0, 1), (96, 192, 32, 1, 1)]


@pytest.mark.parametrize("Hi,d,extra,imp_mul,N", IMP_CASES, ids=[f"Hi{h}-d{d}-ldu+{e}-mul{m}-N{n}" for h, d, e, m, n in IMP_CASES])
def test_importance_bwd_vs_fp64(dev, Hi, d, extra, imp_mul, N):
    L = _lib()
    st = L.stream()
    g = gen(dev, Hi * 7 + d + extra + imp_mul + N)
    num_ims = [N - 1, 0, N, 1]
    M, nims, valid, hid, alpha, w2 = _imp_inputs(g, dev, num_ims, N, Hi, d)
    B = len(num_ims)
    fast = (Hi, d, extra) == (128, 128, 0)
    U = (Hi + d + 31) // 32 * 32 + extra
    dtok = rnd(g, B, N + 1, d)
    tv = torch.cat((torch.zeros(B, 1, dtype=torch.bool, device=dev), valid.view(B, N)), 1)       # row 0: the special token
    dtok = torch.where(tv[..., None], dtok, GARBAGE * (1 + torch.rand_like(dtok))).contiguous()
    pproj = rnd(g, M, d)

    def run():
        du = torch.full((M, U), SENTINEL, device=dev)
        da = torch.full((M,), SENTINEL, device=dev)
        dah = torch.full((M, Hi), SENTINEL, device=dev)
        if fast:
            L.call("paths_importance_bwd", P(dtok), P(pproj), P(hid), P(alpha), P(w2), P(nims), N, M, imp_mul, P(du), P(da), P(dah), st)
        else:
            L.call("paths_importance_bwd_any", P(dtok), P(pproj), P(hid), P(alpha), P(w2), P(nims), N, M, imp_mul, Hi, d, U, P(du), P(da),
                   P(dah), st)
        sync()
        return du, da, dah

    du, da, dah = run()
    du2, da2, dah2 = run()
    assert torch.equal(du, du2) and torch.equal(da, da2) and torch.equal(dah, dah2), "two launches differ"
    assert torch.isfinite(du).all() and torch.isfinite(da).all() and torch.isfinite(dah).all()
    assert not du[:, Hi + d:].any(), "pad columns of dU not zeroed"
    assert not du[~valid].any() and not da[~valid].any() and not dah[~valid].any(), "padded rows not zero"
    rh, rp, rda, rdah, cond = R.importance_bwd_ref(dtok, pproj, hid, alpha, w2, valid, N, imp_mul)
    groups = slide_groups(num_ims, N)
    # dhid, da and dah inherit the conditioning of dalpha = g . P: measured against sum|g_c P_c| alpha (1 - alpha) times their factor
    e = {"dP": elem_err(du[:, Hi:Hi + d], rp, groups),
         "da": sum_err(da, rda, cond),
         "dhid": sum_err(du[:, :Hi], rh, cond[:, None] * w2.double().abs()[None, :] * (hid > 0)),
         "dah": sum_err(dah, rdah, cond[:, None] * hid.double())}
    print(f"[imp] {'fast' if fast else 'any'} Hi={Hi} d={d} ldu={U} mul={imp_mul} N={N}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    assert e["dP"] < BAR["imp_elem"], e
    assert max(e["da"], e["dhid"], e["dah"]) < BAR["imp_dot"], e
    b = longest(num_ims)
    v1 = R.valid_rows(torch.tensor(cut_one(num_ims)), N).to(dev)
    _, wp, _, _, _ = R.importance_bwd_ref(dtok, pproj, hid, alpha, w2, v1, N, imp_mul)
    sl = slice(b * N, (b + 1) * N)
    miss = float((du[sl, Hi:Hi + d].double() - wp[sl]).abs().max()) / float(rp[sl].abs().max())
    print(f"[imp]   against len - 1: {miss:.2e}")
    assert miss >= 10 * BAR["imp_elem"]


# (Hi, D, N); Hi 128 runs the fast kernel
IMP_ROWS_CASES = [(128, 1024, 160), (128, 1536, 7), (128, 1028, 2049), (36, 1024, 160), (64, 132, 7), (96, 1024, 7), (200, 132, 160),
                  (36, 132, 2049), (200, 1024, 1), (64, 1024, 160)]


@pytest.mark.parametrize("Hi,D,N", IMP_ROWS_CASES, ids=[f"Hi{h}-D{d}-N{n}" for h, d, n in IMP_ROWS_CASES])
def test_importance_rows_bwd_vs_fp64(dev, Hi, D, N):
    """lstm = false form: dZ and X of the padded rows hold garbage (the kernel reads every row's dot product, then masks it)."""
    L = _lib()
    st = L.stream()
    g = gen(dev, Hi + D * 3 + N)
    num_ims = [N - 1, 0, N, 1]
    M, nims, valid, hid, alpha, w2 = _imp_inputs(g, dev, num_ims, N, Hi, D)
    dz = garbage_rows(rnd(g, M, D), valid)
    x = garbage_rows(rnd(g, M, D), valid)
    fast = Hi == 128

    def run():
        dh, da, dah = (torch.full(s, SENTINEL, device=dev) for s in ((M, Hi), (M,), (M, Hi)))
        if fast:
            L.call("paths_importance_rows_bwd", P(dz), P(x), D, P(hid), P(alpha), P(w2), P(nims), N, M, P(dh), P(da), P(dah), st)
        else:
            L.call("paths_importance_rows_bwd_any", P(dz), P(x), D, P(hid), P(alpha), P(w2), P(nims), N, M, Hi, P(dh), P(da), P(dah), st)
        sync()
        return dh, da, dah

    dh, da, dah = run()
    dh2, da2, dah2 = run()
    assert torch.equal(dh, dh2) and torch.equal(da, da2) and torch.equal(dah, dah2), "two launches differ"
    assert torch.isfinite(dh).all() and not dh[~valid].any() and not da[~valid].any() and not dah[~valid].any()
    rh, rda, rdah, cond = R.importance_rows_bwd_ref(dz, x, hid, alpha, w2, valid)
    e = {"da": sum_err(da, rda, cond), "dh": sum_err(dh, rh, cond[:, None] * w2.double().abs()[None, :] * (hid > 0)),
         "dah": sum_err(dah, rdah, cond[:, None] * hid.double())}
    print(f"[imp-rows] {'fast' if fast else 'any'} Hi={Hi} D={D} N={N}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    assert max(e.values()) < BAR["imp_rows_dot"], e
    b = longest(num_ims)
    v1 = R.valid_rows(torch.tensor(cut_one(num_ims)), N).to(dev)
    _, wda, _, _ = R.importance_rows_bwd_ref(dz, x, hid, alpha, w2, v1)
    sl = slice(b * N, (b + 1) * N)
    miss = sum_err(da[sl], wda[sl], cond[sl])
    print(f"[imp-rows]   against len - 1: {miss:.2e}")
    assert miss >= 10 * BAR["imp_rows_dot"]


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm: forward statistics, backward, backward + slab sums
# ---------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "constant", "small", "ill")


def ln_rows(g, dev, rows, d, add):
    """x [rows, d] with row r in family r % 4: standard normal, constant after the add (variance 0), scale 1e-3 (eps matters),
    |mean| / std = 3e4.  add [d] (zeros when the kernel gets none) must be dyadic with few bits."""
    x = torch.randn(rows, d, device=dev, generator=g)
    fam = torch.arange(rows, device=dev) % 4
    x = torch.where((fam == 1)[:, None], torch.round(x[:, :1] * 8) / 8 + 0.25 - add, x)     # dyadic: x + add and its mean are exact
    x = torch.where((fam == 2)[:, None], x * 1e-3, x)
    x = torch.where((fam == 3)[:, None], 3e4 + x, x)
    return x.contiguous(), fam


# d, rows, add / y given, rows_per_block
LN_CASES = [(128, 1, True, 4), (128, 5, False, 7), (128, 4097, True, 64), (128, 65, False, 256),
            (36, 3, True, 7), (64, 64, False, 64), (96, 4, True, 4), (160, 63, True, 7), (192, 4097, False, 256), (256, 65, True, 64),
            (320, 5, False, 4), (384, 1, False, 256), (1540, 63, True, 64), (1536, 64, False, 7), (2044, 4097, True, 256),
            (2048, 3, True, 4), (2048, 65, False, 64), (36, 4097, False, 64)]


@pytest.mark.parametrize("d,rows,affine,rpb", LN_CASES, ids=[f"d{d}-rows{r}-{'add' if a else 'noadd'}-rpb{p}" for d, r, a, p in LN_CASES])
def test_layernorm_vs_fp64(dev, d, rows, affine, rpb):
    L = _lib()
    st = L.stream()
    fast = d == 128
    sfx = "" if fast else "_any"
    g = gen(dev, d * 13 + rows + rpb)
    add = torch.round(rnd(g, d) * 8) / 8 if affine else None
    x, fam = ln_rows(g, dev, rows, d, add if affine else torch.zeros(d, device=dev))
    gamma = rnd(g, d)
    gamma[::5] = 0
    beta = rnd(g, d)
    groups = {f: torch.nonzero(fam == i)[:, 0] for i, f in enumerate(FAMILIES)}

    # forward statistics
    def fwd():
        y = torch.full((rows, d), SENTINEL, device=dev) if affine else None
        xh = torch.full((rows, d), SENTINEL, device=dev)
        rs = torch.full((rows,), SENTINEL, device=dev)
        L.call("paths_layernorm_fwd_stats" + sfx, P(x), P(add), P(gamma), P(beta), P(y), P(xh), P(rs), rows, d, 1e-5, st)
        sync()
        return y, xh, rs

    y, xh, rs = fwd()
    y2, xh2, rs2 = fwd()
    assert torch.equal(xh, xh2) and torch.equal(rs, rs2) and (y is None or torch.equal(y, y2)), "two launches differ"
    ry, rxh, rrs = R.ln_fwd_ref(x, add, gamma, beta)
    ef = {}
    for f in ("normal", "constant", "small"):
        gi = groups[f]
        if gi.numel():
            ef[f"xhat_{f}"] = float((xh[gi].double() - rxh[gi]).abs().max())          # xhat is O(1): absolute error
            ef[f"rstd_{f}"] = float(((rs[gi].double() - rrs[gi]) / rrs[gi]).abs().max())
            if affine:
                ef[f"y_{f}"] = elem_err(y, ry, [gi])
    print(f"[ln-fwd] d={d} rows={rows}: " + " ".join(f"{k}={v:.2e}" for k, v in ef.items()))
    assert max(ef.values()) < BAR["ln_fwd"], ef
    gi = groups["normal"]
    _, _, wrs = R.ln_fwd_ref(x[gi], add, None, None, ddof=1)
    miss = float(((rs[gi].double() - wrs) / wrs).abs().max())
    print(f"[ln-fwd]   against variance over d - 1: {miss:.2e}")
    assert miss >= 10 * BAR["ln_fwd"]
    if groups["ill"].numel():
        gi = groups["ill"]
        xin = x[gi] + (add if affine else 0)
        t_out, _, t_rs = torch.native_layer_norm(xin, [d], None, None, 1e-5)
        k_err = float((xh[gi].double() - rxh[gi]).abs().max())
        t_err = float((t_out.double() - rxh[gi]).abs().max())
        k_rs = float(((rs[gi].double() - rrs[gi]) / rrs[gi]).abs().max())
        t_rs_err = float(((t_rs[:, 0].double() - rrs[gi]) / rrs[gi]).abs().max())
        print(f"[ln-fwd]   ill-conditioned rows: xhat kernel {k_err:.2e} torch {t_err:.2e}; rstd kernel {k_rs:.2e} torch {t_rs_err:.2e}")
        assert k_err <= ILL_RATIO * t_err and k_rs <= max(ILL_RATIO * t_rs_err, BAR["ln_fwd"])

    # backward from the float64 statistics rounded to fp32 (each kernel on its own)
    xh32, rs32 = rxh.float().contiguous(), rrs.float().contiguous()
    dy = rnd(g, rows, d)

    def bwd():
        dx = torch.full((rows, d), SENTINEL, device=dev)
        dyx = torch.full((rows, d), SENTINEL, device=dev)
        L.call("paths_layernorm_bwd" + sfx, P(dy), P(xh32), P(rs32), P(gamma), P(dx), P(dyx), rows, d, st)
        nblk = (rows + rpb - 1) // rpb
        dx_s = torch.full((rows, d), SENTINEL, device=dev)
        slabs = torch.full((nblk, 3 * d), SENTINEL, device=dev)
        L.call("paths_layernorm_bwd_sums" + sfx, P(dy), P(xh32), P(rs32), P(gamma), P(dx_s), P(slabs), rows, d, rpb, st)
        gb = torch.full((3 * d,), SENTINEL, device=dev)
        L.call("paths_reduce_slabs_f32", P(slabs), nblk, 3 * d, P(gb), 0, st)
        sync()
        return dx, dyx, dx_s, slabs, gb

    out1, out2 = bwd(), bwd()
    assert all(torch.equal(a, b) for a, b in zip(out1, out2)), "two launches differ"
    dx, dyx, dx_s, slabs, gb = out1
    assert torch.equal(dyx, dy * xh32), "dy * xhat is one fp32 product"
    ref = R.ln_bwd_ref(dy, xh32, rs32, gamma)
    fam_groups = [gi for gi in groups.values() if gi.numel()]
    eb = {"dx": elem_err(dx, ref["dx"], fam_groups), "dx_sums": elem_err(dx_s, ref["dx"], fam_groups)}
    es = {n: sum_err(gb[i * d:(i + 1) * d], ref[n], ref[n + "_abs"]) for i, n in enumerate(("dgamma", "dbeta", "dxsum"))}
    # every slab: the sums over its own rows
    nblk = slabs.shape[0]
    blk = torch.arange(rows, device=dev) // rpb
    seg = lambda t: torch.zeros((nblk, d), dtype=F64, device=dev).index_add_(0, blk, t)      # noqa: E731
    dx64 = ref["dx"]
    terms = [seg(ref["dyxhat"].abs()), seg(dy.double().abs()), seg(ref["dx_abs"])]
    for i, (n, t) in enumerate(zip(("dyxhat", "dy", "dx"), (ref["dyxhat"], dy.double(), dx64))):
        es["slab_" + n] = sum_err(slabs[:, i * d:(i + 1) * d], seg(t), terms[i])
    print(f"[ln-bwd] d={d} rows={rows} rpb={rpb}: " + " ".join(f"{k}={v:.2e}" for k, v in {**eb, **es}.items()))
    assert max(eb.values()) < BAR["ln_bwd"], eb
    assert max(es.values()) < BAR["ln_sum"], es
    # sensitivity: means over d - 1; the sums without their last slab
    w = R.ln_bwd_ref(dy, xh32, rs32, gamma, ddof=1)
    miss_dx = elem_err(dx, w["dx"], fam_groups)
    last = slice((nblk - 1) * rpb, rows)
    miss_sum = max(sum_err(gb[i * d:(i + 1) * d], ref[n] - t[last].sum(0), ref[n + "_abs"])
                   for i, (n, t) in enumerate((("dgamma", ref["dyxhat"]), ("dbeta", dy.double()), ("dxsum", dx64))))
    print(f"[ln-bwd]   against means over d - 1: {miss_dx:.2e}; without the last slab: {miss_sum:.2e}")
    assert miss_dx >= 10 * BAR["ln_bwd"] and miss_sum >= 10 * BAR["ln_sum"]


@pytest.mark.parametrize("d,rows", [(128, 4097), (36, 65), (1540, 63), (2048, 64), (192, 5)])
def test_layernorm_stats_then_backward_vs_autograd(dev, d, rows):
    """The chained pass of the backward (paths_amd/backward.py: _ln_fwd then _ln_bwd_sums) from x, against float64 autograd of
    F.layer_norm(x + add) with eps 1e-5: dx, dgamma, dbeta."""
    L = _lib()
    st = L.stream()
    sfx = "" if d == 128 else "_any"
    g = gen(dev, d + rows)
    x = torch.randn(rows, d, device=dev, generator=g) * 2 + 0.5
    add, gamma, beta, dy = rnd(g, d), rnd(g, d), rnd(g, d), rnd(g, rows, d)
    gamma[::5] = 0
    y, xh, rs = (torch.empty(s, device=dev) for s in ((rows, d), (rows, d), (rows,)))
    L.call("paths_layernorm_fwd_stats" + sfx, P(x), P(add), P(gamma), P(beta), P(y), P(xh), P(rs), rows, d, 1e-5, st)
    rpb = 64
    nblk = (rows + rpb - 1) // rpb
    dx, slabs, gb = torch.empty(rows, d, device=dev), torch.empty(nblk, 3 * d, device=dev), torch.empty(3 * d, device=dev)
    L.call("paths_layernorm_bwd_sums" + sfx, P(dy), P(xh), P(rs), P(gamma), P(dx), P(slabs), rows, d, rpb, st)
    L.call("paths_reduce_slabs_f32", P(slabs), nblk, 3 * d, P(gb), 0, st)
    sync()
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64 = F.layer_norm(x64 + add.double(), (d,), g64, b64, 1e-5)
    (y64 * dy.double()).sum().backward()
    e = {"y": elem_err(y, y64.detach(), [slice(0, rows)]), "dx": elem_err(dx, x64.grad, [slice(0, rows)]),
         "dgamma": sum_err(gb[:d], g64.grad, (dy.double() * R.ln_fwd_ref(x, add, None, None)[1]).abs().sum(0)),
         "dbeta": sum_err(gb[d:2 * d], b64.grad, dy.double().abs().sum(0))}
    print(f"[ln-chain] d={d} rows={rows}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    assert max(e.values()) < BAR["ln_chain"], e


# ---------------------------------------------------------------------------------------------------------------------------------
# column sums and their slabs
# ---------------------------------------------------------------------------------------------------------------------------------
# N, M, splits, lda, base offset (floats), accumulate
COLSUM_CASES = [(1, 1, 1, 1, 0, 0), (3, 7, 16, 5, 0, 1), (36, 1000, 15, 40, 0, 0), (128, 1000, 256, 128, 0, 1), (128, 7, 8, 128, 1, 0),
                (129, 16385, 256, 129, 0, 0), (1280, 1000, 15, 1280, 0, 0), (1280, 16385, 256, 1284, 0, 1), (1792, 7, 1, 1792, 0, 0),
                (1792, 1000, 3, 1800, 1, 1), (4608, 16385, 64, 4608, 0, 0), (4608, 1, 256, 4608, 0, 1), (36, 16385, 200, 37, 0, 0),
                (3, 1000, 1, 3, 0, 0), (1, 16385, 256, 1, 0, 1), (128, 1, 2, 132, 0, 0)]


@pytest.mark.parametrize("N,M,splits,lda,off,acc", COLSUM_CASES, ids=[f"N{n}-M{m}-s{s}-lda{l}-off{o}-acc{a}" for n, m, s, l, o, a in COLSUM_CASES])
def test_colsum_vs_fp64(dev, N, M, splits, lda, off, acc):
    """paths_colsum_f32: the 16-byte partial kernel (<32> up to 128 columns, <64> above) when N, lda and the base allow it, the scalar
    one otherwise (odd N or lda, a base one float off); splits above M leave empty slabs; every slab and the reduced output checked."""
    L = _lib()
    st = L.stream()
    g = gen(dev, N + M + splits + off)
    buf = rnd(g, off + M * lda, lo=-0.5, hi=1.0)                    # partly cancelling columns
    a = buf[off:].view(M, lda)[:, :N]
    init = rnd(g, N)

    def run():
        out = init.clone() if acc else torch.full((N,), SENTINEL, device=dev)
        ws = torch.full((splits * N,), SENTINEL, device=dev)
        L.call("paths_colsum_f32", P(buf) + 4 * off, lda, M, N, P(out), splits, acc, P(ws), st)
        sync()
        return out, ws.view(splits, N)

    out, ws = run()
    out2, ws2 = run()
    assert torch.equal(out, out2) and torch.equal(ws, ws2), "two launches differ"
    a64 = a.double()
    rps = (M + splits - 1) // splits
    seg = torch.arange(M, device=dev) // rps
    ref_ws = torch.zeros((splits, N), dtype=F64, device=dev).index_add_(0, seg, a64)
    abs_ws = torch.zeros((splits, N), dtype=F64, device=dev).index_add_(0, seg, a64.abs())
    ref = a64.sum(0) + (init.double() if acc else 0)
    terms = a64.abs().sum(0) + (init.double().abs() if acc else 0)
    e = {"out": sum_err(out, ref, terms), "slabs": sum_err(ws, ref_ws, abs_ws)}
    print(f"[colsum] N={N} M={M} splits={splits} lda={lda} off={off} acc={acc}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    assert max(e.values()) < BAR["colsum"], e
    assert not ws[(M + rps - 1) // rps:].any(), "empty slabs not zero"
    last = (M - 1) // rps                                          # the last slab that holds rows
    miss = sum_err(out, ref - ref_ws[last], terms)
    print(f"[colsum]   without the last slab: {miss:.2e}")
    assert miss >= 10 * BAR["colsum"]


def test_deferred_reductions_are_bitwise_the_immediate_calls(dev):
    """paths_defer_reductions(1): 35 registered reductions (colsums and LayerNorm slab sums) flush in two launches; an accumulate chain
    of three colsums into one output flushes early (overlap rule).  Before the final flush the pending outputs hold their sentinel;
    after it n_entries is right and every output is bit-equal to the same calls made immediately.  Every workspace stays alive until
    the flush (as backward._keep_slabs keeps them)."""
    import ctypes
    L = _lib()
    lib = L.load()
    st = L.stream()
    g = gen(dev, 99)
    shapes = [(1000 + 37 * i, (36, 128, 129, 1280, 3, 1)[i % 6]) for i in range(24)]
    mats = [rnd(g, M, N) for M, N in shapes]
    slab_in = [(rnd(g, 1 + 5 * i, 3 * (36 + 4 * i))) for i in range(10)]
    chain_in = [rnd(g, 777, 192) for _ in range(3)]
    chain_init = rnd(g, 192)

    def calls(keep):
        outs = []
        chain = chain_init.clone()
        for j, x in enumerate(chain_in):                       # accumulate chain into one output
            ws = torch.empty(16 * 192, device=dev)
            keep.append(ws)
            L.call("paths_colsum_f32", P(x), 192, 777, 192, P(chain), 16, 1, P(ws), st)
        chain_pending = chain.clone() if keep is not None else None
        for x in mats:
            M, N = x.shape
            out = torch.full((N,), SENTINEL, device=dev)
            splits = max(1, min(256, M // 64))
            ws = torch.empty(splits * N, device=dev)
            keep.append(ws)
            L.call("paths_colsum_f32", P(x), N, M, N, P(out), splits, 0, P(ws), st)
            outs.append(out)
        for s in slab_in:
            out = torch.full((s.shape[1],), SENTINEL, device=dev)
            L.call("paths_reduce_slabs_f32", P(s), s.shape[0], s.shape[1], P(out), 0, st)
            outs.append(out)
        return chain, chain_pending, outs

    sync()
    imm_chain, _, imm = calls([])
    sync()
    keep = []
    prev = lib.paths_defer_reductions(1)
    n = ctypes.c_int(-1)
    try:
        chain, chain_before, outs = calls(keep)
        sync()
        pending_before = [bool((o == SENTINEL).all()) for o in outs]
        L.call("paths_flush_reductions", ctypes.byref(n), st)
        sync()
    finally:
        if n.value < 0:                                         # (an assertion above: do not leave entries pointing into freed slabs)
            lib.paths_flush_reductions(None, ctypes.c_void_p(st))
            sync()
        lib.paths_defer_reductions(prev)
        keep.clear()
    assert all(pending_before), "a deferred output was written before the flush"
    assert n.value == len(outs) + 1 > 32, n.value               # the last chain colsum is pending too
    assert not torch.equal(chain_before, chain), "the chain's last colsum ran before the flush"
    assert torch.equal(chain, imm_chain)
    for a, b in zip(outs, imm):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# gradients between levels
# ---------------------------------------------------------------------------------------------------------------------------------
def _between_case(dev, ldk, seed):
    """B = 3 slides with keep_count 0, ldk - 1 and ldk; -1 holes in each of the four child blocks; distinct kept rows and children"""
    g = torch.Generator().manual_seed(seed)
    counts = [0, ldk - 1, ldk] if ldk > 1 else [0, 1, 1]
    B = len(counts)
    n_cur, n_next = ldk + 5, 4 * ldk + 3
    keep_idx = torch.full((B, ldk), -7, dtype=torch.int32)
    child_pos = torch.full((B, 4 * ldk), -9, dtype=torch.int32)
    for b, c in enumerate(counts):
        keep_idx[b, :c] = torch.randperm(n_cur, generator=g)[:c].to(torch.int32)
        pos = torch.randperm(n_next, generator=g)[:4 * c].to(torch.int32)
        for blk in range(4):
            if c > 1 or (c == 1 and blk % 2 == b % 2):
                pos[blk * c + (7 * blk + b) % c] = -1
        child_pos[b, :4 * c] = pos
    return keep_idx.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), child_pos.to(dev), n_cur, n_next


@pytest.mark.parametrize("ldk", [1, 16, 512])
def test_gradients_between_levels_are_bitwise_fp32_block_sums(dev, ldk):
    L = _lib()
    st = L.stream()
    D, Hc = 1024, 256
    Dp, G = D + Hc, 3 * Hc + D
    keep_idx, kc, cp, n_cur, n_next = _between_case(dev, ldk, ldk)
    B = kc.shape[0]
    g = gen(dev, ldk + 1)
    # paths_gather_rows_bwd (GatherFn, the per-child form): d_cur [B, n_cur, Dp]
    d_next = rnd(g, B, n_next, Dp)
    for _ in range(2):
        d_cur = torch.full((B, n_cur, Dp), SENTINEL, device=dev)
        L.call("paths_gather_rows_bwd", P(keep_idx), ldk, P(kc), P(cp), P(d_next), n_next, Dp, P(d_cur), n_cur, B, st)
        sync()
        assert torch.equal(d_cur, R.sibling_sum_ref(d_next, cp, kc, ldk, Dp, torch.full_like(d_cur, SENTINEL), keep_idx))
    # paths_sibling_sum with keep_idx (GatherParentFn: d_c0 into the Hc half of d_cur, row stride Dp)
    d_c0 = rnd(g, B, n_next, Hc)
    d_cur = torch.full((B, n_cur, Dp), SENTINEL, device=dev)
    L.call("paths_sibling_sum", P(keep_idx), ldk, P(kc), P(cp), P(d_c0), n_next, Hc, Hc, P(d_cur) + 4 * D, n_cur, Dp, B, st)
    sync()
    want = torch.full((B, n_cur, Dp), SENTINEL, device=dev)
    want[:, :, D:] = R.sibling_sum_ref(d_c0, cp, kc, ldk, Hc, torch.full((B, n_cur, Hc), SENTINEL, device=dev), keep_idx)
    assert torch.equal(d_cur, want)
    # paths_sibling_sum without keep_idx (selection_backward: dG rows of the children -> the compact kept-parent table dhp)
    N = n_next
    dG = rnd(g, B, N, G)
    dhp = torch.full((B, ldk, G), SENTINEL, device=dev)
    L.call("paths_sibling_sum", None, ldk, P(kc), P(cp), P(dG), N, G, G, P(dhp), ldk, G, B, st)
    sync()
    assert torch.equal(dhp, R.sibling_sum_ref(dG, cp, kc, ldk, G, torch.full_like(dhp, SENTINEL)))
    # paths_scatter_kept_rows (d_hk back into the h half of d_cur)
    d_hk = rnd(g, B, ldk, D)
    d_cur2 = d_cur.clone()
    L.call("paths_scatter_kept_rows", P(d_hk), ldk, D, P(keep_idx), P(kc), P(d_cur2), n_cur, Dp, D, B, st)
    sync()
    assert torch.equal(d_cur2, R.scatter_kept_rows_ref(d_hk, keep_idx, kc, d_cur, D))
    # paths_gather_kept_rows (forward of the once-per-parent form): zero-filled beyond keep_count
    state = rnd(g, B, n_cur, Dp)
    hk = torch.full((B * ldk, D), SENTINEL, device=dev)
    L.call("paths_gather_kept_rows", P(state), n_cur, Dp, P(keep_idx), ldk, P(kc), D, B, P(hk), st)
    sync()
    assert torch.equal(hk.view(B, ldk, D), R.gather_kept_rows_ref(state, keep_idx, kc, ldk, D))
    # the bar is exact: a sum in another order (block 3 first) differs somewhere
    if ldk > 1:
        alt = R.sibling_sum_ref(dG, cp.clone(), kc, ldk, G, torch.full_like(dhp, SENTINEL))
        c = int(kc[2])
        pos = cp[2, :4 * c].view(4, c).long()
        s = torch.zeros(c, G, device=dev)
        for blk in (3, 2, 1, 0):
            s = s + torch.where((pos[blk] >= 0)[:, None], dG[2, pos[blk].clamp(min=0)], torch.zeros(1, device=dev))
        alt[2, :c] = s
        assert not torch.equal(dhp, alt), "block order is not observable at this size"


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage: every entry point a backward pass launches has a direct test
# ---------------------------------------------------------------------------------------------------------------------------------
HERE = "tests/test_gpu_row_backward.py"
ATTN = "tests/test_gpu_attention_backward.py"
BWD = "tests/test_gpu_backward.py"
PARITY = "tests/test_gpu_parity.py"
DIRECT_TESTS = {
    "paths_lstm_bwd_a": HERE + "::test_lstm_bwd_vs_fp64",
    "paths_lstm_bwd_b": HERE + "::test_lstm_bwd_vs_fp64",
    "paths_importance_bwd": HERE + "::test_importance_bwd_vs_fp64",
    "paths_importance_bwd_any": HERE + "::test_importance_bwd_vs_fp64",
    "paths_importance_rows_bwd": HERE + "::test_importance_rows_bwd_vs_fp64",
    "paths_importance_rows_bwd_any": HERE + "::test_importance_rows_bwd_vs_fp64",
    "paths_layernorm_fwd_stats": HERE + "::test_layernorm_vs_fp64",
    "paths_layernorm_fwd_stats_any": HERE + "::test_layernorm_vs_fp64",
    "paths_layernorm_bwd": HERE + "::test_layernorm_vs_fp64",
    "paths_layernorm_bwd_any": HERE + "::test_layernorm_vs_fp64",
    "paths_layernorm_bwd_sums": HERE + "::test_layernorm_vs_fp64",
    "paths_layernorm_bwd_sums_any": HERE + "::test_layernorm_vs_fp64",
    "paths_reduce_slabs_f32": HERE + "::test_layernorm_vs_fp64",
    "paths_colsum_f32": HERE + "::test_colsum_vs_fp64",
    "paths_flush_reductions": HERE + "::test_deferred_reductions_are_bitwise_the_immediate_calls",
    "paths_gather_rows_bwd": HERE + "::test_gradients_between_levels_are_bitwise_fp32_block_sums",
    "paths_sibling_sum": HERE + "::test_gradients_between_levels_are_bitwise_fp32_block_sums",
    "paths_scatter_kept_rows": HERE + "::test_gradients_between_levels_are_bitwise_fp32_block_sums",
    "paths_attention_bwd_x6_planes": ATTN + "::test_attention_backward_vs_fp64",
    "paths_attention_bwd_x6_dropout": ATTN + "::test_attention_backward_vs_fp64",
    "paths_attention_bwd_f32": ATTN + "::test_attention_backward_vs_fp64",
    "paths_attention_bwd_f32_dropout": ATTN + "::test_attention_backward_vs_fp64",
    "paths_attention_bwd_any": ATTN + "::test_attention_backward_vs_fp64",
    "paths_attention_wide_bwd": ATTN + "::test_attention_backward_vs_fp64",
    "paths_attention_token0_bwd": ATTN + "::test_attention_backward_vs_fp64",
    "paths_attention_x6_dropout": ATTN + "::test_training_forward_then_backward_vs_fp64",
    "paths_attention_any_train": ATTN + "::test_training_forward_then_backward_vs_fp64",
    "paths_attention_wide_fwd": ATTN + "::test_training_forward_then_backward_vs_fp64",
    "paths_attention_token0_fwd": ATTN + "::test_training_forward_then_backward_vs_fp64",
    "paths_attention_x6": PARITY + "::test_single_level_vs_reference_golden",
    "paths_attention_f32": PARITY + "::test_single_level_variants",
    "paths_gemm_tn_f32": BWD + "::test_gemm_tn_and_nt_ragged_widths",
    "paths_gemm_tn_x6": BWD + "::test_gemm_tn_x6_matches_fp64",
    "paths_gemm_nt_x6": BWD + "::test_gemm_nt_train_planes_matches_fp64",
    "paths_gemm_nt_f32": BWD + "::test_gemm_tn_and_nt_ragged_widths",
    "paths_x6_pack_weights_t": BWD + "::test_gemm_nt_train_planes_matches_fp64",
    "paths_transpose_f32": BWD + "::test_gemm_tn_colsum_transpose",
    "paths_dropout_rows": BWD + "::test_dropout_forward_backward_vs_fp64_with_exported_masks",
}

COVERAGE_CONFIGS = {"shipped_k16": {}, "td192": {"model_config": {"trans_dim": 192}}, "nolstm": {"model_config": {"lstm": False}},
                    "td64_h1_hi36_nolstm": {"model_config": {"trans_dim": 64, "trans_heads": 1, "importance_mlp_hidden_dim": 36, "lstm": False}}}


def test_direct_test_map_names_real_tests():
    import importlib
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, tid in DIRECT_TESTS.items():
        path, test = tid.split("::")
        assert os.path.isfile(os.path.join(root, path)), tid
        mod = importlib.import_module(path[:-3].replace("/", "."))
        assert callable(getattr(mod, test, None)), tid


@pytest.mark.parametrize("cfg", list(COVERAGE_CONFIGS), ids=list(COVERAGE_CONFIGS))
def test_every_backward_entry_point_has_a_direct_test(dev, cfg):
    """loss.backward() of a small training step (once-per-parent form at K = 16, trans_dim 192, lstm false, td64 / hidden 36 without
    the LSTM) launches only entry points listed in DIRECT_TESTS: a new backward kernel needs a direct test before it ships."""
    from paths_amd import utils as putils
    from tests.test_gpu_backward import _train_setup
    c, model, _, _, batch = _train_setup(dev, top_k=16, base=(6, 7), n_slides=3, cfg_over=COVERAGE_CONFIGS[cfg])
    model.train()
    out = putils.recurse_train(model, batch["slide"], c.top_k_patches, 5)
    _, loss = putils.loss_from_logits(out["logits"], batch, "survival")
    with H.spy_calls() as calls:
        loss.backward()
    sync()
    seen = set(calls)
    missing = sorted(seen - set(DIRECT_TESTS))
    print(f"[coverage] {cfg}: {len(calls)} launches, entry points {sorted(seen)}")
    assert {"paths_colsum_f32", "paths_flush_reductions"} <= seen
    assert not missing, f"backward entry points without a direct test: {missing}"
