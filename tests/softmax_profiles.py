"""Structured score rows for the forward attention kernels' running softmax, and a NumPy model of that softmax.

Every forward attention kernel keeps a running (m, l, O) per query across 64-key steps; the tuned ones defer the rescale, take
exp2 optimistically and revise, and several merge (m, l, O) partials of key splits.  Which of those paths a row takes depends on
WHERE along the key axis its large scores fall - i.i.d. inputs leave that to chance.  Here q, k, v [B, H, T, hd] are built so that
a row's scores follow a chosen profile along the keys and are exact in fp32 and in both operand splits (fp16 hi | lo, bf16 hi | mid |
lo), so that any error belongs to the softmax state and not to the products:

  dimension 0 is a carrier: q[b, h, i, 0] = g(b, i), k[b, h, j, 0] = f_h[j]; the other dimensions are multiples of 1/64 in +-0.25,
  v is uniform in +-1.  f takes multiples of 1/16 (at most 500), g cycles through G_CYCLE with the query index (shifted by the
  slide index, so that the single-query kernels, which read query 0 only, see every g too): one 16-query tile holds rows that rise,
  fall and stay flat, and the wave-wide votes are taken for mixed reasons.  A score is g f + noise with |noise| < 2 a multiple of
  2^-12 and |g f| <= 1000 a multiple of 1/32: 22 bits, and so is every partial sum of it.

Scores are in log2 units (the head-major kernels take q pre-scaled by log2(e) / sqrt(hd): q IS the pre-scaled operand).  For the
token-major kernels (score = qscale q . k) `token_major` divides the carrier by qscale; the product is then exact up to one rounding.

Profiles (PROFILES; f in log2 units, n = the slide's valid length, a key step = 64 keys):
  stairs_up        f = 12 (j // 64): every step's maximum exceeds the running one by 12 g: every step must revise
  slow_ramp        f = j / 16, + 4 per step: the deferral holds (P grows to 2^8) before a revision
  stairs_down      f = -12 (j // 64): nothing revises after step 0 (the rows with g = -1 see stairs_up)
  cliff            f = 0 below key 64, -200 after: nothing revises, the tail underflows exp2
  late_spike       f = 0 but f[n-1] = +40: the spike sits in the masked last step; at n = 64 s + 1 it is that step's only valid key
  late_spike_200   the same with +200: exp2 of the optimistic score is inf, the rescale factor underflows to 0
  in_flight        +40 at key 127 and +80 at key 128: revisions at consecutive steps; the second spike's scores are already computed
                   against the old maximum (in flight) when the first one re-bases
  twin_spikes      +30 at key 1 and at key n-1: two equal maxima that key splits hold in different partials
  offset_up / offset_down   f = +160 / -160 everywhere: with g up to 2, scores of +-320; exp2(s) alone overflows / underflows, only
                   exp2(s - max) means anything; the first step's correction is negative for half of the rows
  masked_max / masked_max_200   late_spike / late_spike_200 with +500 at key n, the first masked key: it is in memory (and finite) and must
                   be ignored
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.attn_ref import LN2, attn_ref_fwd_bwd

LOG2E = math.log2(math.e)
KSTEP = 64
G_CYCLE = (1.0, -1.0, 0.5, 2.0, 0.0)

T = 449                                                   # eight key steps, the last with one key; the pair kernel's ring of four wraps
LENS = (449, 448, 385, 321, 130, 65, 64, 2, 1)
H = 4
# T, valid lengths.  "base": slide ends at every position of a key step and of the kernels' query blocks.  "split": lengths that leave
# at most 32 queries to a 256-query block of the wave-pair kernel (len - 256 k <= 32; csrc/attn_x6.hip: `small`), which then splits
# the KEY steps over its 12 waves and merges: 257 and 288 (five steps: seven waves publish the neutral element), 769 and 800 (13
# steps: wave 0 takes steps 0 and 12); 769 = 64 x 12 + 1 and 257 = 64 x 4 + 1 put the late spike alone into the masked last step.
GEOMS = {"base": (T, LENS), "split": (801, (769, 800, 257, 288))}

PROFILES = ("stairs_up", "slow_ramp", "stairs_down", "cliff",
            "late_spike", "late_spike_200", "in_flight", "twin_spikes",
            "offset_up", "offset_down", "masked_max", "masked_max_200")
# four heads carry four different profiles
BUNDLES = {"steps": PROFILES[0:4], "spikes": PROFILES[4:8], "offsets": PROFILES[8:12]}


def carrier(name: str, n: int, T: int) -> np.ndarray:
    """f [T] (float64, multiples of 1/16) of one slide with n valid keys; keys >= n are padding (only masked_max gives them a meaning)."""
    j = np.arange(T)
    f = np.zeros(T)
    if name == "stairs_up":
        f = 12.0 * (j // KSTEP)
    elif name == "slow_ramp":
        f = j / 16.0
    elif name == "stairs_down":
        f = -12.0 * (j // KSTEP)
    elif name == "cliff":
        f = np.where(j < KSTEP, 0.0, -200.0)
    elif name in ("late_spike", "late_spike_200", "masked_max", "masked_max_200"):
        f[n - 1] = 200.0 if name.endswith("_200") else 40.0
        if name.startswith("masked_max") and n < T:
            f[n] = 500.0
    elif name == "in_flight":
        if T > 127:
            f[127] = 40.0
        if T > 128:
            f[128] = 80.0
    elif name == "twin_spikes":
        if n > 1:
            f[1] = 30.0
        f[n - 1] = 30.0
    elif name == "offset_up":
        f[:] = 160.0
    elif name == "offset_down":
        f[:] = -160.0
    else:
        raise KeyError(name)
    return f.astype(np.float64)


def row_gain(B: int, T: int) -> np.ndarray:
    """g [B, T]: G_CYCLE by (query index + slide index)"""
    b, i = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    return np.asarray(G_CYCLE)[(b + i) % len(G_CYCLE)]


def make_inputs(names, lens=LENS, T: int = T, hd: int = 32, seed: int = 0):
    """q, k, v [B, H, T, hd] float32 (CPU) with head h carrying profile names[h]; head-major convention (scores = q . k, log2 units).
    Padding rows hold finite values like any other row."""
    B, Hh = len(lens), len(names)
    rng = np.random.default_rng(1000 * hd + seed)
    q = rng.integers(-16, 17, size=(B, Hh, T, hd)) / 64.0
    k = rng.integers(-16, 17, size=(B, Hh, T, hd)) / 64.0
    v = rng.uniform(-1.0, 1.0, size=(B, Hh, T, hd))
    q[:, :, :, 0] = row_gain(B, T)[:, None, :]
    for b, n in enumerate(lens):
        for h, name in enumerate(names):
            k[b, h, :, 0] = carrier(name, int(n), T)
    return tuple(torch.from_numpy(x.astype(np.float32)) for x in (q, k, v))


def qscale32(hd: int) -> float:
    """log2(e) / sqrt(hd) as the C ABI passes it: rounded to fp32"""
    return float(np.float32(LOG2E / math.sqrt(hd)))


def token_major(q, k, v, hd: int, spare_rows: int = 128):
    """(q_tm, qkv): q with its carrier divided by qscale (rounded to fp32 once), and the token-major in_proj output [B T + spare, 3 d]
    of q_tm | k | v (spare readable rows behind the last one, as paths_attention_wide_fwd asks for).  The kernels' scores are
    qscale32 * q_tm . k."""
    B, Hh, T, _ = q.shape
    d = Hh * hd
    q_tm = q.clone()
    q_tm[..., 0] = (q[..., 0].double() / qscale32(hd)).float()
    qkv = torch.full((B * T + spare_rows, 3 * d), 0.5)
    for i, x in enumerate((q_tm, k, v)):
        qkv[:B * T, i * d:(i + 1) * d] = x.permute(0, 2, 1, 3).reshape(B * T, d)
    return q_tm, qkv


def reference(q, k, v, lens, score_mul: float = LN2, drop_mask=None, max_queries: int = 0):
    """tests/attn_ref.py in float64: o [B, H, T, hd], lse [B, H, T] (log2 units); rows >= lens[b] are zero."""
    r = attn_ref_fwd_bwd(q, k, v, list(lens), score_mul, torch.zeros_like(q), drop_mask, max_queries)
    return r["o"], r["lse"]


def formula_f32(q, k, v, lens, qmul: float = 1.0, drop_mask=None):
    """The same formula in plain float32 torch (the yardstick of what fp32 itself can do on these inputs): s = (qmul q) k^T,
    p = exp2(s - max), o = (p * mask) v / sum p, lse = max + log2(sum p).  o [B, H, T, hd], lse [B, H, T] float32, zero past lens."""
    B, Hh, T, hd = q.shape
    o = torch.zeros((B, Hh, T, hd))
    lse = torch.zeros((B, Hh, T))
    qm = q * torch.tensor(qmul, dtype=torch.float32)
    for b, n in enumerate(lens):
        n = int(n)
        s = qm[b, :, :n] @ k[b, :, :n].transpose(1, 2)
        m = s.amax(dim=-1, keepdim=True)
        p = torch.exp2(s - m)
        l = p.sum(dim=-1, keepdim=True)
        if drop_mask is not None:
            p = p * drop_mask[b, :, :n, :n].to(p.dtype)
        o[b, :, :n] = (p @ v[b, :, :n]) / l
        lse[b, :, :n] = (m + torch.log2(l))[..., 0]
    return o, lse


# ------------------------------------------------------------------------------------------------
# NumPy model of the running softmax
# ------------------------------------------------------------------------------------------------
FAULTS = ("o_not_rescaled", "in_flight_not_rebased", "masked_key_valid", "no_first_revision", "merge_drops_smaller")


def running_softmax(s, v, n: int, defer: float = 8.0, vote: int = 16, splits: int = 1, fault=None):
    """The optimistic running softmax of csrc/attn_x6.hip in float32: s [nq, >= n] scores (log2 units; columns >= n are masked keys that
    are still in memory), v [>= n, hd].  Per 64-key step the scores arrive relative to the running maximum m (which starts at 0: it is
    subtracted inside the score product) and the NEXT step's scores are computed before this step's softmax, against the same m.
    P = exp2(s) is taken optimistically; a row whose probability sum over the 16 keys of one lane exceeds 2^defer (or is not finite)
    asks for a revision, and so does every row in the first step; `vote` consecutive rows decide together (a wave votes with __any;
    vote = 1: every row for itself).  A revision finds the step's maximum, d = max (first step) or max(max, 0), m += d, and re-bases
    l, O, these scores and the scores in flight by d.  splits > 1: key step kt belongs to worker kt % splits, each worker runs the
    loop over its own steps, and the (m, l, O) partials are merged (a worker without steps holds the neutral element).
    fault: one of FAULTS, planted.  Returns o [nq, hd], lse [nq] (float32) and revised [nq, steps] (bool)."""
    assert fault is None or fault in FAULTS
    f32 = np.float32
    s = np.asarray(s, dtype=f32)
    v = np.asarray(v, dtype=f32)
    nq, hd = s.shape[0], v.shape[1]
    nsteps = (n + KSTEP - 1) // KSTEP
    n_seen = n + 1 if (fault == "masked_key_valid" and n < s.shape[1]) else n      # the last step's mask, off by one
    lane_of_key = (np.arange(KSTEP) // 4) % 4                                         # lane group g4 holds keys 16 t + 4 g4 + r of a step

    def raw(kt):
        blk = np.full((nq, KSTEP), -np.inf, dtype=f32)
        hi = min((kt + 1) * KSTEP, n_seen)
        blk[:, :hi - kt * KSTEP] = s[:, kt * KSTEP:hi]
        return blk

    def vrows(kt):
        blk = np.zeros((KSTEP, hd), dtype=f32)
        hi = min((kt + 1) * KSTEP, n_seen)
        blk[:hi - kt * KSTEP] = v[kt * KSTEP:hi]
        return blk

    revised = np.zeros((nq, nsteps), dtype=bool)
    parts = []
    with np.errstate(all="ignore"):
        for w in range(splits):
            steps = list(range(w, nsteps, splits))
            m = np.zeros(nq, dtype=f32)
            l = np.zeros(nq, dtype=f32)
            O = np.zeros((nq, hd), dtype=f32)
            if not steps:
                parts.append((np.full(nq, -1e30, dtype=f32), l, O))
                continue
            sn = raw(steps[0]) - m[:, None]
            for idx, kt in enumerate(steps):
                sc = sn
                if idx + 1 < len(steps):
                    sn = raw(steps[idx + 1]) - m[:, None]                             # in flight: relative to the maximum of NOW
                p = np.exp2(sc)
                lane_sums = np.stack([p[:, lane_of_key == g].sum(axis=1) for g in range(4)], axis=1)
                want = ~(lane_sums.max(axis=1) <= f32(2.0 ** defer))                  # (also true for NaN)
                first = idx == 0 and fault != "no_first_revision"
                grp = np.arange(nq) // vote
                rev = np.zeros(nq, dtype=bool)
                for g_ in np.unique(grp):
                    rev[grp == g_] = first or bool(want[grp == g_].any())
                mx = sc.max(axis=1)
                d = np.where(rev, mx if first else np.maximum(mx, f32(0)), f32(0)).astype(f32)
                alpha = np.ones(nq, dtype=f32) if first else np.exp2(-d)
                l = l * alpha
                if fault != "o_not_rescaled":
                    O = O * alpha[:, None]
                m = m + d
                sc = sc - d[:, None]
                if fault != "in_flight_not_rebased" or first:            # (planted at the later revisions: any input sees the first)
                    sn = sn - d[:, None]
                p = np.exp2(sc)
                l = l + p.sum(axis=1, dtype=f32)
                O = O + p @ vrows(kt)
                revised[:, kt] = rev
            parts.append((m, l, O))
        M = np.max(np.stack([pm for pm, _, _ in parts]), axis=0)
        l = np.zeros(nq, dtype=f32)
        O = np.zeros((nq, hd), dtype=f32)
        for pm, pl, pO in parts:
            sc = np.exp2(pm - M)
            if fault == "merge_drops_smaller":
                sc = np.where(pm == M, f32(1), f32(0)).astype(f32)
            l = l + pl * sc
            O = O + pO * sc[:, None]
        o = O / l[:, None]
        lse = M + np.log2(l)
    return o.astype(f32), lse.astype(f32), revised
