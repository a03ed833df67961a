"""The inputs of tests/test_gpu_softmax_profiles.py do what they claim, checked without a GPU (tests/softmax_profiles.py):

  exactness       the fp32 q k^T of every profile equals the float64 product bit for bit, and every operand survives the fp16 hi | lo
                  and the bf16 hi | mid | lo split unchanged: an error on these inputs belongs to the softmax state;
  forced paths    the NumPy model of the running softmax reports which key steps revise: asserted exactly, so that a later change
                  to a profile cannot quietly stop exercising its path;
  discrimination  the model with one planted fault at a time misses the float64 reference by at least 10x the GPU test's bar on a
                  NAMED profile; without a fault it is inside the bar on every profile;
  reference       tests/attn_ref.py is finite on every profile, and so is the float32 yardstick formula.
"""
import functools

import numpy as np
import pytest
import torch

from tests import softmax_profiles as SP

BAR = 2e-6                     # the head-major kernels' bar on o in tests/test_gpu_softmax_profiles.py (absolute)
G = np.asarray(SP.G_CYCLE)


@functools.lru_cache(maxsize=None)
def bundle(name, hd=32, geom="base"):
    names = SP.BUNDLES[name]
    T, lens = SP.GEOMS[geom]
    q, k, v = SP.make_inputs(names, lens, T, hd)
    o, lse = SP.reference(q, k, v, lens)
    return names, q, k, v, o, lse


def profile(name):
    """(q, k, v, o64, lse64) [B, T, ..] of one profile's head"""
    for bname, names in SP.BUNDLES.items():
        if name in names:
            _, q, k, v, o, lse = bundle(bname)
            h = names.index(name)
            return q[:, h], k[:, h], v[:, h], o[:, h], lse[:, h]
    raise KeyError(name)


def test_bundles_cover_every_profile_once():
    assert sorted(n for names in SP.BUNDLES.values() for n in names) == sorted(SP.PROFILES)
    assert all(len(names) == SP.H for names in SP.BUNDLES.values())
    assert SP.T == 7 * 64 + 1 and SP.LENS[0] == SP.T                 # eight key steps, the last with one key
    assert all(0 < n <= SP.T for n in SP.LENS)


def split_f16(x):
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.float() + lo.float()


def split_bf16(x):
    hi = x.to(torch.bfloat16)
    mid = (x - hi.float()).to(torch.bfloat16)
    lo = (x - hi.float() - mid.float()).to(torch.bfloat16)
    return (hi.float() + mid.float()) + lo.float()


@pytest.mark.parametrize("hd,geom", [(16, "base"), (32, "base"), (48, "base"), (64, "base"), (96, "base"), (32, "split")])
@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_scores_are_exact_in_fp32_and_in_both_operand_splits(bname, hd, geom):
    names, q, k, v, o64, lse64 = bundle(bname, hd, geom)
    T, lens = SP.GEOMS[geom]
    assert torch.isfinite(o64).all() and torch.isfinite(lse64).all()
    s32 = q @ k.transpose(-1, -2)                                    # every key of the buffer, masked ones included
    s64 = q.double() @ k.double().transpose(-1, -2)
    assert torch.equal(s32.double(), s64)
    # in another summation order too (the kernels sum the head dimension in MFMA order): reversed
    s32r = q.flip(-1) @ k.flip(-1).transpose(-1, -2)
    assert torch.equal(s32r.double(), s64)
    for x in (q, k):
        assert torch.equal(split_f16(x), x) and torch.equal(split_bf16(x), x)
    # the token-major form loses exactly one rounding: of g / qscale
    q_tm, qkv = SP.token_major(q, k, v, hd)
    assert torch.equal(q_tm[..., 1:], q[..., 1:])
    back = q_tm[..., 0].double() * SP.qscale32(hd)
    assert float((back - q[..., 0].double()).abs().max()) <= 2.0 ** -24 * 2.0
    assert qkv.shape == (len(lens) * T + 128, 3 * SP.H * hd) and torch.isfinite(qkv).all()


@pytest.mark.parametrize("bname", sorted(SP.BUNDLES))
def test_references_are_finite_on_every_profile(bname):
    names, q, k, v, o, lse = bundle(bname)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o32, lse32 = SP.formula_f32(q, k, v, SP.LENS)
    assert torch.isfinite(o32).all() and torch.isfinite(lse32).all()
    for b, n in enumerate(SP.LENS):
        assert float((o32[b, :, :n].double() - o[b, :, :n]).abs().max()) < BAR
        assert not o[b, :, n:].any() and not lse[b, :, n:].any()
    # token-major: the same rows up to the rounding of g / qscale
    q_tm, _ = SP.token_major(q, k, v, 32)
    o_tm, lse_tm = SP.reference(q_tm, k, v, SP.LENS, SP.qscale32(32) * SP.LN2)
    assert torch.isfinite(o_tm).all() and torch.isfinite(lse_tm).all()


def model(name, b=0, nq=80, **kw):
    """The model on the first nq queries of slide b of one profile: (o, lse, revised, err of o against float64, g of the rows)"""
    q, k, v, o64, lse64 = profile(name)
    n = SP.LENS[b]
    nq = min(nq, n)
    s = (q[b, :nq] @ k[b].T).numpy()                                  # exact; every key in memory
    o, lse, rev = SP.running_softmax(s, v[b].numpy(), n, **kw)
    if np.isfinite(o).all():
        err = float(np.abs(o.astype(np.float64) - o64[b, :nq].numpy()).max())
    else:
        err = float("inf")
    return o, lse, rev, err, SP.row_gain(len(SP.LENS), SP.T)[b, :nq]


@pytest.mark.parametrize("name", SP.PROFILES)
@pytest.mark.parametrize("splits,vote", [(1, 16), (1, 1), (4, 16), (12, 16)])
def test_model_without_a_fault_is_inside_the_bar(name, splits, vote):
    for b in (0, 1, 4, 5, 8):                                         # 449, 448, 130, 65, 1 keys
        o, lse, _, err, _ = model(name, b, splits=splits, vote=vote)
        assert err < BAR, (name, b, err)
        _, _, _, _, lse64 = profile(name)
        assert float(np.abs(lse.astype(np.float64) - lse64[b, :len(lse)].numpy()).max()) < 1e-4


def test_stairs_up_revises_at_every_step_for_the_rising_rows():
    _, _, rev, _, g = model("stairs_up", vote=1)
    assert rev.shape[1] == 8
    assert rev[g >= 1].all()
    # g = 0.5 climbs 6 per step: 16 keys of a lane sum to 2^10, but the last step of 449 keys holds ONE key (2^6): kept
    assert rev[g == 0.5][:, :7].all() and not rev[g == 0.5][:, 7].any()
    assert rev[g <= 0][:, 0].all() and not rev[g <= 0][:, 1:].any()
    _, _, rev448, _, g448 = model("stairs_up", b=1, vote=1)          # 448 keys: seven full steps
    assert rev448.shape[1] == 7 and rev448[g448 > 0].all()
    _, _, rev16, _, _ = model("stairs_up", vote=16)                  # a wave votes: the falling and flat rows are carried along
    assert rev16.all()


def test_stairs_down_never_revises():
    _, _, rev, _, g = model("stairs_down", vote=1)
    assert rev[:, 0].all()                                           # (the first step always does: m starts at 0)
    assert not rev[g >= 0][:, 1:].any()
    assert rev[g < 0].all()                                          # the rows with g = -1 climb the stairs instead
    _, _, rev_c, _, g = model("cliff", vote=1)
    assert not rev_c[g >= 0][:, 1:].any()


def test_slow_ramp_defers_then_revises():
    _, _, rev, _, g = model("slow_ramp", vote=1)
    r1 = rev[g == 1.0]
    assert not r1[:, 1].any() and r1[:, 2].all()                     # + 4 is kept, + 8 is not
    assert not rev[g <= 0][:, 1:].any()


def test_in_flight_revises_at_two_consecutive_steps():
    _, _, rev, _, g = model("in_flight", vote=1)
    up = rev[g > 0]
    assert up[:, 1].all() and up[:, 2].all()                         # key 127 ends step 1, key 128 opens step 2
    assert not up[:, 3:].any()
    assert not rev[g <= 0][:, 1:].any()


@pytest.mark.parametrize("name", ["late_spike", "late_spike_200", "masked_max", "masked_max_200"])
def test_late_spike_revises_in_the_last_step(name):
    for b in (0, 1, 2):                                              # 449 = 7 x 64 + 1: the spike is the last step's only valid key
        _, _, rev, _, g = model(name, b, vote=1)
        up = rev[g > 0]
        assert up[:, -1].all() and not up[:, 1:-1].any(), (name, b)
        assert not rev[g <= 0][:, 1:].any()


def test_offsets_take_a_negative_first_correction():
    for name in ("offset_up", "offset_down"):
        q, k, v, _, lse64 = profile(name)
        s0 = (q[0, :80] @ k[0, :64].T).amax(dim=-1)
        assert (s0 < -100).any() and (s0 > 100).any()               # the first step's d is far below 0 for some rows of one tile
        assert float(lse64[0].abs().max()) > 300


# fault -> (profile that must see it, slide, model arguments)
SEEN_BY = {
    "o_not_rescaled": ("stairs_up", 0, {}),
    "in_flight_not_rebased": ("slow_ramp", 0, {}),
    "masked_key_valid": ("masked_max", 2, {}),                # 385 = 6 x 64 + 1 keys: key 385 is in the last step
    "no_first_revision": ("offset_down", 0, {}),
    "merge_drops_smaller": ("twin_spikes", 0, {"splits": 4}),
}


@pytest.mark.parametrize("fault", SP.FAULTS)
def test_each_planted_fault_is_seen_by_its_profile(fault):
    name, b, kw = SEEN_BY[fault]
    _, _, _, clean, _ = model(name, b, **kw)
    _, _, _, err, _ = model(name, b, fault=fault, **kw)
    print(f"[profiles] {fault} on {name}: {err:.3e} (without the fault {clean:.3e})")
    assert clean < BAR
    assert err >= 10 * BAR, f"{fault} is not seen by {name}: {err:.3e}"


def test_every_fault_is_named_and_some_profiles_are_blind_to_it():
    """Which profiles see which fault (printed with -s): the table the SEEN_BY choices come from.  i.i.d.-like rows (the g = 0 rows:
    noise only) see none of the revision faults."""
    assert set(SEEN_BY) == set(SP.FAULTS)
    seen = {}
    for fault in SP.FAULTS:
        kw = {"splits": 4} if fault == "merge_drops_smaller" else {}
        seen[fault] = [n for n in SP.PROFILES if model(n, 2, fault=fault, **kw)[3] >= 10 * BAR]
        print(f"[profiles] {fault}: {seen[fault]}")
        assert seen[fault]
    for fault in ("o_not_rescaled", "in_flight_not_rebased"):
        q, k, v, o64, _ = profile("stairs_up")
        rows = np.nonzero(SP.row_gain(len(SP.LENS), SP.T)[0, :80] == 0.0)[0]
        s = (q[0, rows] @ k[0].T).numpy()
        o, _, rev = SP.running_softmax(s, v[0].numpy(), SP.LENS[0], vote=1, fault=fault)
        assert not rev[:, 1:].any()
        assert float(np.abs(o - o64[0, rows].numpy()).max()) < BAR
