"""The undefined-memory harness (tests/poison.py) itself, on the CPU: the fills are the stated bit patterns, the patch comes off
again, integer tensors stay as they are, the guard bands notice a stray write, and the comparison tells a function that reads what
it never wrote from one that does not."""
import math

import pytest
import torch

from tests import poison as P


def _words(t):
    return t.contiguous().view(-1).view(P._INT_VIEW[t.dtype]).tolist()


def _u(words, bits):
    return [w & ((1 << bits) - 1) for w in words]


def test_hostile_fills_are_the_stated_bit_patterns():
    assert P.HOSTILE_F32[3] == (torch.tensor(3.0e38, dtype=torch.float32).view(torch.int32).item() & 0xFFFFFFFF)
    assert P.HOSTILE_F16[3] == (torch.tensor(65504.0, dtype=torch.float16).view(torch.int16).item() & 0xFFFF)
    with P.poisoned_empty("H"):
        a = torch.empty((3, 7), dtype=torch.float32)
        h = torch.empty((9,), dtype=torch.float16)
        b = torch.empty((6,), dtype=torch.bfloat16)
        u = torch.empty((37,), dtype=torch.uint8)
    assert _u(_words(a), 32) == [(0x7FC00000, 0x7F800000, 0xFF800000, 0x7F61B1E6, 0x7F800001)[i % 5] for i in range(21)]
    assert _u(_words(h), 16) == [(0x7E00, 0x7C00, 0xFC00, 0x7BFF)[i % 4] for i in range(9)]
    assert _u(_words(b), 16) == [(0x7FC0, 0x7F80, 0xFF80, 0x7F7F)[i % 4] for i in range(6)]
    assert u.tolist() == [0xFF] * 37
    # the cycle as values: NaN, +Inf, -Inf, a large finite number, NaN
    v = a.view(-1)[:5].tolist()
    assert math.isnan(v[0]) and v[1] == math.inf and v[2] == -math.inf and v[3] == pytest.approx(3.0e38) and math.isnan(v[4])
    assert float(h[3]) == 65504.0 and math.isnan(float(h[0]))
    # 0xff bytes read as NaN in every float format an image may hold
    raw = torch.full((8,), 0xFF, dtype=torch.uint8)
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn):
        assert bool(torch.isnan(raw.view(dt).float()).all()), dt


def test_hostile_cycle_continues_over_a_buffer_larger_than_the_bank():
    n = P._BANK * 2 + 13
    with P.poisoned_empty("H"):
        a = torch.empty((n,), dtype=torch.float32)
    w = a.view(torch.int32)
    want = torch.tensor(P._signed(P.HOSTILE_F32, 32), dtype=torch.int32).repeat(n // 5 + 1)[:n]
    assert torch.equal(w, want)


def test_zero_and_finite_fills():
    with P.poisoned_empty("Z"):
        z = [torch.empty((5, 3), dtype=dt) for dt in P.FILLED]
    for t in z:
        assert t.view(-1).view(torch.uint8).count_nonzero() == 0
    with P.poisoned_empty("F") as sites:
        f = [torch.empty((4099,), dtype=dt) for dt in (torch.float32, torch.float16, torch.bfloat16)]
        u = torch.empty((4096,), dtype=torch.uint8)
        again = torch.empty((4099,), dtype=torch.float32)
    for t in f:
        x = t.double()
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) <= 2.0 and float(x.std()) > 0.5
    assert not torch.equal(f[0], again), "two call sites get different noise"
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn):
        x = u.view(dt).double()
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) <= 2.0, dt
    assert len(set(u.tolist())) > 64
    with P.poisoned_empty("F"):
        f2 = torch.empty((4099,), dtype=torch.float32)
    assert torch.equal(f[0], f2), "F is seeded: the same sequence of calls gets the same noise"
    assert len(sites) == 5


def test_every_replaced_allocator_fills_and_records():
    base = torch.zeros((4, 6), dtype=torch.float32)
    with P.poisoned_empty("H") as sites:
        a = torch.empty(4, 6)
        b = torch.empty_like(base)
        c = torch.empty_strided((4, 3), (6, 2), dtype=torch.float32)
        d = base.new_empty((2, 5))
        e = base.new_empty((3,), dtype=torch.float16)
    for t in (a, b, c, d, e):
        assert bool((~torch.isfinite(t.float())).any()), "filled"
    assert c.stride() == (6, 2)
    assert [s[0] for s in sites] == [__name__] * 5
    lines = [s[1] for s in sites]
    assert lines == sorted(lines) and len(set(lines)) == 5
    assert [s[2] for s in sites] == [torch.float32] * 4 + [torch.float16]
    assert [s[3] for s in sites] == [96, 96, 48, 40, 6]
    assert sites.modules() == {__name__} and sites.filled_bytes() == 286


def test_originals_are_back_on_exit_and_after_an_exception():
    orig = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    assert not P.is_patched()
    with P.poisoned_empty("H"):
        assert P.is_patched() and torch.empty is not orig[0] and torch.Tensor.new_empty is not orig[3]
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig and not P.is_patched()
    with pytest.raises(RuntimeError, match="boom"):
        with P.poisoned_empty("F"):
            torch.empty(3)
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig and not P.is_patched()
    with pytest.raises(AssertionError):
        with P.poisoned_empty("Q"):
            pass
    assert not P.is_patched()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.int16, torch.bool, torch.float64])
def test_integer_tensors_are_left_alone(dtype):
    """Index, count and address buffers are never filled: under every pattern the replacement returns them as the original made
    them.  (What torch.empty leaves in them cannot be asserted; that fill_ does not touch a tensor of the dtype can.)"""
    t = torch.arange(24).to(dtype).view(4, 6)
    keep = t.clone()
    for pat in P.PATTERNS:
        assert P.fill_(t, pat) is t and torch.equal(t, keep)
    with P.poisoned_empty("H") as sites:
        x = torch.empty((4, 6), dtype=dtype)
        y = t.new_empty((5,))
    assert x.dtype == dtype and y.dtype == dtype and sites.filled_bytes() == 0 and len(sites) == 2
    if dtype in (torch.int32, torch.int64):
        g = P.guarded((7,), dtype, "H")
        assert g.tolist() == [0] * 7
        P.check_guards()


def test_guarded_buffers_are_exact_aligned_and_banded():
    for nbytes in (1, 16, 100, 4096, 4100):
        for pat in P.PATTERNS:
            g = P.guarded(nbytes, torch.uint8, pat)
            assert g.shape == (nbytes,) and g.dtype == torch.uint8 and g.data_ptr() % 16 == 0 and g.is_contiguous()
            whole, lo, hi = P._guards[-1]
            assert lo >= 4096 and whole.numel() - hi >= 4096 and hi - lo == nbytes
            assert g.data_ptr() == whole.data_ptr() + lo
            if pat == "H":
                assert g.tolist() == [0xFF] * nbytes
    f = P.guarded((3, 5), torch.float32, "H")
    assert f.shape == (3, 5) and _u(_words(f), 32)[:5] == list(P.HOSTILE_F32)
    h = P.guarded((7,), torch.float16, "F")
    assert bool(torch.isfinite(h.float()).all())
    f.zero_()                                              # writing the whole view is fine
    assert P.check_guards() == 17
    assert P._guards == []


@pytest.mark.parametrize("where", ["before", "behind", "slack"])
def test_check_guards_notices_one_stray_byte(where):
    g = P.guarded(100, torch.uint8, "Z")
    whole, lo, hi = P._guards[-1]
    whole[{"before": lo - 1, "behind": whole.numel() - 1, "slack": hi}[where]] ^= 1
    with pytest.raises(AssertionError, match="wrote outside"):
        P.check_guards("toy")
    assert P._guards == [] and g.numel() == 100


def test_poisoned_empty_can_put_its_results_between_guard_bands():
    """guard=True: what torch.empty returns has exactly the size asked for, holds the pattern and sits between bands that
    check_guards() watches - an existing builder's workspace, sized by a query, becomes a guarded one."""
    with P.poisoned_empty("H", guard=True) as sites:
        ws = torch.empty((1000,), dtype=torch.uint8)
        x = torch.empty((3, 5), dtype=torch.float32)
        idx = torch.empty((7,), dtype=torch.int64)
    assert ws.shape == (1000,) and ws.tolist() == [0xFF] * 1000 and x.shape == (3, 5) and _u(_words(x), 32)[:5] == list(P.HOSTILE_F32)
    assert len(P._guards) == 2 and len(sites) == 3 and idx.dtype == torch.int64, "integer tensors get no guard band either"
    assert ws.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    ws.zero_()
    assert P.check_guards() == 2
    with P.poisoned_empty("Z", guard=True):
        ws = torch.empty((1000,), dtype=torch.uint8)
    whole, lo, hi = P._guards[-1]
    whole[hi + 3] = 0                                     # one byte behind the 1000 the "kernel" was given
    with pytest.raises(AssertionError, match="wrote outside"):
        P.check_guards("toy")


# ------------------------------------------------------------------------------------------------
# negative control: the comparison bites
# ------------------------------------------------------------------------------------------------
def _sums_what_it_never_wrote(pattern):
    """A 'kernel' with the bug these tests are after: rows 5.. of its workspace are never written, and the reduction runs over all."""
    with P.poisoned_empty(pattern):
        ws = torch.empty((8, 4), dtype=torch.float32)
    ws[:5] = torch.arange(20, dtype=torch.float32).view(5, 4)
    return {"sum": ws.sum(dim=0), "rows": ws[:5]}


def _multiplies_by_a_zero_mask(pattern):
    """The other shape of the bug: a mask applied as a multiplication - 0 * NaN is NaN, 0 * finite is 0, so only H tells."""
    with P.poisoned_empty(pattern):
        v = torch.empty((8, 4), dtype=torch.float32)
    v[:5] = 1.0
    mask = (torch.arange(8) < 5).float()[:, None]
    return {"sum": (v * mask).sum(dim=0)}


def _writes_it_fully(pattern):
    with P.poisoned_empty(pattern):
        ws = torch.empty((8, 4), dtype=torch.float32)
        out = torch.empty((4,), dtype=torch.float32)
    ws[:5] = torch.arange(20, dtype=torch.float32).view(5, 4)
    ws[5:] = 0.0
    torch.sum(ws, dim=0, out=out)
    return {"sum": out, "rows": ws[:5]}


def _selects(pattern):
    with P.poisoned_empty(pattern):
        v = torch.empty((8, 4), dtype=torch.float32)
    v[:5] = 1.0
    keep = (torch.arange(8) < 5)[:, None]
    return {"sum": torch.where(keep, v, torch.zeros(())).sum(dim=0)}


def test_negative_control_a_read_of_unwritten_memory_is_reported():
    found = P.dependences(_sums_what_it_never_wrote)
    assert found == {"F#2": ["sum"], "H#3": ["sum"]}, found            # Z against Z agrees, "rows" is defined and agrees
    assert P.dependences(_sums_what_it_never_wrote, runs=("Z", "H")) == {"H#1": ["sum"]}
    with pytest.raises(AssertionError, match="depends on undefined memory"):
        P.assert_independent(_sums_what_it_never_wrote, "toy")
    # a multiplicative mask hides behind finite garbage; only the hostile pattern shows it
    assert P.dependences(_multiplies_by_a_zero_mask) == {"H#3": ["sum"]}


def test_negative_control_full_writes_and_selects_pass():
    assert P.dependences(_writes_it_fully) == {}
    assert P.dependences(_selects) == {}
    first = P.assert_independent(_writes_it_fully, "toy")
    assert first["sum"].tolist() == [40.0, 45.0, 50.0, 55.0]


def test_a_nondeterministic_function_is_reported_as_such():
    calls = []

    def flaky(pattern):
        calls.append(pattern)
        return {"x": torch.full((3,), float(len(calls)))}

    with pytest.raises(AssertionError, match="determinism is broken"):
        P.assert_independent(flaky, "toy")


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan")])
    assert P.same_bits(a, a.clone())
    assert not P.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    q = torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.float32)
    s = torch.tensor([0x7FC00007], dtype=torch.int32).view(torch.float32)
    assert not P.same_bits(q, s) and P.same_bits(s, s.clone())
    assert not P.same_bits(torch.zeros(3), torch.zeros(4)) and not P.same_bits(torch.zeros(3), torch.zeros(3, dtype=torch.float16))
    assert P.same_bits(torch.zeros((0, 4)), torch.zeros((0, 4)))
