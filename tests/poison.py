"""Harness for the undefined-memory tests: what a kernel may look at, as opposed to what it computes.

The package allocates its workspaces, operand images, saved activations and per-level state with torch.empty, and a caller of
the C library brings buffers of its own.  Whatever such memory holds on entry in a place the contract leaves undefined - padded rows,
pad columns, workspaces, read-behind zones - must not reach the defined part of any output.  The project has no float atomics, so the
criterion is exact: the defined outputs are bit-identical whatever the undefined memory held.

Fill patterns (by dtype):
  Z  all zero bytes
  F  seeded finite noise in [-2, 2] (uint8: bytes that read as a finite value of magnitude below 2 in fp32, fp16, bf16 and e4m3)
  H  hostile: fp32 a repeating cycle of quiet NaN 0x7fc00000, +Inf, -Inf, 3.0e38 and the NaN 0x7f800001; fp16 0x7e00, 0x7c00, 0xfc00,
     65504; bf16 the same four kinds; uint8 0xff bytes, which read as NaN in fp32, fp16, bf16 and e4m3

poisoned_empty(pattern) replaces torch.empty, torch.empty_like, torch.empty_strided and Tensor.new_empty for the duration of a
``with`` block (inside a test, never in a conftest.py) by versions that fill float32, float16, bfloat16 and uint8 results with the
pattern and record (module, line, dtype, bytes) of the call site.

INTEGER TENSORS ARE LEFT ALONE, DELIBERATELY.  int32 / int64 buffers hold indices, counts and row ADDRESSES (x_rows, hp_row,
kept_rows): a hostile value followed by a kernel would be a wild address, and these tests must not be able to fault a GPU.  Garbage
in padded index entries is covered where it is safe (tests/test_gpu_removal.py::_garbage, tests/test_gpu_select.py).  bool and
float64 tensors are left alone as well (the package allocates neither on a kernel's path).

guarded(nbytes_or_shape, dtype, pattern) returns a pattern-filled tensor of exactly the size asked for, placed 16-byte aligned
inside a larger buffer whose bands of at least 4 KiB before and behind it hold a sentinel; check_guards() asserts that every band
handed out since the last check still holds it.  The sentinel word is NAN_FILL of tests/test_gpu_chain_forward.py."""
import contextlib
import sys

import torch

GUARD_WORD = 0x7FC00007            # = tests/test_gpu_chain_forward.py:NAN_FILL (importing that module needs the GPU fixtures)
GUARD_BYTES = 4096
PATTERNS = ("Z", "F", "H")
RUNS = ("Z", "Z", "F", "H")        # the four runs of the end-to-end tests: the second Z separates "not deterministic" from "depends"
HOSTILE_F32 = (0x7FC00000, 0x7F800000, 0xFF800000, 0x7F61B1E6, 0x7F800001)       # qNaN, +Inf, -Inf, 3.0e38, a NaN with payload 1
HOSTILE_F16 = (0x7E00, 0x7C00, 0xFC00, 0x7BFF)                                   # qNaN, +Inf, -Inf, 65504
HOSTILE_BF16 = (0x7FC0, 0x7F80, 0xFF80, 0x7F7F)                                  # qNaN, +Inf, -Inf, the largest finite value
FILLED = (torch.float32, torch.float16, torch.bfloat16, torch.uint8)
_INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
_BANK = 1 << 16
_banks = {}
# the originals, bound once: the replacements and the fills below never go through a patched name
_EMPTY, _EMPTY_LIKE, _EMPTY_STRIDED, _NEW_EMPTY = torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty


def _signed(words, bits):
    return [w - (1 << bits) if w >= 1 << (bits - 1) else w for w in words]


def _bank(pattern, dtype, device):
    """About _BANK elements of the pattern in ``dtype`` on ``device`` (cached; a fill tiles it, F from an offset its seed chooses)."""
    key = (pattern, dtype, str(device))
    if key not in _banks:
        if pattern == "F":
            g = torch.Generator().manual_seed(0x5EED)
            if dtype == torch.uint8:
                # high bit = sign, 0..0x3f below it: |value| < 2 as an e4m3 byte and as the top byte of an fp16 / bf16 / fp32 word
                b = torch.randint(0, 0x40, (_BANK,), generator=g, dtype=torch.int32) + 0x80 * torch.randint(0, 2, (_BANK,), generator=g, dtype=torch.int32)
                bank = b.to(torch.uint8)
            else:
                bank = (torch.rand((_BANK,), generator=g, dtype=torch.float32) * 4 - 2).to(dtype)
        else:
            words, bits = {torch.float32: (HOSTILE_F32, 32), torch.float16: (HOSTILE_F16, 16), torch.bfloat16: (HOSTILE_BF16, 16)}[dtype]
            cyc = torch.tensor(_signed(words, bits), dtype=_INT_VIEW[dtype])
            bank = cyc.repeat(_BANK // len(words) + 1)[:_BANK // len(words) * len(words)].view(dtype)
        _banks[key] = bank.to(device)
    return _banks[key]


def fill_(t, pattern, seed=0):
    """Fill every byte of ``t``'s elements with the pattern (in place, on the current stream); other dtypes than FILLED are left alone."""
    assert pattern in PATTERNS, pattern
    if t.dtype not in FILLED or t.numel() == 0:
        return t
    if pattern == "Z":
        return t.zero_()
    if pattern == "H" and t.dtype == torch.uint8:
        return t.fill_(0xFF)
    bank = _bank(pattern, t.dtype, t.device)
    n, off = t.numel(), (seed * 7919) % (_BANK // 2) if pattern == "F" else 0
    flat = bank[off:off + n] if off + n <= bank.numel() else bank.repeat((off + n + bank.numel() - 1) // bank.numel())[off:off + n]
    if t.is_contiguous():
        t.view(-1).copy_(flat)
    else:
        t.copy_(flat.view(t.shape))
    return t


class Sites(list):
    """The recorded call sites: (module, line, dtype, bytes) per call."""

    def modules(self):
        return {s[0] for s in self}

    def filled_bytes(self):
        return sum(s[3] for s in self if s[2] in FILLED)


@contextlib.contextmanager
def poisoned_empty(pattern, seed=0, guard=False):
    """torch.empty / empty_like / empty_strided / Tensor.new_empty fill what they return with ``pattern`` (FILLED dtypes only) and
    record their call sites; yields the record.  The originals are back on exit, also after an exception.

    ``guard``: every contiguous result of a FILLED dtype is a guarded() buffer of exactly the size asked for (so a test can run an
    existing problem builder and have each workspace it sizes with a query sit between guard bands); check_guards() afterwards."""
    assert pattern in PATTERNS, pattern
    sites = Sites()

    def wrap(orig):
        def poisoned(*a, **kw):
            t = orig(*a, **kw)
            f = sys._getframe(1)
            sites.append((f.f_globals.get("__name__", "?"), f.f_lineno, t.dtype, t.numel() * t.element_size()))
            if t.is_meta:
                return t
            with torch.no_grad():
                if guard and t.dtype in FILLED and t.is_contiguous() and not t.requires_grad and t.device.type != "meta":
                    return guarded(tuple(t.shape), t.dtype, pattern, device=t.device, seed=seed + len(sites))
                fill_(t, pattern, seed + len(sites))
            return t
        poisoned.__wrapped__ = orig
        return poisoned

    saved = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    torch.empty, torch.empty_like, torch.empty_strided = wrap(saved[0]), wrap(saved[1]), wrap(saved[2])
    torch.Tensor.new_empty = wrap(saved[3])
    try:
        yield sites
    finally:
        torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty = saved


def is_patched():
    return any(f is not o for f, o in zip((torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty),
                                          (_EMPTY, _EMPTY_LIKE, _EMPTY_STRIDED, _NEW_EMPTY)))


# ------------------------------------------------------------------------------------------------
# guard bands
# ------------------------------------------------------------------------------------------------
_guards = []


def guarded(nbytes_or_shape, dtype=torch.uint8, pattern="Z", device="cpu", seed=0):
    """A ``pattern``-filled contiguous tensor of ``dtype`` - [nbytes] for an int (dtype uint8 then), else of the given shape - whose
    storage lies 16-byte aligned inside a larger sentinel-filled buffer with at least GUARD_BYTES of it on each side.  Integer
    dtypes are zero-filled (this module never poisons them)."""
    shape = (int(nbytes_or_shape),) if isinstance(nbytes_or_shape, int) else tuple(int(s) for s in nbytes_or_shape)
    n = 1
    for s in shape:
        n *= s
    nbytes = n * _EMPTY((), dtype=dtype).element_size()
    body = (nbytes + 15) // 16 * 16                     # the band behind starts at the next 16-byte boundary: at most 15 slack bytes,
    whole = torch.full(((2 * GUARD_BYTES + body) // 4,), GUARD_WORD, dtype=torch.int32, device=device).view(torch.uint8)   # and they hold the sentinel too
    assert whole.data_ptr() % 16 == 0
    view = whole[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0 and view.data_ptr() == whole.data_ptr() + GUARD_BYTES
    if dtype in FILLED:
        fill_(view, pattern, seed)
    else:
        view.zero_()
    _guards.append((whole, GUARD_BYTES, GUARD_BYTES + nbytes))
    return view


def _band_ok(whole, lo, hi):
    """Both bands of one guarded buffer still hold the sentinel (the slack bytes up to the next word boundary included)."""
    want = torch.full((whole.numel() // 4,), GUARD_WORD, dtype=torch.int32, device=whole.device).view(torch.uint8)
    return bool((whole[:lo] == want[:lo]).all()) and bool((whole[hi:] == want[hi:]).all())


def check_guards(label=""):
    """Every guard band handed out since the last call is untouched; forgets them."""
    bad = [i for i, g in enumerate(_guards) if not _band_ok(*g)]
    sizes = [g[2] - g[1] for g in _guards]
    del _guards[:]
    assert not bad, f"{label}: a kernel wrote outside guarded buffer(s) {bad} (sizes in bytes: {[sizes[i] for i in bad]})"
    return len(sizes)


# ------------------------------------------------------------------------------------------------
# comparing runs
# ------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Two tensors of one dtype and shape hold the same bytes (NaN payloads and the sign of zero count)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.numel() == 0:
        return True
    return bool((a.view(-1).view(torch.uint8) == b.view(-1).view(torch.uint8)).all())


def differing(base, other):
    """Names of the entries of two {name: tensor} dicts of defined outputs that are not bit-identical."""
    assert set(base) == set(other), (sorted(base), sorted(other))
    return sorted(k for k in base if not same_bits(base[k], other[k]))


def run_patterns(fn, runs=RUNS):
    """fn(pattern) -> {name: tensor of defined outputs} once per entry of ``runs``; returns the list of results (each cloned, so a
    later run cannot overwrite an earlier one's memory)."""
    out = []
    for k, pat in enumerate(runs):
        res = fn(pat)
        out.append({name: t.detach().clone() for name, t in res.items()})
    return out


def dependences(fn, runs=RUNS):
    """{pattern: names of the defined outputs of fn(pattern) that differ from the first run's}.  Empty = independent of the undefined
    memory (and deterministic, where ``runs`` repeats its first pattern)."""
    res = run_patterns(fn, runs)
    found = {}
    for k in range(1, len(runs)):
        d = differing(res[0], res[k])
        if d:
            found[f"{runs[k]}#{k}"] = d
    return found


def assert_independent(fn, label, runs=RUNS, finite_under_h=True):
    """The defined outputs of fn(pattern) are bit-identical over ``runs``: a repeat of the first pattern that differs is reported as
    broken determinism, another pattern that differs as a dependence on undefined memory.  Returns the first run's results."""
    res = run_patterns(fn, runs)
    for k in range(1, len(runs)):
        d = differing(res[0], res[k])
        if runs[k] == runs[0]:
            assert not d, f"{label}: determinism is broken - two {runs[0]} runs differ in {d}"
        else:
            assert not d, f"{label}: depends on undefined memory - {d} differ between {runs[0]} and {runs[k]}"
    if finite_under_h and "H" in runs:
        h = res[runs.index("H")]
        bad = sorted(k for k, t in h.items() if t.is_floating_point() and not bool(torch.isfinite(t).all()))
        assert not bad, f"{label}: non-finite defined outputs under H: {bad}"
    return res[0]
