"""ctypes binding of ``libpaths_hip.so`` (C ABI in include/paths_hip.h, which this module reads the signatures from).

The product path has NO fallback: if the shared library is missing or a kernel launch fails this
module raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``.

Launches go through :func:`call`.  A :class:`LaunchTape` records them for replay and owns all the state of that: its entries, its HIP
events, the open :class:`fork_behind` block and the recording thread.  The module keeps one name for it, ``TAPE``: the tape that is
recording, or None.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import re
import threading
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PATHS_HIP_LIB") or os.path.join(_HERE, "libpaths_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "paths_hip.h")


class PathsHipError(RuntimeError):
    pass


# The signatures are stated once, in include/paths_hip.h: the library's sources are compiled against it (csrc/common.h includes
# it, so a definition that disagrees does not build) and this binding reads every argtypes / restype from it.  A new entry point
# is defined in csrc/ and declared in the header; nothing is added here.
_PARAMS = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "paths_stream_t": C.c_void_p}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void *": C.c_void_p, "const char *": C.c_char_p}
_NAMED = re.compile(r"\b(paths_[a-z0-9_]+)\s*\(")
_DECLARATION = re.compile(r"([A-Za-z_][\w \t]*[\w*][ \t*]*)" + _NAMED.pattern + r"([^;{()]*)\)\s*;")


def parse_header(text: str) -> dict:
    """name -> (restype, [argtypes]) of every function a C header declares.  Parameters: int, int64_t, float, uint32_t, uint64_t,
    size_t, paths_stream_t and any pointer (c_void_p); returns: int, int64_t, void*, const char*.  Anything else raises, and so does a
    ``paths_name(`` in the text (comments apart) that is not part of a declaration this reads: no function stays silently unbound."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    out = {}
    for ret, name, params in _DECLARATION.findall(text):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise PathsHipError(f"declaration of {name}: return type '{ret}' is none of {sorted(_RETURNS)}")
        if name in out:
            raise PathsHipError(f"{name} is declared twice")
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            words = [w for w in p.replace("*", " * ").split() if w != "const"]
            if "*" in words:
                args.append(C.c_void_p)
            elif len(words) == 2 and words[0] in _PARAMS:             # type and name
                args.append(_PARAMS[words[0]])
            else:
                raise PathsHipError(f"declaration of {name}: parameter '{p.strip()}' is neither a pointer nor one of {sorted(_PARAMS)}")
        out[name] = (_RETURNS[ret], args)
    named = _NAMED.findall(text)
    if len(named) != len(out):
        raise PathsHipError(f"{len(named)} functions are named but {len(out)} declarations could be read: check "
                            f"{sorted(set(named) - set(out)) or 'for a name used twice'}")
    return out


def _read_header() -> dict:
    if not os.path.isfile(HEADER_PATH):
        raise PathsHipError(f"{HEADER_PATH} not found: the binding reads every signature from the C header of the source tree")
    with open(HEADER_PATH) as f:
        try:
            return parse_header(f.read())
        except PathsHipError as e:
            raise PathsHipError(f"{HEADER_PATH}: {e}") from None


DECLARATIONS = _read_header()                                              # name -> (restype, [argtypes]), read once
SIGNATURES = {name: args for name, (_, args) in DECLARATIONS.items()}      # name -> [argtypes]
ABI_VERSION = 3     # include/paths_hip.h: paths_abi_version() of the library this binding was written against
_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise PathsHipError(f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build()); "
                                "paths_amd has no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        lib.paths_abi_version.restype = C.c_int
        if lib.paths_abi_version() != ABI_VERSION:
            raise PathsHipError(f"{LIB_PATH} has ABI version {lib.paths_abi_version()}, this binding needs {ABI_VERSION}: rebuild it "
                                "(__graft_entry__.build())")
        for name, (res, args) in DECLARATIONS.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
        _lib = lib
    return _lib


def ptr(t):
    """Device address of a tensor; ``None`` and an ``int`` that already is an address pass through."""
    if t is None or type(t) is int:
        return t
    return t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def stream() -> int:
    """Handle of torch's current stream on the current device.  Called once per launch (~600 times per training step): the public
    ``torch.cuda.current_stream()`` builds a Stream object through four Python layers (5 ms per step measured under cProfile); the
    two C bindings below return the same handle directly."""
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream().cuda_stream


TAPE = None        # the LaunchTape that is recording (LaunchTape.record), else None: launches are only executed


class LaunchTape:
    """Everything one launch tape needs: the recorded entries ``(fn, args, name)``, the pool of HIP events its stream joins use (one per
    tape position, created once and re-used when the tape is recorded again - a weight changed - so re-recording leaks none), the
    :class:`fork_behind` block open on it and the thread that records.  While ``with tape.record():`` runs, ``TAPE`` is this object and
    every launch of the recording thread (:func:`call`, :func:`stream_wait`, :func:`zeros`) is executed AND appended; an entry from any
    other thread raises.  :meth:`converted` / :meth:`play` replay it, :meth:`close` destroys the events."""

    def __init__(self):
        self.entries, self.events, self.cursor, self.block, self.thread = None, [], 0, None, None

    @contextlib.contextmanager
    def record(self):
        """Record into fresh entries from the first event of the pool.  Refuses to start while another tape records or a stop event is
        pending; on every way out ``TAPE`` is None again, after an exception with nothing armed."""
        global TAPE
        if TAPE is not None:
            raise PathsHipError("a launch tape is already being recorded")
        lib = load()
        if lib.paths_stop_event_pending():
            raise PathsHipError("a stop event is pending: a launch tape cannot start recording behind it")
        self.entries, self.cursor, self.block, self.thread = [], 0, None, threading.get_ident()
        TAPE = self
        try:
            yield self
        except BaseException:
            lib.paths_clear_stop_event()
            raise
        finally:
            TAPE, self.block, self.thread = None, None, None

    def append(self, fn, args, name):
        if threading.get_ident() != self.thread:
            raise PathsHipError(f"{name} was launched from another thread while a launch tape records: it is not part of the tape")
        self.entries.append((fn, args, name))

    def next_event(self):
        """The event of the next tape position: taken from the pool, created when the pool has none left.  Only while recording."""
        if threading.get_ident() != self.thread:         # (None when not recording)
            raise PathsHipError("next_event: this launch tape is not recording on this thread")
        if self.cursor == len(self.events):
            ev = load().paths_event_create()
            if not ev:
                raise PathsHipError("paths_event_create failed")
            self.events.append(ev)
        self.cursor += 1
        return self.events[self.cursor - 1]

    def converted(self) -> list:
        """The entries with their arguments converted to their ctypes types, once: a replayed call then skips ctypes' per-argument
        conversion."""
        self.entries = [(fn, tuple(a if a is None else t(a) for t, a in zip(fn.argtypes, args)), name) for fn, args, name in self.entries]
        return self.entries

    @staticmethod
    def play(entries):
        """Replay ``entries`` in order.  The first one that fails ends it: the stop event is cleared (a failure between
        paths_set_stop_event and the kernel that takes it leaves nothing armed) and PathsHipError names the entry."""
        for fn, args, name in entries:
            if fn(*args) != 0:
                lib = load()
                msg = lib.paths_last_error().decode()
                lib.paths_clear_stop_event()
                raise PathsHipError(f"{name} failed during tape replay: {msg}")

    def close(self, device=None):
        """Drop the entries and destroy every event, once (a second call finds none); ``device`` is synchronised first, so that no replay
        in flight still waits on them.  Safe at interpreter shutdown, when the runtime may be gone already."""
        evs, self.events, self.cursor, self.entries = self.events, [], 0, None
        if evs:
            try:
                if device is not None:
                    torch.cuda.synchronize(device)
                lib = load()
                for ev in evs:
                    lib.paths_event_destroy(ev)
            except Exception:
                pass


def call(name: str, *args):
    lib = load()
    fn = getattr(lib, name)
    rc = fn(*args)
    if rc != 0:
        raise PathsHipError(f"{name} failed ({rc}): {lib.paths_last_error().decode()}")
    if TAPE is not None:
        TAPE.append(fn, args, name)
        fb = TAPE.block
        if fb is not None and fb.taken_at is None and name != "paths_set_stop_event" and not lib.paths_stop_event_pending():
            fb.taken_at = len(TAPE.entries) - 1          # this call's kernel carries the block's stop event


def stream_wait(dst: "torch.cuda.Stream", src: "torch.cuda.Stream"):
    """``dst.wait_stream(src)``; recorded on the launch tape (as a paths_stream_wait with its own event) when one is being built."""
    dst.wait_stream(src)
    if TAPE is not None:
        TAPE.append(load().paths_stream_wait, (dst.cuda_stream, src.cuda_stream, TAPE.next_event()), "paths_stream_wait")


STOP_EVENTS = os.environ.get("PATHS_STOP_EVENTS", "1") != "0"


# entries of a launch tape that are not kernel launches on the block's stream (fork_behind looks for the block's LAST launch)
_TAPE_PLUMBING = {"paths_set_stop_event", "paths_flush_stop_event", "paths_stream_wait_event", "paths_stream_wait", "paths_record_event",
                  "paths_clear_stop_event"}


class fork_behind:
    """``with fork_behind([dst...], src): <launches on src>`` - afterwards every ``dst`` waits for what ran on ``src``.  While a
    launch tape is recorded the join travels as a STOP EVENT of the block's stop-capable kernel (include/paths_hip.h:
    paths_set_stop_event; the finish kernel of the importance / projection GEMM, the top-K kernel) instead of an event record behind it;
    otherwise (eager launches, or PATHS_STOP_EVENTS=0) it is :func:`stream_wait` per destination.

    The stop event covers the block only if the kernel that took it is the block's LAST launch on ``src``.  That is checked, not
    assumed: the C call that owns the stop-capable kernel is the one during which ``paths_stop_event_pending()`` falls to 0
    (:func:`call` notes it); if any launch was recorded after it the event is recorded again behind the block the ordinary way
    (``paths_record_event``: waiters then wait for the later record), so a launch added behind the finish / top-K kernel cannot let
    ``dst`` start early on a replayed tape.

    The library arms ONE event per host thread, so a tape has one block open at a time (``LaunchTape.block``): entering a second one, or
    entering while an event is still pending, raises before anything is armed."""

    def __init__(self, dsts, src):
        self.dsts, self.src = list(dsts), src
        self.ev = None
        self.taken_at = None       # tape index of the call whose kernel took the event

    def __enter__(self):
        if TAPE is not None and STOP_EVENTS:
            if TAPE.block is not None:
                raise PathsHipError("fork_behind inside another fork_behind: the library arms one stop event at a time")
            if load().paths_stop_event_pending():
                raise PathsHipError("fork_behind: a stop event is already pending")
            self.ev = TAPE.next_event()
            call("paths_set_stop_event", self.ev)
            TAPE.block = self
        return self

    def __exit__(self, et, ev, tb):
        if self.ev is not None:
            TAPE.block = None
            if et is not None:
                load().paths_clear_stop_event()         # an exception inside the block: leave nothing armed for an unrelated launch
                return False
            call("paths_flush_stop_event", self.src.cuda_stream)
            if self.taken_at is not None and any(nm not in _TAPE_PLUMBING for _, _, nm in TAPE.entries[self.taken_at + 1:]):
                call("paths_record_event", self.ev, self.src.cuda_stream)     # launches followed the stop-capable kernel: cover them
            for d in self.dsts:
                call("paths_stream_wait_event", d.cuda_stream, self.ev)
        elif et is None:
            for d in self.dsts:
                stream_wait(d, self.src)
        return False


def zeros(shape, **kw) -> torch.Tensor:
    """``torch.zeros`` whose fill is repeated on every replay of a launch tape (status words, importance of padding rows)."""
    t = torch.zeros(shape, **kw)
    if TAPE is not None:
        TAPE.append(load().paths_memset_zero, (t.data_ptr(), t.numel() * t.element_size(), stream()), "paths_memset_zero")
    return t


def require_cuda(*tensors: torch.Tensor):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise PathsHipError("paths_amd runs on the GPU only: got a CPU tensor (no CPU fallback)")


def float_from_bits(bits: int) -> float:
    """fp32 value of a bit pattern written by paths_tissue_mask_absmax; any NaN pattern (above +inf) reads as inf."""
    import struct
    bits &= 0xFFFFFFFF
    return float("inf") if bits >= 0x7F800000 else struct.unpack("<f", struct.pack("<I", bits))[0]


def absmax(t: torch.Tensor) -> float:
    """max|x| of a contiguous fp32 device tensor (inf if not finite) through the same kernel; one host sync."""
    require_cuda(t)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() % 4 == 0
    bits = torch.zeros((1,), dtype=torch.int32, device=t.device)
    D = t.shape[-1] if (t.dim() > 1 and t.shape[-1] % 4 == 0) else 4
    call("paths_tissue_mask_absmax", t.data_ptr(), t.numel() // D, D, None, bits.data_ptr(), stream())
    return float_from_bits(int(bits.item()))
