"""ctypes binding of ``libpaths_hip.so`` (C ABI in include/paths_hip.h, which this module reads the signatures from).

The product path has NO fallback: if the shared library is missing or a kernel launch fails this
module raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
from __future__ import annotations

import ctypes as C
import os
import re
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


TAPE = None        # a list while paths_amd.utils.TapedRecursion records: every launch is executed AND appended as (fn, args, name)
TAPE_EVENTS = None # the recorder's event pool: [events, next index]; events are created once per tape position and re-used when a
                   # tape is recorded again (a weight changed), so re-recording does not leak HIP events


def call(name: str, *args):
    lib = load()
    fn = getattr(lib, name)
    rc = fn(*args)
    if rc != 0:
        raise PathsHipError(f"{name} failed ({rc}): {lib.paths_last_error().decode()}")
    if TAPE is not None:
        TAPE.append((fn, args, name))
        fb = fork_behind.active
        if fb is not None and fb.taken_at is None and name != "paths_set_stop_event" and not lib.paths_stop_event_pending():
            fb.taken_at = len(TAPE) - 1                  # this call's kernel carries the block's stop event


def _next_event():
    """The event of the next tape position: taken from the recorder's pool, created when the pool has none left."""
    pool = TAPE_EVENTS if TAPE_EVENTS is not None else [[], 0]
    if pool[1] == len(pool[0]):
        ev = load().paths_event_create()
        if not ev:
            raise PathsHipError("paths_event_create failed")
        pool[0].append(ev)
    pool[1] += 1
    return pool[0][pool[1] - 1]


def stream_wait(dst: "torch.cuda.Stream", src: "torch.cuda.Stream"):
    """``dst.wait_stream(src)``; recorded on the launch tape (as a paths_stream_wait with its own event) when one is being built."""
    dst.wait_stream(src)
    if TAPE is not None:
        TAPE.append((load().paths_stream_wait, (dst.cuda_stream, src.cuda_stream, _next_event()), "paths_stream_wait"))


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
    ``dst`` start early on a replayed tape."""

    active = None        # the block being recorded (call() reports to it)

    def __init__(self, dsts, src):
        self.dsts, self.src = list(dsts), src
        self.ev = None
        self.taken_at = None       # tape index of the call whose kernel took the event

    def __enter__(self):
        if TAPE is not None and STOP_EVENTS:
            self.ev = _next_event()
            call("paths_set_stop_event", self.ev)
            self.prev, fork_behind.active = fork_behind.active, self
        return self

    def __exit__(self, et, ev, tb):
        if self.ev is not None:
            fork_behind.active = self.prev
            if et is not None:
                load().paths_clear_stop_event()         # an exception inside the block: leave nothing armed for an unrelated launch
                return False
            call("paths_flush_stop_event", self.src.cuda_stream)
            if self.taken_at is not None and any(nm not in _TAPE_PLUMBING for _, _, nm in TAPE[self.taken_at + 1:]):
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
        TAPE.append((load().paths_memset_zero, (t.data_ptr(), t.numel() * t.element_size(), stream()), "paths_memset_zero"))
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
