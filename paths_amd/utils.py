"""Recursion driver (reference utils.py:228-305), device-resident.

``inference_end2end`` keeps the reference's signature and return values but replaces its per-level host round
trip (``importance.cpu()``, per-slide Python loop with ``torch.topk`` / child expansion / host gather /
``collate_fn``; reference utils.py:248-260, data_utils/slide.py:277-360, data_utils/dataset.py:206-243) by three
kernel launches per level (paths_topk, paths_expand_children, paths_gather_rows).  There is NO host
synchronisation inside the level loop: padded length per level is the static capacity
``4 * min(N_prev, keep)`` instead of the data-dependent per-batch max, padding is masked by ``num_ims``.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import contextlib
import math
import torch
import torch.nn.functional as F

from . import _lib, ops
from .data_utils.slide import DeviceSlide, DeviceSlideBatch, HostSlide, any_on_demand, mask_kernel, slide_batch

OVERLAP_AGGREGATOR = os.environ.get("PATHS_OVERLAP_AGGREGATOR", "1") != "0"
ROCTX_RANGES = os.environ.get("PATHS_ROCTX", "0") != "0"     # roctx ranges "level i: selection / aggregator / expansion" around the launches
                                                             # of each level (rocprofv3 --marker-trace; torch.cuda.nvtx = roctx on ROCm)
ROWS_IN_PLACE = os.environ.get("PATHS_ROWS_IN_PLACE", "1") != "0"
TRAIN_PARENT = os.environ.get("PATHS_TRAIN_PARENT", "1") != "0"      # training: h half of the LSTM gates once per kept parent
_STREAMS: Dict[int, tuple] = {}


def nll_loss(hazards, y, c, alpha=0.4, eps=1e-7):
    """Discrete-time survival NLL (MCAT) — reference utils.py:283-305.  [B,4] tensors: host-side plumbing."""
    B = hazards.shape[0]
    surv = torch.cumprod(1 - hazards, dim=1)
    surv_pad = torch.cat([torch.ones((B, 1), dtype=surv.dtype, device=surv.device), surv], dim=1)
    r = torch.arange(B, device=hazards.device)
    uncensored = -(1 - c) * (torch.log(surv_pad[r, y].clamp(min=eps)) + torch.log(hazards[r, y].clamp(min=eps)))
    censored = -c * torch.log(surv_pad[r, y + 1].clamp(min=eps))
    return ((1 - alpha) * (censored + uncensored) + alpha * uncensored).mean()


class RecursionError_(RuntimeError):
    pass


def recurse(model, slides, keep_patches: Sequence[int], num_levels: int,
            trace: Optional[list] = None, check_status: bool = True, attention: bool = False,
            rollout: bool = False) -> Dict[str, torch.Tensor]:
    """Optimistic sync-free pass; if some slide produced zero children (status bit 0, checked once at the end) the
    batch is re-run level by level with the reference's rare fallback (data_utils/slide.py:336-352) handled on the
    device.  See :func:`_recurse` for the arguments.

    ``attention`` (needs ``trace``): every trace record also gets "attention" [B, L, H, N] and "attention_self" [B, L, H], the
    special token's attention over the level's patches (in the order of its locs / importance, 0 on padding) and on itself, per
    decoder layer and head.  ``rollout`` (needs ``trace``, independent of ``attention``): every trace record also gets "rollout" [B, N]
    and "rollout_self" [B], the special token's attention rollout over the decoder stack (same order, 0 on padding)."""
    if attention and trace is None:
        raise ValueError("recurse(attention=True) returns the attention in the trace records: pass trace=[]")
    if rollout and trace is None:
        raise ValueError("recurse(rollout=True) returns the rollout in the trace records: pass trace=[]")
    out = _recurse(model, slides, keep_patches, num_levels, trace, careful=False, attention=attention, rollout=rollout)
    if not check_status:
        return out
    if check_status_word(out["status"]):        # the only host sync of the fast path, after the last level
        if trace is not None:
            trace.clear()
        out = _recurse(model, slides, keep_patches, num_levels, trace, careful=True, attention=attention, rollout=rollout)
        check_status_word(out["status"], fallback_done=True)
    return out


def check_status_word(status, fallback_done: bool = False) -> bool:
    """Decode the device status word of one recursion (ONE host sync).  Returns True when the batch needs the careful re-run (bit 0:
    some slide produced zero children, reference data_utils/slide.py:336-352); raises on the bits that invalidate the results - bit 1
    (child capacity exceeded) and bit 2 (a bounded in-launch hand-off wait of the token-0 tail gave up, csrc/token0_ws.hip).  Every
    path that returns recursion outputs goes through here: recurse(), GraphedRecursion.run(), TapedRecursion.run() and the
    training forward (autograd.forward_backward)."""
    code = int(status.item()) if torch.is_tensor(status) else int(status)
    if code & 2:
        raise RecursionError_("child capacity exceeded (internal error)")
    if code & 4:
        raise RecursionError_("a bounded in-launch hand-off wait of the token-0 tail gave up (csrc/token0_ws.hip): results invalid")
    return bool(code & 1) and not fallback_done


def _param_versions(model):
    """What a captured graph / recorded tape of ``model`` was built from: it is stale once any parameter's version counter has moved."""
    return tuple((p.data_ptr(), p._version) for p in model.parameters())


def _checked(rec, out) -> Dict[str, torch.Tensor]:
    """The status check of :func:`recurse` behind a replay of ``rec`` (a Graphed / TapedRecursion): one host sync after the last level;
    a batch with a slide without tissue children is handed to ``recurse()`` (eager, careful path)."""
    if check_status_word(out["status"]):
        with torch.no_grad():
            return recurse(rec.model, rec.batch, rec.keep, rec.levels)
    return out


def _stored_batch(slides, what: str) -> DeviceSlideBatch:
    """The batch of an entry point that needs every level's rows BEFORE its first launch (recorded or captured launch sequences,
    training): resident or host-resident slides.  On-demand slides raise - their rows come from a host callback between the levels."""
    if any_on_demand(slides):
        raise NotImplementedError(f"{what}: on-demand slides (OnDemandSlide) are served by recurse() / inference_end2end() only - "
                                  "their rows are supplied by a host callback between the levels")
    return slides if isinstance(slides, DeviceSlideBatch) else DeviceSlideBatch(slides)


class GraphedRecursion:
    """One batch's whole recursion (all levels, all three streams) captured ONCE into a HIP graph and replayed per step.

    The optimistic pass is sync-free with static capacities, static slide tables and cached weight images, so a step is a fixed
    launch sequence: capturing it takes Python (14 launches per level, ~1.6 ms of host time per 8-slide step) off the critical
    path - the replay is one hipGraphLaunch (host share of a step 0.65 -> 0.13, bit-identical outputs).  Measured on ROCm 7.2 /
    MI355X the replay runs the three captured streams with much less overlap than eager launches do (3.92 ms against 2.43 ms
    per 8-slide step at K = 2048), so this is an OPTION for host-bound deployments (many ranks per host core), not the default.  The graph owns its buffers (torch's graph-private pool); ``replay()`` returns the same output
    tensors every time (logits, ctx_slide, ctx_patch, importance, status), valid until the next replay.

    Validity: the capture bakes in the weight images that were current at capture time; ``replay()`` re-captures when any
    parameter's version counter has moved (optimizer step, load_state_dict).  The status word (bit 0: a slide without tissue
    children) is NOT handled inside the graph: callers check it like :func:`recurse` does and fall back to ``recurse()`` (eager,
    careful path) for such a batch - :meth:`run` does that."""

    def __init__(self, model, slides, keep_patches: Sequence[int], num_levels: int):
        self.model, self.keep, self.levels = model, list(keep_patches), int(num_levels)
        self.batch = _stored_batch(slides, "GraphedRecursion")
        if self.batch.host_resident:
            raise NotImplementedError("GraphedRecursion: host-resident slides (HostSlide) are not captured into a HIP graph; use "
                                      "TapedRecursion / PipelinedRecursion or recurse()")
        self.graph, self.out, self.versions = None, None, None

    def capture(self):
        dev = self.batch.device
        with torch.no_grad():
            # warm-up outside the capture: builds every cached image / table (some of which sync) and the side streams
            _recurse(self.model, self.batch, self.keep, self.levels, None, careful=False)
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = _recurse(self.model, self.batch, self.keep, self.levels, None, careful=False)
        self.graph, self.out, self.versions = g, out, _param_versions(self.model)
        return self

    def replay(self) -> Dict[str, torch.Tensor]:
        if self.graph is None or self.versions != _param_versions(self.model):
            self.capture()
        self.graph.replay()
        return self.out

    def run(self) -> Dict[str, torch.Tensor]:
        """replay + the status check of :func:`recurse` (one host sync after the last level)."""
        return _checked(self, self.replay())


class TapedRecursion:
    """One batch's recursion recorded ONCE as a flat launch tape and replayed per step.

    The optimistic pass is sync-free with static capacities, resident slides and cached weight images: a step is a fixed sequence
    of ~70 kernel launches, a dozen cross-stream joins and two zero fills on three HIP streams.  The first call runs it eagerly
    while a ``_lib.LaunchTape`` records every C call with its final arguments (device pointers, sizes, the stream handle); a replay
    is then its tight loop over that list - no tensor allocation, no pack look-ups, no Python-side shape logic - on the SAME three
    streams with the same joins, so the overlap of the eager schedule is kept (a captured HIP graph loses most of it on ROCm 7.2,
    see GraphedRecursion) while the host's share of a step drops from ~0.65 to ~0.15.  Outputs live in the buffers of the recorded
    pass and are overwritten by every replay.

    Validity: the tape holds the weight images current at recording time; ``replay()`` records again when any parameter's version
    counter has moved.  Like the eager fast path it does not handle the zero-children fallback itself: :meth:`run` checks the
    status word and hands such a batch to ``recurse()``.  ``slide_ctx_mode="concat"`` stacks contexts with a torch op per level
    and is not taped (eager path).

    This class is a client of the tape: it keeps the memory pool, the private table copy, the parameter versions and ``tape``, the
    plain list of ``(fn, ctypes_args, name)`` that is replayed (None before recording; replaceable).  Recording, the events, the replay
    loop and their clean-up are the ``LaunchTape``'s.  ``lane`` picks the stream triple the pass is recorded on and replays on."""

    def __init__(self, model, slides, keep_patches: Sequence[int], num_levels: int, lane: int = 0):
        self.model, self.keep, self.levels, self.lane = model, list(keep_patches), int(num_levels), int(lane)
        self.batch = _stored_batch(slides, "TapedRecursion")
        self.tape, self.out, self.versions, self.stream_handle = None, None, None, None
        self._unjoined = False               # a replay(join=False) whose streams the caller stream has not waited for yet
        self._rec_batch = None               # private copy of the recorded batch's table TENSORS: what the tape addresses (rebind() re-points them)
        self._tape = _lib.LaunchTape()       # records the pass; owns the HIP events of its stream joins across re-recordings
        # The tape holds raw device addresses of every intermediate of the recorded pass.  Those tensors are freed when the pass
        # returns; from the default caching allocator their blocks would be handed to whoever allocates next, and a replay would
        # then write into memory somebody else owns.  So the recorded pass allocates from a pool of its own: freed blocks stay in
        # it (re-used only by this tape's next recording) for as long as the tape lives.
        self._pool = torch.cuda.MemPool()
        if model.procs[0].config.slide_ctx_mode == "concat":
            raise NotImplementedError("TapedRecursion: slide_ctx_mode='concat' is not taped; use recurse()")

    def close(self):
        """Drop the tape and destroy the HIP events of its stream joins (a service that records one tape per batch would otherwise
        accumulate about a dozen events per tape).  Called by __del__; the tape can be recorded again afterwards."""
        self.tape = None
        if hasattr(self, "_tape"):                               # (__init__ may have raised before _tape existed)
            self._tape.close(self.batch.device)

    def __del__(self):
        self.close()

    def record(self):
        with torch.no_grad():
            tab = self.batch.clone_tables()                  # the tape's OWN table tensors (rebind() re-points them)
            _recurse(self.model, tab, self.keep, self.levels, None, careful=False, lane=self.lane)      # warm-up: builds cached images / tables
            torch.cuda.synchronize(self.batch.device)
            self.out = None                                   # (a re-recording re-uses the pool's blocks: drop the old outputs first)
            with self._tape.record(), torch.cuda.use_mem_pool(self._pool, device=self.batch.device):
                out = _recurse(self.model, tab, self.keep, self.levels, None, careful=False, lane=self.lane)
            torch.cuda.synchronize(self.batch.device)
        self.tape, self.out, self.versions = self._tape.converted(), out, _param_versions(self.model)
        self.stream_handle = torch.cuda.current_stream(self.batch.device).cuda_stream
        self._rec_batch = tab
        return self

    def rebind(self, slides) -> "TapedRecursion":
        """Point the recorded tape at ANOTHER batch of slides of the same kind (resident, or host-resident: one recorded launch sequence
        then serves a whole cohort streamed from pinned host memory) without recording again (a stream of distinct slides would
        otherwise pay record() per batch or run eager).  The tape addresses the recorded batch's per-level TABLE tensors (grid / mask
        base pointers, grid dims: a private copy made by record()), never the slides themselves, and every capacity in it is static - so a batch
        with the same slide count, feature width and level count whose level-0 cell count, grid extents and operand range fit the
        recorded ones is bound by copying its tables into those tensors (a few hundred bytes per level, device to device, enqueued
        on the current stream: no host sync).  Anything else drops the tape; the next replay records for the new batch."""
        new = _stored_batch(slides, "TapedRecursion.rebind")
        rec = self._rec_batch
        if new.dtype != self.batch.dtype:           # (the launches differ by grid dtype: a tape never serves both)
            raise ValueError(f"rebind: the tape serves {self.batch.dtype} grids, the new batch holds {new.dtype} grids")
        if new.host_resident != self.batch.host_resident:      # (a host batch's tape stages its rows, a resident batch's does not)
            kind = lambda h: "host-resident" if h else "resident"
            raise ValueError(f"rebind: the tape serves {kind(self.batch.host_resident)} slides, the new batch is {kind(new.host_resident)}")
        if new.packed != self.batch.packed:         # (other entry points, one more table per level)
            form = lambda k: "packed" if k else "dense"
            raise ValueError(f"rebind: the tape serves {form(self.batch.packed)} slides, the new batch is {form(new.packed)}")
        fits = (self.tape is not None and rec is not None and len(new) == len(rec) and new.dim == rec.dim and new.device == rec.device
                and new.num_levels >= self.levels and new.n0 <= rec.n0
                and all(new.max_dim[l] <= rec.max_dim[l] for l in range(self.levels))
                and ops.h3_in_range(new.feat_absmax) == ops.h3_in_range(rec.feat_absmax)
                and new.masked == rec.masked)            # (masked views add a launch at level 0)
        if not fits:
            self.tape, self._rec_batch = None, None
            self.batch = new
            return self
        if self._unjoined:
            # the previous replay(join=False) may still be reading the tables on the lane's streams: the caller stream (which carries
            # the copy below) waits for them first - a write-after-read race otherwise
            self.join()
        with torch.no_grad():
            src, dst = new.flat_tables(), rec.flat_tables()
            if src.numel() == dst.numel():                 # same level count: ONE copy of all tables (a few hundred bytes)
                dst.copy_(src, non_blocking=True)
            else:
                for l in range(self.levels):
                    rec.grid_ptrs[l].copy_(new.grid_ptrs[l], non_blocking=True)
                    rec.mask_ptrs[l].copy_(new.mask_ptrs[l], non_blocking=True)
                    rec.gx[l].copy_(new.gx[l], non_blocking=True)
                    rec.gy[l].copy_(new.gy[l], non_blocking=True)
                    if new.packed:
                        rec.index_ptrs[l].copy_(new.index_ptrs[l], non_blocking=True)
        self.batch = new                 # (keeps the bound slides alive; run()'s fallback recurses on them)
        return self

    def replay(self, join: bool = True) -> Dict[str, torch.Tensor]:
        """join=False leaves out the tape's last entry (the caller stream waiting for this lane's streams): several lanes
        (sub-batches recorded on different stream triples) are then enqueued back to back and run CONCURRENTLY; call
        :meth:`join` on each afterwards."""
        if self.tape is None or self.versions != _param_versions(self.model):
            self.record()
        assert torch.cuda.current_stream(self.batch.device).cuda_stream == self.stream_handle, "replay on the stream the tape was recorded on"
        assert self.tape[-1][2] == "paths_stream_wait"
        self._tape.play(self.tape if join else self.tape[:-1])
        self._unjoined = not join
        return self.out

    def join(self):
        self._tape.play(self.tape[-1:])
        self._unjoined = False

    def run(self) -> Dict[str, torch.Tensor]:
        """replay + the status check of :func:`recurse` (one host sync after the last level)."""
        return _checked(self, self.replay())


class PipelinedRecursion:
    """Several resident batches served with TWO in flight: batch k is recorded as a :class:`TapedRecursion` on stream triple
    ``1 + k % 2`` and :meth:`submit` replays it WITHOUT the tape's final join, so the next batch's selection chain (other streams)
    starts while this batch's last aggregator still runs - the ~165-us gap a single stream triple leaves at every step boundary
    (profiles/r04_experiments.md, selection-queue timeline; bench.py ``host.launch_modes.replay_two_lanes``: +2.7 %).
    :meth:`result` joins batch k into the caller's stream and returns its outputs (valid until that batch is submitted again);
    the status word is checked there like in ``TapedRecursion.run``.  Same launches, same buffers, same results as one lane."""

    def __init__(self, model, batches, keep_patches: Sequence[int], num_levels: int, lanes: int = 2):
        self.tapes = [TapedRecursion(model, b, keep_patches, num_levels, lane=1 + k % max(1, int(lanes))).record() for k, b in enumerate(batches)]

    def submit(self, k: int):
        self.tapes[k].replay(join=False)

    def result(self, k: int, check: bool = True) -> Dict[str, torch.Tensor]:
        t = self.tapes[k]
        t.join()
        return _checked(t, t.out) if check else t.out

    def close(self):
        for t in self.tapes:
            t.close()
        self.tapes = []


class _Range:
    """roctx range around a group of launches (host side: marks where the launches were ENQUEUED); a no-op unless PATHS_ROCTX=1."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if ROCTX_RANGES:
            torch.cuda.nvtx.range_push(self.name)

    def __exit__(self, *exc):
        if ROCTX_RANGES:
            torch.cuda.nvtx.range_pop()
        return False


def _streams(dev, lane: int = 0):
    """(selection-chain stream, aggregator stream, parent-partials stream) of a device, one triple per ``lane``.  The selection chain is the critical path of the recursion,
    so it gets the high-priority queue: its workgroups are dispatched first and the aggregator fills what is left."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, lane)
    if key not in _STREAMS:
        hi = -1 if os.environ.get("PATHS_STREAM_PRIORITIES", "1") != "0" else 0
        agg = torch.cuda.Stream(device=idx, priority=0)
        ncu = int(os.environ.get("PATHS_AGG_CU_MASK", "0"))
        if ncu > 0:
            # measurement aid: the aggregator stream confined to `ncu` of the chip's compute units, spread evenly over the
            # mask's bit positions (which interleave the XCDs); the selection streams keep the whole chip
            import ctypes
            total = torch.cuda.get_device_properties(idx).multi_processor_count
            words = (total + 31) // 32
            mask = (ctypes.c_uint32 * words)()
            for j in range(ncu):
                bit = (j * total) // ncu
                mask[bit // 32] |= 1 << (bit % 32)
            with torch.cuda.device(idx):
                h = _lib.load().paths_stream_create_masked(mask, words)
            if not h:
                raise _lib.PathsHipError("paths_stream_create_masked failed: " + _lib.load().paths_last_error().decode())
            agg = torch.cuda.ExternalStream(h, device=idx)
        _STREAMS[key] = (torch.cuda.Stream(device=idx, priority=hi), agg, torch.cuda.Stream(device=idx, priority=hi))
    return _STREAMS[key]


def _recurse(model, slides, keep_patches: Sequence[int], num_levels: int,
             trace: Optional[list] = None, careful: bool = False, attention: bool = False, rollout: bool = False, lane: int = 0) -> Dict[str, torch.Tensor]:
    batch = slide_batch(slides)
    if batch.on_demand:
        # max|x| is only known as the rows arrive: every level whose rows raise it enters a range_guard of its own on this stack
        # (_note_range), all left when the pass ends
        with contextlib.ExitStack() as guards:
            batch.begin_pass()
            batch.guards = guards
            guards.callback(batch.end_pass)
            try:
                return _recurse_streams(model, batch, keep_patches, num_levels, trace, careful, attention, rollout, lane)
            except BaseException:
                # (a refused slide, a bad encode() result, inf / NaN rows: the pass's streams have not been joined - nothing of it
                # is in flight any more when its buffers are dropped and the error leaves)
                torch.cuda.synchronize(batch.device)
                raise
    with ops.range_guard(batch.feat_absmax):       # out-of-range features run on the exact bf16 split (no fp16 overflow)
        return _recurse_streams(model, batch, keep_patches, num_levels, trace, careful, attention, rollout, lane)


def _recurse_streams(model, batch, keep_patches, num_levels, trace, careful, attention=False, rollout=False, lane=0):
    if not (OVERLAP_AGGREGATOR and batch.device.type == "cuda"):
        return _recurse_body(model, batch, keep_patches, num_levels, trace, careful, None, None, attention, rollout)
    caller = torch.cuda.current_stream(batch.device)
    sel_stream, agg_stream, par_stream = _streams(batch.device, lane)
    if torch.cuda.is_current_stream_capturing():
        # HIP graph capture (GraphedRecursion): on ROCm 7.2 a stream that forks from an already-forked stream crashes
        # hipStreamEndCapture, so every side stream forks from the capture's origin stream: the selection chain runs on the origin
        # stream itself, the aggregator and expansion streams fork from / join into it (the body joins them at its end)
        _lib.stream_wait(agg_stream, caller)
        _lib.stream_wait(par_stream, caller)
        return _recurse_body(model, batch, keep_patches, num_levels, trace, careful, agg_stream, par_stream, attention, rollout)
    _lib.stream_wait(sel_stream, caller)
    _lib.stream_wait(agg_stream, caller)
    _lib.stream_wait(par_stream, caller)
    with torch.cuda.stream(sel_stream):
        out = _recurse_body(model, batch, keep_patches, num_levels, trace, careful, agg_stream, par_stream, attention, rollout)
    _lib.stream_wait(caller, sel_stream)     # (the body has already joined agg_stream into sel_stream)
    return out


def _child_capacity(n: int, keep: int):
    """The static capacities of the step from a level of ``n`` (padded) patches to its children: (cap_keep = the most parents the
    top-K keeps (``keep`` < 0: all), Nn = 4 * cap_keep = the children's padded length; padding is masked by ``num_ims``)."""
    cap_keep = n if keep < 0 else min(n, keep)
    return cap_keep, 4 * cap_keep


TOPK_LDS_MAX = 8192       # csrc/select.hip TOPK_MAX: the most keys paths_topk / paths_topk_rows hold in LDS


def topk_entry(N: int, rows: bool) -> str:
    """The top-K entry point for a level of ``N`` (padded) patches: the LDS-resident kernel up to 8,192, above that its tiled form
    (csrc/topk_tiled.hip; same arguments, same outputs), which refuses N above PATHS_TOPK_TILED_MAX = 65,535 itself.  ``rows``: the
    form that also writes the kept rows' addresses."""
    name = "paths_topk_rows" if rows else "paths_topk"
    return name if N <= TOPK_LDS_MAX else name + "_tiled"


def _level_sizes(n0: int, keep_patches, num_levels: int) -> List[int]:
    """Padded patch count of every level of the optimistic pass (the careful path may grow a level: _expand_children)."""
    sizes = [n0]
    for i in range(num_levels - 1):
        sizes.append(_child_capacity(sizes[-1], int(keep_patches[i]))[1])
    return sizes


def _child_buffers(B: int, cap: int, want_hp_row: bool, device):
    """The expansion's output buffers for ``cap`` children per slide: (num_out [B] i64, locs [B,cap,2] i64, parent [B,cap] i64,
    src_row [B,cap] i32, src_cell [B,cap] i32, hp_row [B,cap] i32 or None)."""
    i32, i64 = dict(device=device, dtype=torch.int32), dict(device=device, dtype=torch.int64)
    return (torch.empty((B,), **i64), torch.empty((B, cap, 2), **i64), torch.empty((B, cap), **i64),
            torch.empty((B, cap), **i32), torch.empty((B, cap), **i32), torch.empty((B, cap), **i32) if want_hp_row else None)


def _expand_children(batch, nxt: int, patch_size: int, keep_idx, keep_count, locs, N: int, Nn: int, status, stream: int, careful: bool,
                     want_child_pos: bool, want_hp_row: bool):
    """The children (level ``nxt``) of the kept patches: paths_expand_children into buffers of capacity ``Nn`` on ``stream``.  Returns
    (Nn, num_next [B], locs_next [B,Nn,2], parent_next [B,Nn], src_row [B,Nn], src_cell [B,Nn], child_pos [B, 4 cap_keep] or None,
    hp_row [B,Nn] (child -> kept slot) or None).

    ``careful``: one host sync; a slide whose kept patches have no tissue children falls back to all tissue cells of the next grid
    with zero parent state (reference data_utils/slide.py:336-352, paths_fallback_all_cells: src_row = -1, no gradient to any parent -
    child_pos of that slide is all -1), in buffers regrown to hold them (the returned Nn)."""
    B, cap_keep, p = len(batch), keep_idx.shape[1], _lib.ptr
    child_pos = torch.empty((B, 4 * cap_keep), device=batch.device, dtype=torch.int32) if want_child_pos else None
    if batch.on_demand:
        return (Nn, *_expand_on_demand(batch, nxt, patch_size, keep_idx, keep_count, locs, N, Nn, status, stream, child_pos, want_hp_row))
    gx, gy, masks = p(batch.gx[nxt]), p(batch.gy[nxt]), p(batch.mask_ptrs[nxt])

    def expand(cap):
        bufs = _child_buffers(B, cap, want_hp_row, batch.device)
        _lib.call("paths_expand_children", p(keep_idx), cap_keep, p(keep_count), p(locs), N, patch_size, gx, gy, masks, B, cap,
                  *(p(t) for t in bufs[:5]), p(status), p(child_pos), p(bufs[5]), stream)
        return bufs

    bufs = ops.timed("expand", lambda: expand(Nn))
    if careful:
        empty = (bufs[0] == 0).cpu()                      # per-level sync: slow path only
        if bool(empty.any()):
            need = Nn
            for b in torch.nonzero(empty).flatten().tolist():
                tissue = int(batch.slides[b].masks[nxt].sum().item())
                X, Y = batch.slides[b].shape(nxt)
                need = max(need, tissue if tissue > 0 else X * Y)
            if need > Nn:
                Nn = need
                bufs = expand(Nn)
            _lib.call("paths_fallback_all_cells", gx, gy, masks, patch_size, B, Nn, *(p(t) for t in bufs[:5]), p(status), p(bufs[5]), stream)
    return (Nn, *bufs[:5], child_pos, bufs[5])


def _mask_supplied(batch, buf, want_mask: bool, stream: int):
    """The resident slides' mask pass over rows an on-demand batch was just supplied with (``buf`` [B, cap, D], a grid of B * cap
    cells): max|x| accumulates into the batch's running maximum; returns the tissue mask [B, cap] (``want_mask``).  The same kernel
    as DeviceSlide's, so the tissue predicate sums in the same order."""
    B, cap, D = buf.shape
    mask = torch.empty((B, cap), device=batch.device, dtype=torch.uint8) if want_mask else None
    _lib.call(mask_kernel(batch.dtype), buf.data_ptr(), B * cap, D, _lib.ptr(mask), batch.absmax_bits.data_ptr(), stream)
    return mask


def _note_range(batch, amax_before: float):
    """On-demand batch, after a read-back: the range contract for the rows supplied so far.  A level whose rows raised max|x| enters
    its own ops.range_guard (out of the fp16-split range: the rest of the pass runs on the three-plane kernels; inf / NaN raises)."""
    if batch.feat_absmax > amax_before:
        batch.guards.enter_context(ops.range_guard(batch.feat_absmax))


def _expand_on_demand(batch, nxt: int, patch_size: int, keep_idx, keep_count, locs, N: int, Nn: int, status, stream: int, child_pos,
                      want_hp_row: bool):
    """_expand_children for on-demand slides: the expansion split around the caller's encoder.  candidates -> one host
    read of their counts -> ``encode`` per slide into one [B, 4 cap_keep, D] buffer -> mask + max|x| -> admit -> one host read of the
    admitted counts and max|x|.  Everything runs on ``stream``, which is torch's current stream: the first read waits for the candidate
    kernel, the encoder's writes precede the mask launch, and the rows stay alive in ``batch.supplied`` until the pass has joined its
    streams.  Returns _expand_children's tuple without its first entry."""
    assert stream == _lib.stream(), "the on-demand expansion synchronises with torch's current stream"
    B, cap_keep, p = len(batch), keep_idx.shape[1], _lib.ptr
    i32 = dict(device=batch.device, dtype=torch.int32)
    i64 = dict(device=batch.device, dtype=torch.int64)
    Nc = 4 * cap_keep
    cand_count, cand_cells, cand_slot = torch.empty((B,), **i32), torch.empty((B, Nc, 2), **i64), torch.empty((B, Nc), **i32)
    ops.timed("candidates", lambda: _lib.call("paths_candidate_children", p(keep_idx), cap_keep, p(keep_count), p(locs), N, patch_size,
                                              p(batch.gx[nxt]), p(batch.gy[nxt]), B, p(cand_count), p(cand_cells), p(cand_slot), stream))
    counts = cand_count.cpu().tolist()                    # the host read: waits for the current stream, i.e. for the candidate kernel
    buf = batch.supply(nxt, [cand_cells[b, :counts[b]] for b in range(B)], Nc)
    mask = _mask_supplied(batch, buf, True, stream)
    bufs = _child_buffers(B, Nn, want_hp_row, batch.device)
    ops.timed("admit", lambda: _lib.call("paths_admit_children", p(cand_count), p(cand_cells), p(cand_slot), p(mask), p(keep_idx), cap_keep,
                                         p(keep_count), patch_size, B, Nn, *(p(t) for t in bufs[:5]), p(status), p(child_pos), p(bufs[5]), stream))
    before = batch.feat_absmax
    num_out = batch.read_back(bufs[0])
    empty = [b for b in range(B) if num_out[b] == 0]
    if empty:
        names = ", ".join(repr(batch.slides[b].slide_id or f"#{b}") for b in empty)
        raise _lib.PathsHipError(
            f"on-demand slide {names}: none of the {[counts[b] for b in empty]} cells requested at level {nxt} is tissue.  The reference "
            "would continue with every cell of that level's grid (data_utils/slide.py:336-352), i.e. encode the whole grid - what "
            "on-demand slides exist to avoid; preprocess such a slide (DeviceSlide / HostSlide) or keep more patches")
    _note_range(batch, before)
    return (*bufs[:5], child_pos, bufs[5])


def _stage_rows(batch, rows, n: int, zero_row, stream: int):
    """Host-resident slides whose rows are read in place: pull the rows the address table ``rows`` [B,n] names over the host link into a
    compact HBM buffer and point the table at the copies.  Returns the buffer (alive for as long as a level reads through the table)."""
    buf = torch.empty((len(batch), n, batch.dim), device=batch.device, dtype=batch.dtype)
    p = _lib.ptr
    ops.timed("stage", lambda: _lib.call("paths_stage_rows", p(rows), len(batch) * n, batch.dim * buf.element_size(), p(buf), p(zero_row), stream))
    return buf


def _rows_in_place(r) -> bool:
    """Whether the current GEMM mode reads feature rows where they live (row-pointer operands) instead of gathered fp32 copies."""
    mc, D, Dp = r.mc, r.D, r.Dp
    return bool(r.share_parent and ops.use_x6(D, Dp - D) and ops.split_planes() == 2 and ROWS_IN_PLACE
                and (ops.fast_path(mc) or ops.generic_add_route(mc, D, Dp - D)))


def _level0(r) -> SimpleNamespace:
    """Level 0's rows: every cell of the base grids (paths_level0_batch)."""
    B, N, D, p = r.B, r.batch.n0, r.D, _lib.ptr
    lv = SimpleNamespace(N=N, state_prev=None, parent=None, staged=None)
    lv.fts = None if r.rows_in_place else torch.empty((B, N, D), **r.f32)
    lv.x_rows = torch.empty((B, N), **r.i64) if r.rows_in_place else None
    lv.locs = torch.empty((B, N, 2), **r.i64)
    lv.parent_inds = torch.empty((B, N), **r.i64)
    lv.num_ims = torch.empty((B,), **r.i64)
    _lib.call(r.batch.entry("paths_level0_batch"), p(r.batch.grid_ptrs[0]), p(r.batch.gx[0]), p(r.batch.gy[0]), B, D, r.mc.patch_size, N,
              p(lv.fts), p(lv.locs), p(lv.parent_inds), p(lv.num_ims), 0, p(lv.x_rows), p(r.zero_row), *r.batch.index_args(0), r.st)
    if r.batch.masked:        # views (DeviceSlide.with_masks): a cleared level-0 cell reads as a background cell's zero row
        _lib.call("paths_level0_mask_rows", p(r.batch.mask_ptrs[0]), p(r.batch.gx[0]), p(r.batch.gy[0]), B, D, N, p(lv.fts), p(lv.x_rows),
                  p(r.zero_row), r.st)
    if r.stage_host:
        lv.staged = _stage_rows(r.batch, lv.x_rows, N, r.zero_row, r.st)
    return lv


def _aggregate(r, lvl_pack, sel, ctx_hist, N: int):
    """The aggregator launches of one level (attention, token chain, classifier) on the current stream, with the optional attention /
    rollout exports."""
    mc, B, f32 = r.mc, r.B, r.f32
    ctx_prev = ctx_hist[-1] if (ctx_hist and mc.slide_ctx_mode == "residual") else None
    ctx_all = torch.stack(ctx_hist, dim=1) if (ctx_hist and mc.slide_ctx_mode == "concat") else None
    att = None
    if r.attention:                                 # (allocated on the aggregator's stream, like its logits)
        Hh, Lt = mc.trans_heads, mc.trans_layers
        att = (torch.empty((B, Lt, Hh, N), **f32), torch.empty((B, Lt, Hh), **f32))
    ro = (torch.empty((B, N), **f32), torch.empty((B,), **f32)) if r.rollout else None
    agg = ops.aggregator_forward(mc, lvl_pack, sel["tokens"], sel["num_ims"], ctx_prev, ctx_all, status=r.status, qkv=sel, attention=att,
                                 rollout=ro)
    if att is not None:
        agg = dict(agg, attention=att[0], attention_self=att[1])
    if ro is not None:
        agg = dict(agg, rollout=ro[0], rollout_self=ro[1])
    return agg


def _child_step(r, i: int, lv, out, keep: int):
    """From level ``i`` (``lv``, outputs ``out``) to level i + 1: top-K, the kept parents' h-partials, child expansion, row gathers.
    Returns (the next level's rows, keep_idx, keep_count)."""
    B, D, Dp, N, p, st = r.B, r.D, r.Dp, lv.N, _lib.ptr, r.st
    batch, share_parent, rows_in_place = r.batch, r.share_parent, r.rows_in_place
    cap_keep, Nn = _child_capacity(N, keep)
    # After the top-K the chain forks: the kept parents' h-partials (gather + GEMM, the longer branch) stay on this stream,
    # the child expansion and the row gathers (tiny latency-bound kernels) run beside them on a third stream and are joined
    # before the next level's gate GEMMs.  (The fork travels as the top-K kernel's stop event: _lib.fork_behind.)
    forked = r.overlap and share_parent
    keep_idx = torch.empty((B, cap_keep), **r.i32)
    keep_count = torch.empty((B,), **r.i32)
    kept_rows = None
    with (_lib.fork_behind([r.par_stream], r.main_stream) if forked else contextlib.nullcontext()):
        if rows_in_place:
            # ... with the addresses of the kept parents' h rows (row b, i -> ctx_patch[b, keep_idx[b, i], :D]) for the parent GEMM
            kept_rows = torch.empty((B, cap_keep), **r.i64)
            ops.timed("topk", lambda: _lib.call(topk_entry(N, True), p(out["importance"]), N, p(lv.num_ims), B, N, keep, p(keep_idx), cap_keep,
                                                p(keep_count), p(out["ctx_patch"]), Dp, N, p(kept_rows), p(r.zero_row), st))
        else:
            _lib.call(topk_entry(N, False), p(out["importance"]), N, p(lv.num_ims), B, N, keep, p(keep_idx), cap_keep, p(keep_count), st)
    hp = ops.parent_partials(r.lstm_pack, out["ctx_patch"], keep_idx, keep_count, kept_rows) if share_parent else None
    st2 = r.par_stream.cuda_stream if forked else st
    nx = SimpleNamespace(fts=None, x_rows=None, staged=None, state_prev=None, parent=None)
    with (torch.cuda.stream(r.par_stream) if forked else contextlib.nullcontext()):
        Nn, num_next, locs_next, parent_next, src_row, src_cell, _, hp_row = _expand_children(
            batch, i + 1, r.mc.patch_size, keep_idx, keep_count, lv.locs, N, Nn, r.status, st2, r.careful, False, share_parent)
        nx.N, nx.num_ims, nx.locs, nx.parent_inds = Nn, num_next, locs_next, parent_next
        if batch.on_demand:          # the rows just supplied may have moved the pass to the three-plane kernels (_note_range)
            rows_in_place = r.rows_in_place = _rows_in_place(r)
        gather, grid, pk = batch.entry("paths_gather_rows"), p(batch.grid_ptrs[i + 1]), batch.index_args(i + 1)
        if share_parent:
            # children only need their parent's c row (h enters through the per-parent partials)
            Hc = Dp - D
            c0 = torch.empty((B, Nn, Hc), **r.f32)
            if rows_in_place:
                # ... and their feature rows are not copied either: the GEMMs of the next level read them in the resident grids
                nx.x_rows = torch.empty((B, Nn), **r.i64)
                ops.timed("gather", lambda: _lib.call(
                    gather, grid, p(src_cell), D, out["ctx_patch"].data_ptr() + 4 * D, N, Dp,
                    p(src_row), Hc, p(num_next), B, Nn, None, p(c0), 0, p(nx.x_rows), p(r.zero_row), *pk, st2))
                if r.stage_host:
                    nx.staged = _stage_rows(batch, nx.x_rows, Nn, r.zero_row, st2)
            else:
                nx.fts = torch.empty((B, Nn, D), **r.f32)
                _lib.call(gather, grid, p(src_cell), D, out["ctx_patch"].data_ptr() + 4 * D, N, Dp,
                          p(src_row), Hc, p(num_next), B, Nn, p(nx.fts), p(c0), 0, None, None, *pk, st2)
            nx.parent = {"hp": hp, "hp_row": hp_row, "c0": c0}
        else:
            nx.fts = torch.empty((B, Nn, D), **r.f32)
            nx.state_prev = torch.empty((B, Nn, Dp), **r.f32)
            _lib.call(gather, grid, p(src_cell), D, p(out["ctx_patch"]), N, Dp, p(src_row), Dp,
                      p(num_next), B, Nn, p(nx.fts), p(nx.state_prev), 0, None, None, *pk, st2)
        if forked:            # allocated on the expansion stream, read by the next level on the selection stream
            r.keepalive.append((nx, src_row, src_cell))
    return nx, keep_idx, keep_count


def _recurse_body(model, batch, keep_patches: Sequence[int], num_levels: int, trace: Optional[list], careful: bool, agg_stream,
                  par_stream, attention: bool = False, rollout: bool = False) -> Dict[str, torch.Tensor]:
    """Run all levels for a DeviceSlideBatch of HBM-resident slides or of host-resident ones (HostSlide: the rows a level selected are
    staged into HBM over the host link right after their addresses are known, paths_stage_rows).  ``agg_stream`` / ``par_stream``:
    both None = everything on the current stream; else the aggregator and the child expansion overlap the selection chain on them.
    Returns the last level's output dict (+ "status").

    ``trace`` (a list) receives one dict per level with device tensors num_ims / locs / parent_inds / importance /
    logits / ctx_slide / keep_idx / keep_count, for parity tests and heat-map export; with ``attention`` also attention /
    attention_self (the special token's attention per decoder layer and head: ops.aggregator_forward); with ``rollout`` also
    rollout / rollout_self (its attention rollout).
    """
    mc = model.procs[0].config
    ops.check_supported(mc)
    assert batch.num_levels >= num_levels
    B, dev, D = len(batch), batch.device, batch.dim
    Dp = model.procs[0].ctx_dim()[1]
    f32 = dict(device=dev, dtype=torch.float32)
    # fp16 grids: the selection-chain kernels and the row-addressed GEMMs take their _h16 forms; every gathered copy is fp32
    h16 = batch.dtype == torch.float16
    lstm_pack = ops.pack_lstm(model.lstm) if model.use_lstm else None
    share_parent = model.use_lstm          # siblings share the parent's h: h-half of the gate GEMM once per kept parent
    # The aggregator of level i (attention, token chain, classifier) feeds nothing of level i+1 except the slide context, so
    # it runs on a second HIP stream beside the selection chain of level i+1 (top-K, expansion, gathers, gate GEMMs).  Several
    # of those kernels cannot fill 256 CUs alone (116-232 workgroups, one per CU); the other chain's waves take the idle CUs.
    overlap = agg_stream is not None
    main_stream = torch.cuda.current_stream(dev) if overlap else None
    keepalive = []                         # tensors read on a stream other than the one that allocated them: kept until the streams join
    # Host-resident slides: the grid addresses are pinned host memory.  Where rows are copied (fts) the copying kernel reads them over
    # the host link once and nothing else does; where they are read in place, the address table is staged: the selected rows are
    # pulled into a compact HBM buffer on the stream that wrote the table and the table is pointed at the copies.
    # packed slides: the two address-forming kernels take their _packed forms (+ the cell-index table); nothing else changes
    r = SimpleNamespace(mc=mc, batch=batch, B=B, D=D, Dp=Dp, st=_lib.stream(), f32=f32,
                        i32=dict(device=dev, dtype=torch.int32), i64=dict(device=dev, dtype=torch.int64),
                        lstm_pack=lstm_pack, share_parent=share_parent,
                        careful=careful, attention=attention, rollout=rollout, overlap=overlap, main_stream=main_stream,
                        par_stream=par_stream, keepalive=keepalive, status=None)
    if batch.on_demand:
        # level 0 asks every slide for all of its level-0 cells (the reference keeps every level-0 cell, data_utils/slide.py:257-269);
        # their max|x| is read before the first GEMM mode is chosen
        _mask_supplied(batch, batch.supply(0, batch.cells0, batch.n0), False, r.st)
        batch.read_back(None)
        _note_range(batch, 0.0)
    # default split mode: feature rows are read in place in the resident grids (row-pointer GEMM operands) instead of being
    # copied (level 0) or gathered (children)
    r.rows_in_place = rows_in_place = _rows_in_place(r)
    r.zero_row = torch.zeros((D,), **f32) if rows_in_place else None
    r.stage_host = batch.host_resident and rows_in_place
    lv = _level0(r)
    # importance of padded rows is 0 (reference utils.py:106-115): ONE zero fill for all levels (sizes are known up front
    # unless the careful path has to grow a level)
    sizes = _level_sizes(lv.N, keep_patches, num_levels)
    # (the status word rides on the same zero fill as the importance rows: one fill launch per step instead of two at its head)
    zbuf = _lib.zeros((B * sum(sizes) + 64,), **f32)
    imp_all = zbuf[:B * sum(sizes)]
    r.status = status = zbuf[B * sum(sizes) + 32:B * sum(sizes) + 33].view(torch.int32)
    imp_off = [B * sum(sizes[:i]) for i in range(num_levels)]
    out, ctx_hist, fork_pending = None, [], False
    for i in range(num_levels):
        lvl_pack = ops.pack_level(model.procs[i])
        if fork_pending:
            _lib.stream_wait(main_stream, par_stream)     # this level's rows / bookkeeping from the expansion branch are ready
        N = lv.N
        imp_buf = imp_all[imp_off[i]:imp_off[i] + B * N].view(B, N) if N == sizes[i] else None
        # (the aggregator's fork travels as the stop event of the chain's last kernel where that kernel can carry one: _lib.fork_behind)
        last = i == num_levels - 1
        with _Range(f"level {i}: selection chain (LSTM gates, importance, projection)"), \
                (_lib.fork_behind([agg_stream], main_stream) if overlap else contextlib.nullcontext()):
            sel = ops.selection_forward(mc, lstm_pack, lvl_pack, lv.fts, lv.locs, lv.num_ims, lv.state_prev, True, parent=lv.parent,
                                        max_pos=batch.max_dim[i], x_rows=lv.x_rows, feat_dim=D, importance_out=imp_buf,
                                        last_level=last, x_rows_h16=h16 and r.rows_in_place)
        if overlap:                                       # (agg_stream already waits for this level's tokens / num_ims: fork_behind above)
            keepalive.append((sel["tokens"], sel["num_ims"], sel.get("qkv_img"), sel.get("_qkv_ws")))
        with (torch.cuda.stream(agg_stream) if overlap else contextlib.nullcontext()), \
                _Range(f"level {i}: aggregator (second stream)" if overlap else f"level {i}: aggregator"):
            agg = _aggregate(r, lvl_pack, sel, ctx_hist, N)
        out = {"logits": agg["logits"], "ctx_slide": agg["ctx_slide"], "ctx_patch": sel["ctx_patch"], "importance": sel["importance"]}
        ctx_hist.append(out["ctx_slide"])
        rec = None
        if trace is not None:
            rec = {"num_ims": lv.num_ims, "locs": lv.locs, "parent_inds": lv.parent_inds, "importance": out["importance"],
                   "logits": out["logits"], "ctx_slide": out["ctx_slide"]}
            if attention:
                rec["attention"], rec["attention_self"] = agg["attention"], agg["attention_self"]
            if rollout:
                rec["rollout"], rec["rollout_self"] = agg["rollout"], agg["rollout_self"]
            trace.append(rec)
        if last:
            break
        lv, keep_idx, keep_count = _child_step(r, i, lv, out, int(keep_patches[i]))
        fork_pending = overlap and share_parent
        if rec is not None:
            rec["keep_idx"], rec["keep_count"] = keep_idx, keep_count
    if overlap:
        _lib.stream_wait(main_stream, agg_stream)
        _lib.stream_wait(main_stream, par_stream)
        keepalive.clear()
    out = dict(out)
    out["status"] = status
    return out


def recurse_train(model, slides, keep_patches: Sequence[int], num_levels: int, careful: bool = False,
                  trace: Optional[list] = None, path: Optional[Sequence] = None, points=None) -> Dict[str, torch.Tensor]:
    """Differentiable recursion for training: same kernels as :func:`recurse`, but every level goes through
    paths_amd.autograd.LevelFn / GatherFn so that ``loss.backward()`` runs the hand-written backward kernels.
    Padded rows are zero-filled and computed (no tile skipping) so that every saved activation is finite.

    Like :func:`recurse` the default pass is optimistic and sync-free; the returned ``status`` word has bit 0 set when some
    slide's kept patches had no tissue children.  The caller (:func:`forward_backward`) then repeats the step with
    ``careful=True``: one host sync per level and the reference's fallback to all tissue cells of the next grid with zero
    parent state (data_utils/slide.py:336-352), handled on the device (paths_fallback_all_cells).

    ``trace`` (a list) turns the pass into the one feature gradients are taken from (paths_amd/saliency.py:input_gradients): every
    level's feature rows become a detached leaf that requires a gradient, the parameters enter detached (no parameter gradient is
    computed or accumulated) and the list receives one dict per level in the format of :func:`recurse`'s trace - num_ims / locs /
    parent_inds / importance / logits, keep_idx / keep_count below the last level - plus ``fts``, the leaf [B,N,D].

    ``path`` freezes the selection: per level below the last, (keep_idx [B, cap_keep] int32, keep_count [B] int32) as a
    trace records them.  paths_topk is not launched; the recorded indices go to the child expansion, the gathers and the
    once-per-parent form, which read nothing but them, the locations and the precomputed masks - the pass visits the recorded
    patches whatever the feature values are.  ``points(level, fts, num_ims) -> fts'`` replaces a level's feature rows [B,N,D] (padded
    rows zero) before they enter the level (and before they become the leaf of the ``trace`` mode).  Both None: every launch and
    every result is what it is without them."""
    batch = _stored_batch(slides, "recurse_train")
    with ops.range_guard(batch.feat_absmax):
        return _recurse_train_body(model, batch, keep_patches, num_levels, careful, trace, path, points)


def _recurse_train_body(model, batch, keep_patches, num_levels, careful, trace=None, path=None, points=None):
    from . import autograd as pag
    mc = model.procs[0].config
    ops.check_supported(mc, training=True)
    B, dev, D = len(batch), batch.device, batch.dim
    st = _lib.stream()
    p = _lib.ptr
    i32 = dict(device=dev, dtype=torch.int32)
    i64 = dict(device=dev, dtype=torch.int64)
    f32 = dict(device=dev, dtype=torch.float32)
    status = torch.zeros(1, **i32)
    N = batch.n0
    fts = torch.empty((B, N, D), **f32)
    locs = torch.empty((B, N, 2), **i64)
    parent = torch.empty((B, N), **i64)
    num_ims = torch.empty((B,), **i64)
    h16 = batch.dtype == torch.float16                     # fp16 grids: the gathers write fp32 copies, the training kernels are unchanged
    _lib.call(batch.entry("paths_level0_batch"), p(batch.grid_ptrs[0]), p(batch.gx[0]), p(batch.gy[0]), B, D, mc.patch_size, N, p(fts),
              p(locs), p(parent), p(num_ims), 1, None, None, *batch.index_args(0), st)
    if batch.masked:
        _lib.call("paths_level0_mask_rows", p(batch.mask_ptrs[0]), p(batch.gx[0]), p(batch.gy[0]), B, D, N, p(fts), None, None, st)
    state_prev, ctx_prev, ctx_hist = None, None, []
    logits = None
    # Once-per-parent form (LSTM, optimistic pass): siblings share their parent's h, so the h half of the gate pre-activations is one
    # product over the kept parents and its gradients are products over a quarter of the rows (autograd.LevelFn ``parent`` /
    # GatherParentFn).  The careful re-run (rare: a slide whose kept patches have no tissue children) keeps the per-child form,
    # whose fallback rows carry no parent.  PATHS_TRAIN_PARENT=0 keeps the per-child form everywhere.
    parent_form = TRAIN_PARENT and model.use_lstm and not careful
    par = None
    for i in range(num_levels):
        if mc.slide_ctx_mode == "concat":          # the classifier reads every previous level's slide context (model/paths.py:134-137)
            ctx_prev = torch.stack(ctx_hist, dim=1) if ctx_hist else None
        if points is not None:
            new = points(i, fts, num_ims)
            assert new.shape == fts.shape and new.dtype == fts.dtype and new.is_contiguous(), "points: [B,N,D] fp32 rows like the level's"
            fts = new
        if trace is not None:                      # (the gathers mark their feature rows non-differentiable: a fresh leaf per level)
            fts = fts.detach().requires_grad_(True)
        logits, ctx_slide, state_out, importance = pag.level_apply(model.procs[i], model.lstm if model.use_lstm else None, fts, locs,
                                                                   num_ims, state_prev, ctx_prev, parent=par,
                                                                   detach_params=trace is not None)
        ctx_prev = ctx_slide
        ctx_hist.append(ctx_slide)
        rec = None
        if trace is not None:
            rec = {"num_ims": num_ims, "locs": locs, "parent_inds": parent, "importance": importance, "logits": logits.detach(),
                   "fts": fts}
            trace.append(rec)
        if i == num_levels - 1:
            break
        keep = int(keep_patches[i])
        cap_keep, Nn = _child_capacity(N, keep)
        if path is not None:                       # the frozen path: the recorded selection instead of this pass's top-K
            keep_idx, keep_count = path[i]
            if not (keep_idx.shape == (B, cap_keep) and keep_count.shape == (B,) and keep_idx.dtype == keep_count.dtype == torch.int32
                    and keep_idx.is_contiguous() and keep_idx.device == keep_count.device == dev):
                raise ValueError(f"path[{i}]: (keep_idx [{B}, {cap_keep}] int32, keep_count [{B}] int32) on {dev} expected, got "
                                 f"{tuple(keep_idx.shape)} {keep_idx.dtype} / {tuple(keep_count.shape)} {keep_count.dtype}")
        else:
            keep_idx = torch.empty((B, cap_keep), **i32)
            keep_count = torch.empty((B,), **i32)
            _lib.call(topk_entry(N, False), p(importance), N, p(num_ims), B, N, keep, p(keep_idx), cap_keep, p(keep_count), st)
        Nn, num_next, locs_next, parent_next, src_row, src_cell, child_pos, hp_row = _expand_children(
            batch, i + 1, mc.patch_size, keep_idx, keep_count, locs, N, Nn, status, st, careful, True, parent_form)
        if rec is not None:
            rec["keep_idx"], rec["keep_count"] = keep_idx, keep_count
        if parent_form:
            fts, c0, h_kept = pag.GatherParentFn.apply(state_out, batch.grid_ptrs[i + 1], src_cell, src_row, num_next, keep_idx, keep_count,
                                                       child_pos, D, Nn, h16, batch.index_table(i + 1))
            par = {"c0": c0, "h_kept": h_kept, "hp_row": hp_row, "child_pos": child_pos, "keep_count": keep_count, "cap": cap_keep}
            state_prev = None
        else:
            fts, state_prev = pag.GatherFn.apply(state_out, batch.grid_ptrs[i + 1], src_cell, src_row, num_next, keep_idx,
                                                 keep_count, child_pos, D, Nn, h16, batch.index_table(i + 1))
        locs, parent, num_ims, N = locs_next, parent_next, num_next, Nn
    return {"logits": logits, "status": status}


def _label_to(x, dev):
    """A label vector on the device without a blocking copy: a pageable-memory upload would hold the host until everything already
    enqueued on the stream (the whole forward) has run, and the backward could only be enqueued after that."""
    t = torch.as_tensor(x)
    if t.device == dev:
        return t
    if dev.type == "cuda" and not t.is_cuda:
        return t.pin_memory().to(dev, non_blocking=True)
    return t.to(dev)


def loss_from_logits(logits, batch, task: str, global_batch: Optional[int] = None):
    """Loss of reference utils.py:263-279 on the last level's logits.  With ``global_batch`` the mean is taken over the
    GLOBAL batch (sum of local terms / global_batch) so that data-parallel shards add up exactly."""
    dev = logits.device
    n = logits.shape[0]
    scale = 1.0 if global_batch is None else n / float(global_batch)
    if task == "survival":
        hazards = torch.sigmoid(logits)
        loss = nll_loss(hazards, _label_to(batch["survival_bin"], dev), _label_to(batch["censored"], dev))
        return hazards, loss * scale
    elif task == "subtype_classification":
        return logits, F.cross_entropy(logits, _label_to(batch["subtype"], dev)) * scale
    raise ValueError(task)


_STATUS_HOST: Dict[int, torch.Tensor] = {}


def forward_backward(model, batch, num_levels, keep_patches, task: str = "survival", global_batch: Optional[int] = None):
    """Forward recursion + loss + backward of one (local) batch, with the recursion's status word checked BEFORE any gradient
    leaves the rank (all-reduce / optimizer): the status is copied to pinned memory right after the forward and read once the
    backward has been enqueued (by then the forward has long finished, so the wait is free).  Bit 0 (a slide without tissue
    children) repeats forward + backward on the careful path (reference fallback, data_utils/slide.py:336-352); bit 2
    (capacity) raises.  Gradients must be clear (set to None) on entry.  Returns (outputs, loss)."""
    from . import autograd as pag
    out = recurse_train(model, batch["slide"], keep_patches, num_levels)
    dev = out["status"].device
    host = _STATUS_HOST.get(dev.index)
    if host is None:
        host = _STATUS_HOST[dev.index] = torch.zeros((1,), dtype=torch.int32).pin_memory()
    host.copy_(out["status"], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    outputs, loss = loss_from_logits(out["logits"], batch, task, global_batch)
    loss.backward()
    ev.synchronize()
    if check_status_word(int(host[0])):
        model.zero_grad(set_to_none=True)
        out = recurse_train(model, batch["slide"], keep_patches, num_levels, careful=True)
        outputs, loss = loss_from_logits(out["logits"], batch, task, global_batch)
        loss.backward()
        check_status_word(out["status"], fallback_done=True)
    pag.fill_dead_grads(model)
    return outputs, loss


def train_step(model, optimizer, batch, num_levels, keep_patches, task: str = "survival", global_batch: Optional[int] = None,
               allreduce=None):
    """One optimisation step with the reference's semantics (train.py:59-68): forward recursion, mean loss,
    backward, [gradient all-reduce], optimizer step.  Dead parameters get the reference's zero gradients.
    ``batch`` None = this rank holds no slide of a short global batch: it contributes zeros for exactly the gradient set of
    an active rank.  Returns the (local share of the) loss as a tensor (None for an idle rank)."""
    from . import autograd as pag
    pag.clear_grads(model, optimizer)              # (optimizer.zero_grad for the live parameters; the dead ones keep their shared zero views)
    loss = None
    if batch is None:
        pag.zero_live_grads(model, num_levels)
    else:
        _, loss = forward_backward(model, batch, num_levels, keep_patches, task, global_batch)
        loss = loss.detach()
    if allreduce is not None:
        allreduce(model, num_levels=num_levels)
    optimizer.step()
    return loss


def inference_end2end(num_levels, keep_patches, model, base_power, batch, task: str):
    """reference utils.py:228-279.  ``batch["slide"]`` is a list of :class:`DeviceSlide` (or of :class:`HostSlide`, or of :class:`OnDemandSlide`); labels as in the reference
    (``survival_bin`` / ``censored`` or ``subtype``).  Returns (hazards or logits, loss)."""
    slides = slide_batch(batch["slide"])
    dev = slides.device
    out = recurse(model, slides, keep_patches, num_levels)
    logits = out["logits"]
    if task == "survival":
        labels = torch.as_tensor(batch["survival_bin"]).to(dev)
        censors = torch.as_tensor(batch["censored"]).to(dev)
        hazards = torch.sigmoid(logits)
        return hazards, nll_loss(hazards, labels, censors)
    elif task == "subtype_classification":
        subtypes = torch.as_tensor(batch["subtype"]).to(dev)
        return logits, F.cross_entropy(logits, subtypes)
    raise ValueError(task)
