"""HBM-resident preprocessed slides (the device-side analogue of reference
data_utils/slide.py:PreprocessedSlide, :225-271).

A slide is its per-level feature grids ``[X, Y, D]`` fp32 (reference grid format: an all-zero row is a
background cell, preprocess/preprocess.py:89,172-175) kept RESIDENT in HBM, plus a one-byte-per-cell tissue
mask computed once on upload (``sum(dim=1) != 0``, reference data_utils/slide.py:324).  The per-level host
gather + H2D copy of the reference disappears: child rows are gathered on the device straight from these grids.
At K=2048 one slide is 2.9 GB (level-4 grid alone 2.1 GB); 288 GB of HBM holds ~90 of them.

Grids may also be kept in fp16 (``dtype=torch.float16``, opt-in): half the HBM per slide (~180 K=2048 slides per MI355X).  The
device kernels read fp16 rows where they live and widen them exactly; the host conversion goes through :func:`to_float16`, which
refuses values an fp16 grid cannot hold.  bf16 is not supported.

:class:`HostSlide` is the sibling for cohorts that do not fit in HBM: its grids stay in PINNED host memory, only the tissue masks
live on the device, and the recursion fetches just the rows it selects over the host link (paths_stage_rows).

:meth:`DeviceSlide.with_masks` / :meth:`HostSlide.with_masks` give a MASKED VIEW of a stored slide: the same grids behind other tissue
masks - a slide with some of its tissue turned to background, at the cost of the masks alone (saliency.removal_curves).

:class:`OnDemandSlide` holds no grid at all: the recursion asks the caller's ``encode`` for the features of exactly the cells it is
about to visit (reference ``RawSlide.recurse``, data_utils/slide.py:173-198).  :class:`CachedOnDemandSlide` keeps what
the encoder has produced on the device across passes and hands the visited part over as a packed :class:`DeviceSlide`.

PACKED slides (``slide.pack()``, ``packed=True``, ``from_patches``) leave the background out: per level the kept rows
``rows[l]`` [n_l, D] behind a cell index ``index[l]`` (int32 [X, Y] on the device: the row of a cell, or -1).  Only rows that are all
+0.0 are dropped, and such a cell reads as the zero row it was, so every result is bit-identical to the dense twin's.

One storage model serves all of these (:class:`_Slide`): per level ONE ROW TABLE - the dense grid seen as [X*Y, D], or the kept rows -
plus an optional cell index, in fp32 or fp16, in HBM or in pinned host memory.
"""
from __future__ import annotations

import copy
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib, synthetic

GRID_DTYPES = (torch.float32, torch.float16)
FP16_MAX = 65504.0


def check_grid_dtype(dtype) -> torch.dtype:
    """The storage dtype of resident grids: torch.float32 (default) or torch.float16."""
    if dtype == torch.bfloat16:
        raise NotImplementedError("bfloat16 feature grids are not supported (torch.float32 or torch.float16)")
    if dtype not in GRID_DTYPES:
        raise ValueError(f"feature grids must be torch.float32 or torch.float16, got {dtype}")
    return dtype


def entry_name(name: str, h16: bool, packed: bool = False) -> str:
    """The C entry point of ``name`` for a storage form, ``name[_packed][_h16]``: the ``_h16`` forms read fp16 rows, the ``_packed``
    forms take one more table (the level's cell index, :func:`index_args`) in front of the stream."""
    return name + ("_packed" if packed else "") + ("_h16" if h16 else "")


def index_args(index_ptrs: Optional[torch.Tensor]) -> tuple:
    """What a ``_packed`` entry point takes in front of its stream: a level's cell-index table (None - dense slides: nothing)."""
    return () if index_ptrs is None else (_lib.ptr(index_ptrs),)


def mask_kernel(dtype) -> str:
    """The mask pass over rows of ``dtype``: per-row tissue flags + max|x| bits accumulated into a one-word buffer."""
    return entry_name("paths_tissue_mask_absmax", dtype == torch.float16)


def to_float16(grid, chunk_rows: int = 1 << 16) -> Tuple[torch.Tensor, float]:
    """Host grid [..., D] (numpy or CPU tensor, any float dtype; taken as fp32 first) -> (fp16 CPU tensor rounded to nearest even,
    max |fp16 - fp32| rounding error).  Raises ValueError when a value is not finite or |x| > 65504, or when a tissue row (nonzero
    fp32 values) rounds to all zeros - the cell would silently turn into background."""
    g = torch.as_tensor(grid, dtype=torch.float32)
    assert g.device.type == "cpu", "to_float16 converts host grids"
    D = g.shape[-1]
    flat = g.reshape(-1, D)
    out = torch.empty(flat.shape, dtype=torch.float16)
    err = 0.0
    for r0 in range(0, flat.shape[0], chunk_rows):
        x = flat[r0:r0 + chunk_rows]
        if not bool(torch.isfinite(x).all()):
            raise ValueError("to_float16: the grid holds inf or NaN")
        amax = float(x.abs().max()) if x.numel() else 0.0
        if amax > FP16_MAX:
            raise ValueError(f"to_float16: |x| = {amax:g} exceeds the fp16 range ({FP16_MAX:g})")
        h = x.to(torch.float16)
        lost = (x != 0).any(dim=1) & ~(h != 0).any(dim=1)
        if bool(lost.any()):
            row = r0 + int(torch.nonzero(lost)[0])
            raise ValueError(f"to_float16: tissue row {row} rounds to all zeros in fp16 (it would become background)")
        if x.numel():
            err = max(err, float((h.to(torch.float32) - x).abs().max()))
        out[r0:r0 + chunk_rows] = h
    return out.reshape(g.shape), err


def pack_host_grid(g: torch.Tensor, chunk_rows: int = 1 << 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host grid [X, Y, D] (CPU tensor, fp32 or fp16) -> (rows [n, D], index int32 [X, Y]): the packed form of one level.  A row is kept
    iff any of its BITS is set - only all-+0.0 rows are dropped (a -0.0 element is a set bit; a row whose elements cancel to a zero sum
    is kept) - and kept rows are ranked in row-major cell order.  The contract of the device kernels (csrc/pack_rows.hip)."""
    check_grid_dtype(g.dtype)
    assert g.device.type == "cpu" and g.dim() == 3, "pack_host_grid packs host grids [X, Y, D]"
    X, Y, D = g.shape
    flat = g.contiguous().view(X * Y, D)
    bits = flat.view(torch.int32 if g.dtype == torch.float32 else torch.int16)
    kept = torch.empty((X * Y,), dtype=torch.bool)
    for r0 in range(0, X * Y, chunk_rows):
        kept[r0:r0 + chunk_rows] = (bits[r0:r0 + chunk_rows] != 0).any(dim=1)
    rank = torch.cumsum(kept, dim=0, dtype=torch.int64) - 1
    index = torch.where(kept, rank, torch.full_like(rank, -1)).to(torch.int32).view(X, Y)
    return flat[kept].contiguous(), index


def unpack_grid(rows: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """(rows [n, D], index [X, Y]) on one device -> the dense grid [X, Y, D]: cells without a row are +0.0."""
    X, Y = index.shape
    g = torch.zeros((X * Y, rows.shape[1]), dtype=rows.dtype, device=rows.device)
    idx = index.reshape(-1).to(torch.int64)
    kept = idx >= 0
    if rows.shape[0] > 0:
        g[kept] = rows[idx[kept]]
    return g.view(X, Y, rows.shape[1])


def check_patches(coords: Sequence, features: Sequence, shapes: Sequence, dtype) -> List[torch.Tensor]:
    """The checks of ``from_patches`` (all on the host, before any kernel is launched): returns the per-level linear cells x * Y + y
    (int64 CPU tensors [n_l]).  ValueError on a dtype that :func:`check_grid_dtype` refuses, on lists of different lengths, on coordinates
    that are not int64 [n_l, 2], lie outside the level's grid or name a cell twice, and on features that are not [n_l, D] with one D
    (a positive multiple of 4) for all levels."""
    try:
        check_grid_dtype(dtype)
    except NotImplementedError as e:
        raise ValueError(f"from_patches: {e}") from e
    if not (len(coords) == len(features) == len(shapes)) or len(shapes) < 1:
        raise ValueError(f"from_patches: one coords / features / shapes entry per level (got {len(coords)} / {len(features)} / {len(shapes)})")
    cells, D = [], None
    for l, (c, f, (X, Y)) in enumerate(zip(coords, features, shapes)):
        X, Y = int(X), int(Y)
        if X < 1 or Y < 1:
            raise ValueError(f"from_patches: level {l} has the grid shape {(X, Y)}")
        if not torch.is_tensor(c) or c.dtype != torch.int64 or c.dim() != 2 or c.shape[1] != 2:
            raise ValueError(f"from_patches: coords[{l}] is an int64 [n, 2] tensor of cell coordinates")
        if not torch.is_tensor(f) or f.dim() != 2 or not f.dtype.is_floating_point:
            raise ValueError(f"from_patches: features[{l}] is a floating-point [n, D] tensor")
        if f.shape[0] != c.shape[0]:
            raise ValueError(f"from_patches: level {l} has {c.shape[0]} coordinates for {f.shape[0]} feature rows")
        D = int(f.shape[1]) if D is None else D
        if int(f.shape[1]) != D or D < 4 or D % 4 != 0:
            raise ValueError(f"from_patches: the feature width is one positive multiple of 4 for all levels (level {l}: {int(f.shape[1])})")
        c = c.cpu()
        if c.numel() and (int(c.min()) < 0 or int(c[:, 0].max()) >= X or int(c[:, 1].max()) >= Y):
            raise ValueError(f"from_patches: level {l} has a cell outside its {X} x {Y} grid")
        lin = c[:, 0] * Y + c[:, 1]
        if torch.unique(lin).numel() != lin.numel():
            raise ValueError(f"from_patches: level {l} names a cell twice")
        cells.append(lin)
    return cells


def _patch_rows(f: torch.Tensor, dtype) -> torch.Tensor:
    """Feature rows of ``from_patches`` in the slide's dtype (still where they are); fp16 goes through :func:`to_float16`."""
    if f.dtype == dtype:
        return f.contiguous()
    if dtype == torch.float16:
        return to_float16(f.cpu())[0]
    return f.to(torch.float32).contiguous()


def _patch_index(cells: torch.Tensor, shape) -> torch.Tensor:
    """int32 CPU index [X, Y] of rows given in the order of ``cells`` (linear, distinct)."""
    X, Y = int(shape[0]), int(shape[1])
    index = torch.full((X * Y,), -1, dtype=torch.int32)
    index[cells] = torch.arange(cells.numel(), dtype=torch.int32)
    return index.view(X, Y)


def _scatter_flags(flags: Optional[torch.Tensor], index: torch.Tensor) -> torch.Tensor:
    """Per-ROW flags [n] (None: no rows) -> the per-CELL uint8 mask [X, Y] through the cell index (cells without a row: 0)."""
    m = torch.zeros((index.numel(),), dtype=torch.uint8, device=index.device)
    if flags is not None:
        idx = index.reshape(-1).to(torch.int64)
        kept = idx >= 0
        m[kept] = flags[idx[kept]]
    return m.view(index.shape)


def _pack_device_grid(g: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device grid [X, Y, D] -> (rows [n, D], index int32 [X, Y]) with the pack kernels (paths_pack_flags / _index / _rows); one host
    read of the row count."""
    _lib.require_cuda(g)
    g = g.contiguous()
    X, Y, D = g.shape
    cells, dev = X * Y, g.device
    h16 = check_grid_dtype(g.dtype) == torch.float16
    flags = torch.empty((cells,), dtype=torch.uint8, device=dev)
    index = torch.empty((X, Y), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    partials = torch.empty((int(_lib.load().paths_pack_index_partials(cells)),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream()
        _lib.call(entry_name("paths_pack_flags", h16), g.data_ptr(), cells, D, flags.data_ptr(), st)
        _lib.call("paths_pack_index", flags.data_ptr(), cells, index.data_ptr(), count.data_ptr(), partials.data_ptr(), st)
        n = int(count.item())
        rows = torch.empty((n, D), dtype=g.dtype, device=dev)
        if n > 0:
            _lib.call(entry_name("paths_pack_rows", h16), g.data_ptr(), cells, D, index.data_ptr(), n, rows.data_ptr(), st)
    return rows, index


def _level_dtype(levels: Sequence[torch.Tensor], who: str) -> torch.dtype:
    """The one storage dtype of a slide's levels (before any I/O or device touch)."""
    assert len(levels) >= 1
    dtype = check_grid_dtype(levels[0].dtype)
    if any(t.dtype != dtype for t in levels):
        raise ValueError(f"{who}: all levels of a slide must have the same dtype")
    return dtype


def _nbytes(tensors) -> int:
    return sum(t.numel() * t.element_size() for t in tensors)


class _Slide:
    """The storage model behind :class:`DeviceSlide` and :class:`HostSlide`.  Per level a slide holds ONE ROW TABLE and an optional cell
    index: dense, the table is ``grids[l]`` seen as [X*Y, D] and there is no index (``rows`` / ``index`` are None); packed, the table is
    the kept rows ``rows[l]`` behind ``index[l]`` (``grids`` is None).  ``masks[l]`` are uint8 [X, Y] device tensors either way.  The
    two classes differ in where a table lives (:meth:`_put`), how a dense level is packed (:meth:`_pack_grid`), how a synthetic level
    is produced (:meth:`_synth_level`) and how a table's rows reach the mask kernel (:meth:`_row_chunks`); everything else is here."""

    host_resident = False           # the tables live in HBM (HostSlide: in pinned host memory)
    on_demand = False
    packed = False                  # (the dense form's values; every slide carries its own)
    rows = None
    index = None

    @classmethod
    def _new(cls, dtype, device, masks, grids=None, rows=None, index=None, absmax: Optional[float] = None, absmax_bits=None,
             patch_size: int = 256, slide_id: str = "", subtype=None, masked_view: bool = False, synthetic_spec=None, into=None):
        """THE private constructor: a slide of ``cls`` (``into``: the object a public ``__init__`` is filling) made of exactly what it is
        handed - ``grids``, or ``rows`` + ``index`` - with every attribute set; nothing is checked, placed or launched."""
        s = object.__new__(cls) if into is None else into
        s.dtype, s.device = dtype, device                       # device: where the masks (and a packed slide's index) live
        s.packed = grids is None
        s.grids, s.rows, s.index, s.masks = grids, rows, index, list(masks)
        s._absmax, s._absmax_bits = absmax, absmax_bits         # max|feature| over all levels / its fp32 bit pattern from the mask pass
        s.patch_size, s.slide_id, s.subtype = patch_size, slide_id, subtype
        s.masked_view = masked_view                             # (with_masks: the same tables behind other tissue masks)
        s.synthetic_spec = synthetic_spec                       # (synthetic(): the generator of the grids, else None)
        return s

    def _ident(self) -> dict:
        """What every conversion of a slide keeps."""
        return dict(patch_size=self.patch_size, slide_id=self.slide_id, subtype=self.subtype, masked_view=self.masked_view,
                    synthetic_spec=self.synthetic_spec)

    @classmethod
    def _build(cls, levels, device, dtype, packed: bool, masks=None, absmax=None, patch_size: int = 256, slide_id: str = "", subtype=None,
               masked_view: bool = False, synthetic_spec=None, into=None, **pass_kw):
        """The slide of ``levels``: an iterable of dense grids [X, Y, D] or - ``packed`` only - of (rows, index) pairs, all in ``dtype``
        and anywhere.  Every table is put where the class keeps it; ``packed``: a dense level is packed and dropped before the next one
        is asked for (peak memory is the packed slide plus one dense level), the index goes to the device.  Masks and max|x| come from
        the mask pass over the tables (``pass_kw``: the class's :meth:`_row_chunks` options) unless cached ``masks=`` + ``absmax=`` are
        given."""
        if (masks is None) != (absmax is None):
            raise ValueError(f"{cls.__name__}: cached masks= and absmax= come together")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.PathsHipError(f"paths_amd runs on the GPU only: {cls._NEEDS_GPU} (no CPU fallback)")
        grids, rows, index = (None, [], []) if packed else ([], None, None)
        for lv in levels:
            if device.index is None:        # (the device is first touched here: after the host-side conversion of the first level)
                device = torch.device("cuda", torch.cuda.current_device())
            if packed:
                r, ix = lv if isinstance(lv, tuple) else cls._pack_grid(lv, device)
                del lv
                rows.append(cls._put(r, device))
                index.append(ix.to(device))
            else:
                if lv.dim() != 3:
                    raise ValueError(f"{cls.__name__}: grids are tensors [X, Y, D]")
                grids.append(cls._put(lv, device))
        s = cls._new(dtype, device, masks or (), grids, rows, index, None if absmax is None else float(absmax), patch_size=patch_size,
                     slide_id=slide_id, subtype=subtype, masked_view=masked_view, synthetic_spec=synthetic_spec, into=into)
        if masks is None:
            s._mask_pass(**pass_kw)
        else:
            _lib.require_cuda(*s.masks)
            if len(s.masks) != s.num_levels or any(m.dtype != torch.uint8 or tuple(m.shape) != s.shape(l) or not m.is_contiguous()
                                                   for l, m in enumerate(s.masks)):
                raise ValueError(f"{cls.__name__}: masks are contiguous uint8 [X, Y] device tensors, one per grid")
        return s

    def _mask_pass(self, **kw):
        """THE mask pass: paths_tissue_mask_absmax[_h16] over every row table -> per-row flags + max|x| bits in a one-word buffer; the
        flags are the per-cell mask of a dense level and go to their cells through the index of a packed one."""
        dev = self.device
        tables = self.rows if self.packed else [g.view(-1, g.shape[2]) for g in self.grids]
        with torch.cuda.device(dev):
            bits = self._absmax_bits = torch.zeros((1,), dtype=torch.int32, device=dev)
            flags = [torch.empty((t.shape[0],), dtype=torch.uint8, device=dev) if t.shape[0] else None for t in tables]
            for l, r0, ptr, n in self._row_chunks(tables, **kw):
                _lib.call(mask_kernel(self.dtype), ptr, n, self.dim, flags[l].data_ptr() + r0, bits.data_ptr(), _lib.stream())
            self.masks = [_scatter_flags(f, self.index[l]) if self.packed else f.view(self.grids[l].shape[:2]) for l, f in enumerate(flags)]
            if self.host_resident:
                # the host must not re-use or free the bounce buffer's view of the last chunk early; the pass is once per slide
                torch.cuda.current_stream(dev).synchronize()

    def feature_absmax(self) -> float:
        """max|x| over every grid of the slide (inf if any element is inf or NaN): the operand-range check of the default
        fp16-split GEMM mode (paths_amd/ops.py:h3_in_range).  One host sync on first use, cached."""
        if self._absmax is None:
            self._absmax = _lib.float_from_bits(int(self._absmax_bits.item()))
        return self._absmax

    def with_masks(self, masks: Sequence[torch.Tensor]):
        """A masked view of this slide: the same ``grids`` (shared, not copied), dtype, ``patch_size`` and recorded max|x| behind the
        given per-level tissue masks - contiguous uint8 [X, Y] tensors on the device of the slide's own masks (ValueError otherwise).  A
        cell whose byte is 0 is background to the recursion: the child filter drops it, and at level 0 - where every cell is loaded,
        background included - it reads as the all-zero row a background cell is.  Nothing is launched and nothing is allocated; batches
        take views like any slide, several views of one slide in one batch included."""
        masks = list(masks)
        if len(masks) != self.num_levels:
            raise ValueError(f"with_masks: one mask per level ({self.num_levels}) expected, got {len(masks)}")
        for l, (m, own) in enumerate(zip(masks, self.masks)):
            if not torch.is_tensor(m) or m.dtype != torch.uint8 or tuple(m.shape) != tuple(self.shape(l)) or not m.is_contiguous():
                got = f"{m.dtype} {tuple(m.shape)}" if torch.is_tensor(m) else type(m).__name__
                raise ValueError(f"with_masks: level {l} needs a contiguous uint8 [X, Y] = {list(self.shape(l))} tensor, got {got}")
            if m.device != own.device:
                raise ValueError(f"with_masks: the mask of level {l} lives on {m.device}, the slide's masks on {own.device}")
        # (the recorded max|x| of the source - its cached value: no launch)
        return self._new(self.dtype, self.device, masks, self.grids, self.rows, self.index, self.feature_absmax(),
                         **dict(self._ident(), masked_view=True))

    @property
    def num_levels(self) -> int:
        return len(self.index if self.packed else self.grids)

    def shape(self, level: int) -> Tuple[int, int]:
        g = self.index[level] if self.packed else self.grids[level]
        return g.shape[0], g.shape[1]

    @property
    def dim(self) -> int:
        return self.rows[0].shape[1] if self.packed else self.grids[0].shape[2]

    def resident_bytes(self) -> int:
        """Device memory held by the slide: the masks, a packed slide's cell index and - DeviceSlide - the grids or the packed rows."""
        tables = [] if self.host_resident else (self.rows if self.packed else self.grids)
        return _nbytes(tables) + _nbytes(self.index or ()) + _nbytes(self.masks)

    def pack(self):
        """The packed twin (this slide is left as it is): per level the rows with any bit set, in row-major cell order, behind the cell
        index on the device - a DeviceSlide is packed on the device (csrc/pack_rows.hip), a HostSlide on the host
        (:func:`pack_host_grid`; the kept rows go to pinned memory).  A masked view packs to a view: its masks and recorded max|x| are
        kept; else both come from the mask pass over the packed rows."""
        if self.packed:
            return self
        cached = dict(masks=self.masks, absmax=self.feature_absmax()) if self.masked_view else {}
        return self._build(self.grids, self.device, self.dtype, True, **cached, **self._ident())

    def to_dense(self):
        """The dense twin: every cell without a row becomes an all-zero row again (torch indexing: a construction-time path); its masks
        and max|x| are this slide's (no mask pass)."""
        if not self.packed:
            return self
        grids = [unpack_grid(r, ix.to(r.device)) for r, ix in zip(self.rows, self.index)]
        return self._build(grids, self.device, self.dtype, False, masks=self.masks, absmax=self.feature_absmax(), **self._ident())

    @classmethod
    def from_patches(cls, coords: Sequence, features: Sequence, shapes: Sequence, device="cuda", dtype=torch.float32, patch_size: int = 256,
                     slide_id: str = "", subtype=None, **kw):
        """A packed slide straight from the coords + features lists feature extractors write: ``coords[l]`` int64 [n_l, 2] cell
        coordinates (the convention of ``OnDemandSlide.encode``'s ``cells``), ``features[l]`` [n_l, D], ``shapes[l]`` = (X, Y).  Cells not
        listed are background; rows keep the given order; n_l = 0 is a level without tissue.  ValueError (before anything is launched:
        :func:`check_patches`) on a cell named twice or outside its grid, mismatched lengths, or a refused dtype; fp16 goes through
        :func:`to_float16`.  A HostSlide keeps the rows in pinned host memory (the same arguments, checks and row order)."""
        cells = check_patches(coords, features, shapes, dtype)
        levels = [(_patch_rows(f, dtype), _patch_index(c, sh)) for c, f, sh in zip(cells, features, shapes)]
        return cls._build(levels, device, dtype, True, patch_size=patch_size, slide_id=slide_id, subtype=subtype, **kw)

    @classmethod
    def from_host(cls, grids: Sequence, device="cuda", dtype=torch.float32, packed: bool = False, **kw):
        """Host grids (numpy or CPU tensors, e.g. ``torch.load('<slide>_<power:.3f>.pt')``) as ``dtype`` grids of the class: uploaded
        (DeviceSlide) or pinned (HostSlide; grids that already are pinned tensors of ``dtype`` are used where they are).  torch.float16:
        converted on the host by :func:`to_float16`, which raises on values fp16 cannot hold.  ``packed``: every level is converted,
        packed and dropped before the next one (what :meth:`pack` of the dense slide gives)."""
        if check_grid_dtype(dtype) == torch.float32:
            conv = lambda g: torch.as_tensor(g, dtype=torch.float32)
        else:       # (a HostSlide takes fp16 tensors as they are)
            conv = lambda g: g if (cls.host_resident and torch.is_tensor(g) and g.dtype == torch.float16) else to_float16(g)[0]
        return cls._build((conv(g) for g in grids), device, dtype, packed, **kw)

    @classmethod
    def from_preprocessed(cls, root: str, slide_id: str, powers: Sequence[float], device="cuda", patch_size: int = 256,
                          subtype=None, dtype=torch.float32, packed: bool = False, **kw):
        """Load the reference's preprocessed-grid files ``<root>/<slide_id>_<power:.3f>.pt`` (one ``[X, Y, D]`` float
        tensor per magnification, all-zero row = background; written by reference preprocess/preprocess.py:89,134 and
        read by preprocess/loader.py:14-18 / data_utils/slide.py:247-253) and keep them as ``dtype`` grids of the class (see
        :meth:`from_host`).  The dtype is checked before any file is read or the device is touched; a HostSlide also checks every path
        (FileNotFoundError) before it loads any."""
        import os
        check_grid_dtype(dtype)
        paths = [os.path.join(root, slide_id + f"_{power:.3f}.pt") for power in powers]
        for path in paths if cls.host_resident else ():
            if not os.path.isfile(path):
                raise FileNotFoundError(f"Pre-process load: path '{path}' not found!")
        grids = []
        for path in paths:
            assert os.path.isfile(path), f"Pre-process load: path '{path}' not found!"
            g = torch.load(path, map_location="cpu")
            assert g.dim() == 3, f"{path}: expected a [X, Y, D] grid, got {tuple(g.shape)}"
            grids.append(g.float() if dtype == torch.float32 else g)
        return cls.from_host(grids, device, dtype=dtype, packed=packed, patch_size=patch_size, slide_id=slide_id, subtype=subtype, **kw)

    @classmethod
    def synthetic(cls, seed: int, slide: int, base_shape: Tuple[int, int], dim: int = 1024, num_levels: int = 5, p_bg: float = 0.1,
                  device="cuda", patch_size: int = 256, dtype=torch.float32, packed: bool = False, **kw):
        """The counter-based synthetic pyramid: a DeviceSlide generates it directly in HBM (paths_synth_grid; torch.float16:
        paths_synth_grid_h16, the same values rounded to nearest even), a HostSlide on the host (synthetic.SyntheticSlide.grid: the same
        bytes) straight into pinned memory."""
        h16 = check_grid_dtype(dtype) == torch.float16
        spec = synthetic.SyntheticSlide(seed, slide, tuple(base_shape), dim, num_levels, p_bg, feature_dtype="float16" if h16 else "float32")
        levels = (cls._synth_level(spec, l, dtype, device, packed) for l in range(num_levels))
        return cls._build(levels, device, dtype, packed, patch_size=patch_size, slide_id=f"synthetic-{seed}-{slide}", synthetic_spec=spec, **kw)


class DeviceSlide(_Slide):
    _NEEDS_GPU = "a DeviceSlide lives on a GPU device"

    def __init__(self, grids: Sequence[torch.Tensor], patch_size: int = 256, slide_id: str = "", subtype=None):
        """``grids``: device tensors [X, Y, D], all torch.float32 or all torch.float16 (kept as they are: no fp32 copy is made)."""
        dtype = _level_dtype(grids, "DeviceSlide")
        for g in grids:
            _lib.require_cuda(g)
            assert g.dim() == 3
        self._build(grids, grids[0].device, dtype, False, patch_size=patch_size, slide_id=slide_id, subtype=subtype, into=self)

    @staticmethod
    def _put(t: torch.Tensor, device) -> torch.Tensor:
        return t.to(device).contiguous()

    @staticmethod
    def _pack_grid(g: torch.Tensor, device):
        return _pack_device_grid(g.to(device))

    def _row_chunks(self, tables):
        """One launch over each table, where it lives."""
        return ((l, 0, t.data_ptr(), t.shape[0]) for l, t in enumerate(tables) if t.shape[0])

    @staticmethod
    def _synth_level(spec, l: int, dtype, device, packed: bool) -> torch.Tensor:
        X, Y = spec.shape(l)
        g = torch.empty((X, Y, spec.dim), dtype=dtype, device=device)
        _lib.call(entry_name("paths_synth_grid", dtype == torch.float16), g.data_ptr(), X, Y, spec.dim,
                  int(synthetic.slide_level_key(spec.seed, spec.slide, l)), l, synthetic.bg_threshold(spec.p_bg), _lib.stream())
        return g

    @classmethod
    def from_patches(cls, coords: Sequence, features: Sequence, shapes: Sequence, device, dtype=torch.float32, patch_size: int = 256,
                     slide_id: str = "", subtype=None) -> "DeviceSlide":
        """:meth:`_Slide.from_patches`; a resident slide names its ``device``, and takes no mask-pass options."""
        return super().from_patches(coords, features, shapes, device, dtype, patch_size, slide_id, subtype)

    @classmethod
    def from_host(cls, grids: Sequence, device, dtype=torch.float32, packed: bool = False, **kw) -> "DeviceSlide":
        """:meth:`_Slide.from_host`; a resident slide names its ``device``."""
        return super().from_host(grids, device, dtype, packed, **kw)


def plan_mask_chunks(cells: int, D: int, itemsize: int, budget_bytes: int) -> List[Tuple[int, int]]:
    """Row chunks ``[(row0, rows), ...]`` in which a host grid of ``cells`` rows of ``D`` elements is streamed through a device bounce
    buffer of ``budget_bytes``: every row exactly once, in order, no chunk larger than the budget (the last one may be partial).
    Raises ValueError when the budget does not hold one row."""
    row_bytes = int(D) * int(itemsize)
    if cells <= 0 or row_bytes <= 0:
        raise ValueError(f"plan_mask_chunks: empty grid (cells {cells}, row of {row_bytes} bytes)")
    per = int(budget_bytes) // row_bytes
    if per < 1:
        raise ValueError(f"plan_mask_chunks: a bounce buffer of {budget_bytes} bytes does not hold one row of {row_bytes} bytes")
    return [(r0, min(per, cells - r0)) for r0 in range(0, cells, per)]


class HostSlide(_Slide):
    """A slide whose feature grids stay in PINNED host memory (the reference keeps them in host RAM too and gathers on the CPU,
    data_utils/slide.py:320-331).  The read surface is :class:`DeviceSlide`'s; ``grids[l]`` are CPU tensors [X, Y, D] that the
    device can address (pinned = device-mapped), ``masks[l]`` are the usual uint8 [X, Y] DEVICE tensors.  Device memory per slide is
    the masks alone (0.7 MB at K = 2048 x 5 levels against 2.86 GB of grids).  Packed: pinned ``rows`` + device ``index`` instead of
    ``grids``.

    The masks and max|x| come from ONE pass of the resident slides' kernel (paths_tissue_mask_absmax[_h16]) over the grid, streamed
    in row chunks through a bounded device bounce buffer (``bounce_bytes``, or a caller-owned uint8 device tensor ``bounce`` shared by
    many slides); ``masks=`` + ``absmax=`` skip the pass for callers who cached them.  Grids that are not pinned yet are copied into
    pinned memory here: a kernel must never be handed pageable memory."""

    host_resident = True
    _NEEDS_GPU = "a HostSlide needs a GPU device for its masks"

    def __init__(self, grids: Sequence[torch.Tensor], device="cuda", patch_size: int = 256, slide_id: str = "", subtype=None,
                 masks: Optional[Sequence[torch.Tensor]] = None, absmax: Optional[float] = None, bounce_bytes: int = 64 << 20,
                 bounce: Optional[torch.Tensor] = None):
        dtype = _level_dtype(grids, "HostSlide")
        if any(g.device.type != "cpu" or g.dim() != 3 for g in grids):
            raise ValueError("HostSlide: grids are CPU tensors [X, Y, D] (DeviceSlide holds device grids)")
        self._build(grids, device, dtype, False, masks, absmax, patch_size, slide_id, subtype, into=self, bounce_bytes=bounce_bytes,
                    bounce=bounce)

    @staticmethod
    def _put(t: torch.Tensor, device) -> torch.Tensor:
        """``t`` as a contiguous CPU tensor in pinned memory: itself when it already is, else a pinned copy (no rows: nothing to pin)."""
        t = t.cpu().contiguous()
        return t if (t.numel() == 0 or t.is_pinned()) else t.pin_memory()

    @staticmethod
    def _pack_grid(g: torch.Tensor, device):
        return pack_host_grid(g)

    def _row_chunks(self, tables, bounce_bytes: int = 64 << 20, bounce: Optional[torch.Tensor] = None):
        """Every table in row chunks through the bounce buffer (:func:`plan_mask_chunks`)."""
        dev, es, D = self.device, tables[0].element_size(), self.dim
        if bounce is None:
            # (no larger than the largest grid; whole rows)
            largest = max(max(t.numel() for t in tables), D) * es
            plan_mask_chunks(1, D, es, bounce_bytes)                       # raises if the budget holds no row
            bounce = torch.empty((min(int(bounce_bytes), largest),), dtype=torch.uint8, device=dev)
        else:
            _lib.require_cuda(bounce)
            assert bounce.dtype == torch.uint8 and bounce.is_contiguous() and bounce.data_ptr() % 16 == 0
        for l, flat in enumerate(tables):
            for r0, rows in (plan_mask_chunks(flat.shape[0], D, es, bounce.numel()) if flat.shape[0] else []):
                assert flat.is_pinned()
                chunk = bounce[:rows * D * es].view(self.dtype).view(rows, D)
                chunk.copy_(flat[r0:r0 + rows], non_blocking=True)               # same stream as the kernel: chunks follow each other
                yield l, r0, chunk.data_ptr(), rows

    @staticmethod
    def _synth_level(spec, l: int, dtype, device, packed: bool) -> torch.Tensor:
        X, Y = spec.shape(l)
        g = torch.empty((X, Y, spec.dim), dtype=dtype, pin_memory=not packed)
        g.copy_(torch.from_numpy(spec.grid(l)))             # (fp16: the values are fp16-representable already, the cast is exact)
        return g

    def host_bytes(self) -> int:
        """Pinned host memory held by the grids (packed: by the kept rows)."""
        return _nbytes(self.rows if self.packed else self.grids)

    def to_device(self) -> DeviceSlide:
        """The equivalent resident slide (a full upload of every grid; packed: of the kept rows - the twin is packed too) behind this
        slide's masks and max|x|."""
        levels = zip(self.rows, self.index) if self.packed else self.grids
        return DeviceSlide._build(levels, self.device, self.dtype, self.packed, masks=self.masks, absmax=self.feature_absmax(), **self._ident())


class _SlideBatch:
    """What :class:`DeviceSlideBatch` and :class:`OnDemandSlideBatch` share: the static per-level tables every recursion reads (``gx`` /
    ``gy`` / ``max_dim`` / ``n0`` / ``dim`` / ``dtype`` / ``num_levels``), the storage form of the slides, and the two things the launch
    code asks of it (:meth:`entry`, :meth:`index_args`)."""

    on_demand = False               # the rows of a level are supplied by the caller's encoder during the pass
    host_resident = False           # grid_ptrs hold pinned host addresses (the recursion stages the selected rows into HBM)
    packed = False                  # grid_ptrs hold every slide's first packed row, index_ptrs its cell index
    masked = False                  # some slide is a masked view (level 0 then reads cleared cells as zero rows)
    index_ptrs = None

    def __len__(self):
        return len(self.slides)

    def _derive(self, dev, rows_word: str):
        """``device`` and the tables that follow from the slides' shapes; ValueError when the slides differ in width or dtype."""
        who, slides = type(self).__name__, self.slides
        L = min(s.num_levels for s in slides)
        self.device, self.num_levels = dev, L
        self.dim = slides[0].dim
        if any(s.dim != self.dim for s in slides):
            raise ValueError(f"{who}: slides of one batch share the feature width")
        self.dtype = slides[0].dtype            # dtype of the whole batch: the recursion picks its kernels by it
        if any(s.dtype != self.dtype for s in slides):
            raise ValueError(f"{who}: slides of one batch must share the {rows_word} dtype (got "
                             + ", ".join(sorted({str(s.dtype) for s in slides})) + ")")
        extent = lambda k: [torch.tensor([s.shape(l)[k] for s in slides], device=dev, dtype=torch.int32) for l in range(L)]
        self.gx, self.gy = extent(0), extent(1)
        self.n0 = max(s.shape(0)[0] * s.shape(0)[1] for s in slides)
        self.max_dim = [max(max(s.shape(l)) for s in slides) for l in range(L)]   # bound of locs // patch_size per level

    def entry(self, name: str) -> str:
        """The entry point of an address-forming kernel (``paths_level0_batch``, ``paths_gather_rows``) for this batch's storage."""
        return entry_name(name, self.dtype == torch.float16, self.packed)

    def index_table(self, level: int) -> Optional[torch.Tensor]:
        """The cell-index table of ``level`` (a packed batch), else None."""
        return self.index_ptrs[level] if self.packed else None

    def index_args(self, level: int) -> tuple:
        """What that entry point takes in front of its stream for ``level``: the cell-index table of a packed batch, else nothing."""
        return index_args(self.index_table(level))


class DeviceSlideBatch(_SlideBatch):
    """Per-batch device tables (grid / mask base pointers and grid dims per level) built ONCE.

    ``torch.tensor(list, device=...)`` is a blocking host->device copy that also waits for everything queued on
    the stream; building these tables inside every recursion call cost ~1.5 ms of idle GPU per step.

    The slides are all :class:`DeviceSlide` or all :class:`HostSlide` (``host_resident``: ``grid_ptrs`` then hold pinned host
    addresses, which the device can dereference; the recursion stages the selected rows into HBM, paths_stage_rows).
    """

    def __init__(self, slides):
        assert len(slides) > 0
        self.slides = list(slides)
        # (the kind checks read tolerantly: stand-ins with the few attributes a check needs are enough to be refused)
        if any(getattr(s, "on_demand", False) for s in self.slides):
            raise ValueError("DeviceSlideBatch: on-demand slides (OnDemandSlide) form batches of their own (slide_batch / OnDemandSlideBatch), "
                             "not mixed with resident or host-resident slides")
        kinds = {bool(getattr(s, "host_resident", False)) for s in self.slides}
        if len(kinds) != 1:
            raise ValueError("DeviceSlideBatch: slides of one batch are all resident (DeviceSlide) or all host-resident (HostSlide)")
        self.host_resident = kinds.pop()
        forms = {bool(getattr(s, "packed", False)) for s in self.slides}
        if len(forms) != 1:
            raise ValueError("DeviceSlideBatch: slides of one batch are all packed or all dense (slide.pack() / slide.to_dense())")
        self.packed = forms.pop()
        self.masked = any(getattr(s, "masked_view", False) for s in self.slides)
        dev = (self.slides[0].masks if (self.host_resident or self.packed) else self.slides[0].grids)[0].device
        self._derive(dev, "grid")

        def table(fn):
            return [torch.tensor([fn(s, l) for s in self.slides], device=dev, dtype=torch.int64) for l in range(self.num_levels)]

        def grid_ptr(s, l):
            g = s.rows[l] if self.packed else s.grids[l]
            if g.numel() == 0:              # a packed level without rows: its index holds -1 only, the address is never dereferenced
                return 0
            if self.host_resident:          # a kernel that touches pageable host memory faults: only pinned grids get into the table
                assert (not g.is_cuda) and g.is_pinned() and g.is_contiguous(), "HostSlide grids must be pinned host memory"
            return g.data_ptr()

        self.grid_ptrs = table(grid_ptr)
        self.mask_ptrs = table(lambda s, l: s.masks[l].data_ptr())
        self.index_ptrs = table(lambda s, l: s.index[l].data_ptr()) if self.packed else None
        self.feat_absmax = max(s.feature_absmax() for s in self.slides)
        self._flat_tables = None

    def _tables(self) -> list:
        """The per-level table lists in the order of the flat layout: grid pointers, mask pointers, gx, gy; packed batches: + index
        pointers."""
        return [self.grid_ptrs, self.mask_ptrs, self.gx, self.gy] + ([self.index_ptrs] if self.packed else [])

    def flat_tables(self) -> torch.Tensor:
        """Every per-level table in ONE byte buffer, level by level in the order of :meth:`_tables`, built once per batch: binding a
        recorded launch tape to this batch is then a single small device-to-device copy."""
        if self._flat_tables is None:
            self._flat_tables = torch.cat([t[l].view(torch.uint8) for l in range(self.num_levels) for t in self._tables()])
        return self._flat_tables

    def clone_tables(self) -> "DeviceSlideBatch":
        """The same batch with PRIVATE copies of the table tensors (a recorded launch tape addresses these, and re-points them at
        other batches: paths_amd.utils.TapedRecursion.rebind); the slides themselves are shared.  The copies are views of one flat
        buffer laid out like :meth:`flat_tables`."""
        c = copy.copy(self)
        c._flat_tables = self.flat_tables().clone()
        order = [t[l] for l in range(self.num_levels) for t in self._tables()]
        views = [b.view(t.dtype) for b, t in zip(c._flat_tables.split([t.numel() * t.element_size() for t in order]), order)]
        k = len(order) // self.num_levels
        c.grid_ptrs, c.mask_ptrs, c.gx, c.gy = (views[j::k] for j in range(4))
        c.index_ptrs = views[4::k] if self.packed else None
        c.max_dim = list(self.max_dim)
        return c


class OnDemandSlide:
    """A slide whose features are encoded ON DEMAND: nothing is preprocessed, the recursion asks ``encode`` for the cells it is about
    to visit - all of level 0, then only the in-bounds children of the patches each level keeps (reference ``RawSlide.recurse``,
    data_utils/slide.py:173-198).  At K = 2048 x 5 levels that is at most 34,816 of the pyramid's 698,368 cells per pass.

    ``shapes[l]``: the (X, Y) grid size of level ``l`` (known from the slide's dimensions).  ``encode(level, cells)`` receives an int64
    ``[n, 2]`` tensor of cell coordinates on ``device`` (n >= 1) and returns ``[n, dim]`` features on that device in ``dtype``, an
    all-zero row meaning background (the grid contract of :class:`DeviceSlide`).  It is called with the recursion's stream current:
    work it enqueues there (or on streams it joins into the current one before returning) is ordered before the kernels that read the
    rows.  It is never asked for a cell outside the level's grid and never twice for the same cell within one pass; ``requested[l]``
    holds the cells asked of level ``l`` during the last pass (None: level not reached).

    WSI reading and the encoder are the caller's; the tissue masking of pixels and the hand-over to the
    encoder are ``paths_amd.pixels.TileEncoder``, an ``encode`` built from a tile reader and a model.  Inference only."""

    on_demand = True
    host_resident = False
    caching = False                 # (CachedOnDemandSlide: keeps the rows its encoder has produced)

    def __init__(self, shapes: Sequence[Tuple[int, int]], encode: Callable, dim: int, device, patch_size: int = 256,
                 dtype=torch.float32, slide_id: str = "", subtype=None):
        self.dtype = check_grid_dtype(dtype)
        self.shapes = [(int(x), int(y)) for x, y in shapes]
        if len(self.shapes) < 1 or any(x < 1 or y < 1 for x, y in self.shapes):
            raise ValueError(f"OnDemandSlide: shapes are the (X, Y) grid sizes of the levels, all positive (got {list(shapes)})")
        if not callable(encode):
            raise ValueError("OnDemandSlide: encode(level, cells) must be callable")
        if int(dim) < 4 or int(dim) % 4 != 0:
            raise ValueError(f"OnDemandSlide: the feature width must be a positive multiple of 4 (got {dim})")
        self.encode, self._dim = encode, int(dim)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.patch_size, self.slide_id, self.subtype = patch_size, slide_id, subtype
        self.synthetic_spec = None              # (from_slide: the source's)
        self.requested: List[Optional[torch.Tensor]] = [None] * len(self.shapes)

    @property
    def num_levels(self) -> int:
        return len(self.shapes)

    def shape(self, level: int) -> Tuple[int, int]:
        return self.shapes[level]

    @property
    def dim(self) -> int:
        return self._dim

    def with_masks(self, masks):
        raise NotImplementedError("OnDemandSlide.with_masks: an on-demand slide holds no tissue masks (background is what its encoder "
                                  "returns as all-zero rows); masked views are for DeviceSlide and HostSlide")

    def begin_pass(self):
        self.requested = [None] * len(self.shapes)

    def request(self, level: int, cells: torch.Tensor) -> Optional[torch.Tensor]:
        """Ask the encoder for ``cells`` (int64 [n, 2], inside the grid, no cell twice: the recursion's candidates are) of ``level``,
        once per level and pass; checks what comes back (ValueError) and returns it.  n = 0: nothing is asked, None."""
        if self.requested[level] is not None:
            raise RuntimeError(f"OnDemandSlide {self.slide_id!r}: level {level} was already requested in this pass")
        self.requested[level] = cells
        return self._encode(level, cells)

    def _encode(self, level: int, cells: torch.Tensor) -> Optional[torch.Tensor]:
        """``encode(level, cells)`` with its result checked (ValueError); n = 0: nothing is asked, None."""
        n = int(cells.shape[0])
        if n == 0:
            return None
        rows = self.encode(level, cells)
        if not torch.is_tensor(rows) or tuple(rows.shape) != (n, self._dim):
            got = tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__
            raise ValueError(f"OnDemandSlide {self.slide_id!r}: encode(level {level}) must return [{n}, {self._dim}] features, got {got}")
        if rows.dtype != self.dtype:
            raise ValueError(f"OnDemandSlide {self.slide_id!r}: encode(level {level}) returned {rows.dtype}, the slide's dtype is {self.dtype}")
        if rows.device != self.device:
            raise ValueError(f"OnDemandSlide {self.slide_id!r}: encode(level {level}) returned rows on {rows.device}, the slide lives on {self.device}")
        return rows

    @classmethod
    def from_slide(cls, slide, **kw) -> "OnDemandSlide":
        """A :class:`DeviceSlide` or :class:`HostSlide` behind the on-demand interface: ``encode`` indexes its grids (a preprocessed
        cohort replayed through this path; the twin of the tests and of tools/on_demand_time.py).  Anything with a slide's read surface
        will do: ``packed`` and ``synthetic_spec`` are read tolerantly."""
        packed = getattr(slide, "packed", False)
        dev = slide.device if slide.host_resident else (slide.index if packed else slide.grids)[0].device

        def encode(level, cells):
            if packed:            # through the cell index; a cell without a row is the all-zero row it was
                rows, ix = slide.rows[level], slide.index[level]
                c = cells.to(ix.device)
                r = ix[c[:, 0], c[:, 1]].to(rows.device, torch.int64)
                out = torch.zeros((r.shape[0], slide.dim), dtype=rows.dtype, device=rows.device)
                if rows.shape[0] > 0:
                    out[r >= 0] = rows[r[r >= 0]]
                return out.to(dev)
            g = slide.grids[level]
            c = cells.to(g.device)
            return g[c[:, 0], c[:, 1]].to(dev)

        s = cls([slide.shape(l) for l in range(slide.num_levels)], encode, slide.dim, dev, patch_size=slide.patch_size,
                dtype=slide.dtype, slide_id=slide.slide_id, subtype=slide.subtype, **kw)
        s.synthetic_spec = getattr(slide, "synthetic_spec", None)
        return s


class CachedOnDemandSlide(OnDemandSlide):
    """An :class:`OnDemandSlide` that KEEPS what its encoder has produced, on the device, across passes: a second
    ``recurse`` (with ``attention=True``, under the next fold's model, in a later epoch) pays the encoder only for cells no earlier
    pass has visited.  Same constructor plus ``max_rows`` - an int, or one int per level: the most rows the cache stores per level;
    None: no bound.

    Per level ``l`` it owns ``index[l]`` (int32 [X, Y] on the device: the row of a cell in the store, or -1; allocated when the level
    is first reached) and ``store[l]`` ([capacity, D] in the slide's dtype, ``count[l]`` rows in use, grown by doubling).  A row is
    stored exactly as ``encode`` returned it, an all-zero background row like any other.  At K = 2,048 x 5 levels that is at most
    34,816 rows = 142.6 MB per slide in fp32 (half in fp16) and 2.8 MB of indices.

    The contract towards ``encode`` changes in one word: it is called with the cells the cache does NOT hold, in request order
    (n >= 1), and not at all for a level whose cells are all held.  ``requested[l]`` is still what the recursion asked;
    ``encoded[l]`` is what the encoder was asked in the last pass (an empty [0, 2] tensor: all held; None: level not reached).
    ``stats`` counts requests, hits, misses and stored rows per level over the cache's life; :meth:`clear` empties the cache.  When
    ``max_rows[l]`` is reached the first ``max_rows[l] - count[l]`` misses in request order are stored and the rest pass through:
    encoded, used, not stored, asked again next time - results never depend on ``max_rows``.  Rows are never rewritten: a row the
    encoder got wrong (a NaN that made the pass raise) stays until :meth:`clear`.

    It stays ``on_demand``: whatever refuses an on-demand slide refuses this one.  :meth:`visited` hands the stored part over as an
    ordinary packed :class:`DeviceSlide`, on which every stored-slide entry point works."""

    caching = True

    def __init__(self, shapes: Sequence[Tuple[int, int]], encode: Callable, dim: int, device, patch_size: int = 256,
                 dtype=torch.float32, slide_id: str = "", subtype=None, max_rows=None):
        super().__init__(shapes, encode, dim, device, patch_size, dtype, slide_id, subtype)
        L = len(self.shapes)
        per_level = list(max_rows) if isinstance(max_rows, (list, tuple)) else [max_rows] * L
        if len(per_level) != L or any(m is not None and (isinstance(m, bool) or not isinstance(m, int) or m < 0) for m in per_level):
            raise ValueError(f"CachedOnDemandSlide: max_rows is None, a non-negative int or one per level ({L}), got {max_rows}")
        self.max_rows: List[Optional[int]] = per_level
        self.encoded: List[Optional[torch.Tensor]] = [None] * L
        self.clear()

    def clear(self):
        """Empty the cache: every index, store and count (``stats`` start again too)."""
        L = len(self.shapes)
        for t in list(getattr(self, "index", ())) + list(getattr(self, "store", ())):
            if t is not None and t.is_cuda:         # (a pass on another stream may still read them: not reused before that stream gets there)
                t.record_stream(torch.cuda.current_stream(t.device))
        self.index: List[Optional[torch.Tensor]] = [None] * L
        self.store: List[Optional[torch.Tensor]] = [None] * L
        self.count: List[int] = [0] * L
        self.stats = {k: [0] * L for k in ("requests", "hits", "misses", "stored")}

    def begin_pass(self):
        super().begin_pass()
        self.encoded = [None] * len(self.shapes)

    def row_limit(self, level: int) -> int:
        """The most rows level ``level`` can ever store: its cells, or ``max_rows[level]`` if that is fewer."""
        X, Y = self.shapes[level]
        m = self.max_rows[level]
        return X * Y if m is None else min(m, X * Y)

    def capacity(self, level: int) -> int:
        return 0 if self.store[level] is None else int(self.store[level].shape[0])

    def cell_index(self, level: int) -> torch.Tensor:
        """``index[level]``, allocated (all -1) on first use."""
        if self.index[level] is None:
            self.index[level] = torch.full(self.shapes[level], -1, dtype=torch.int32, device=self.device)
        return self.index[level]

    def reserve(self, level: int, more: int):
        """Room for ``more`` further rows at ``level``, as far as :meth:`row_limit` allows: the store is regrown by doubling (a copy
        enqueued on the current stream; the rows a running pass reads are the copies in its batch buffer, never these)."""
        need = min(self.count[level] + int(more), self.row_limit(level))
        cap = self.capacity(level)
        if need <= cap:
            return
        new = torch.empty((min(max(need, 2 * cap, 64), self.row_limit(level)), self._dim), dtype=self.dtype, device=self.device)
        old = self.store[level]
        if old is not None:
            new[:self.count[level]].copy_(old[:self.count[level]])
            old.record_stream(torch.cuda.current_stream(self.device))
        self.store[level] = new

    def request_misses(self, level: int, cells: torch.Tensor, misses: torch.Tensor) -> Optional[torch.Tensor]:
        """:meth:`request` for a level of which the cache holds all but ``misses`` (a subset of ``cells`` in request order): the encoder
        is asked for those alone, with the same checks.  The rows come back contiguous and 16-byte aligned (what paths_cache_fill reads)."""
        if self.requested[level] is not None:
            raise RuntimeError(f"OnDemandSlide {self.slide_id!r}: level {level} was already requested in this pass")
        self.requested[level], self.encoded[level] = cells, misses
        n, m = int(cells.shape[0]), int(misses.shape[0])
        for k, v in (("requests", n), ("hits", n - m), ("misses", m)):
            self.stats[k][level] += v
        rows = self._encode(level, misses)
        if rows is not None and (not rows.is_contiguous() or rows.data_ptr() % 16 != 0):
            rows = rows.clone(memory_format=torch.contiguous_format)
        return rows

    def note_stored(self, level: int, misses: int):
        """Host bookkeeping behind paths_cache_fill: the first ``capacity - count`` of ``misses`` rows are in the store now."""
        self.count[level] += max(0, min(int(misses), self.capacity(level) - self.count[level]))
        self.stats["stored"][level] = self.count[level]

    def export_patches(self):
        """``(coords, features, shapes)`` in :meth:`DeviceSlide.from_patches`' format: per level the stored cells (int64 [n_l, 2] device
        tensors) and their rows in insertion order.  ``features[l]`` is a VIEW of the store's first ``count[l]`` rows - they are never
        rewritten, so a slide built from them may share them; writing the lists to disk is the caller's."""
        coords, features = [], []
        for l, (X, Y) in enumerate(self.shapes):
            n = self.count[l]
            if n == 0:
                coords.append(torch.empty((0, 2), dtype=torch.int64, device=self.device))
                features.append(torch.empty((0, self._dim), dtype=self.dtype, device=self.device))
                continue
            coords.append(stored_cells(self.index[l], n))
            features.append(self.store[l][:n])
        return coords, features, list(self.shapes)

    def visited(self, packed: bool = True) -> "DeviceSlide":
        """The visited part of the slide as an ordinary stored slide (``DeviceSlide.from_patches`` of :meth:`export_patches`;
        ``packed=False``: its dense twin).  Cells no pass has asked for are background, stored background is what ``from_patches`` makes
        of all-zero rows (a row whose tissue mask is 0).

        With the model that filled the cache a free ``recurse`` on it takes the same path and gives the same results bit for bit -
        every cell it can reach was requested - and so do ``saliency.input_gradients`` / ``attention_relevance`` and the frozen-path
        functions given that pass's trace.  THE LIMIT: with OTHER weights (the next fold's model, a model after further training) the
        selection may leave the cached set, and those cells read as background, silently.  :func:`uncached_children` is the guard: all
        zeros for a pass's trace means the pass saw everything the full slide would have shown it.  With ``max_rows`` set the cache
        may not hold every requested cell, and the same guard tells.  Training an on-demand slide end to end stays out of scope."""
        coords, features, shapes = self.export_patches()
        s = DeviceSlide.from_patches(coords, features, shapes, self.device, self.dtype, self.patch_size, self.slide_id, self.subtype)
        s.synthetic_spec = self.synthetic_spec
        return s if packed else s.to_dense()

    def uncached_children(self, trace, keep_patches, patch_size: Optional[int] = None) -> torch.Tensor:
        """:func:`uncached_children` for the trace of a one-slide pass: int64 [levels]."""
        return uncached_children([self], trace, keep_patches, patch_size)[0]

    @classmethod
    def from_slide(cls, slide, max_rows=None) -> "CachedOnDemandSlide":
        """:meth:`OnDemandSlide.from_slide` with a cache in front of the stored slide's rows (the twin of the tests and of
        tools/on_demand_cache_time.py)."""
        return super().from_slide(slide, max_rows=max_rows)


def stored_cells(index: torch.Tensor, n: int) -> torch.Tensor:
    """int64 [n, 2] coordinates of the cells a cache index [X, Y] names, in the order of their rows 0 .. n - 1."""
    flat = index.reshape(-1)
    cells = torch.nonzero(flat >= 0).flatten()
    if int(cells.numel()) != int(n):
        raise RuntimeError(f"the cache index names {int(cells.numel())} cells for {n} stored rows (was a cell requested twice?)")
    lin = cells[torch.argsort(flat[cells])]
    Y = index.shape[1]
    return torch.stack([lin // Y, lin % Y], dim=1)


class OnDemandSlideBatch(_SlideBatch):
    """The batch type of :class:`OnDemandSlide`, beside :class:`DeviceSlideBatch`: the static per-level tables come from the shapes
    (``gx`` / ``gy`` / ``max_dim`` / ``n0`` / ``dim`` / ``dtype``); what a resident batch knows up front and this one cannot - the rows'
    addresses (``grid_ptrs[l]``: per slide, the first of the rows supplied for level ``l``) and max|x| (``feat_absmax``, of the rows
    supplied so far) - is per-pass state, filled by :meth:`supply` as the recursion goes (paths_amd/utils.py).

    A batch is all plain or all caching (:class:`CachedOnDemandSlide`; ``caching``): a caching batch serves :meth:`supply` from the
    slides' row caches and asks the encoders for the misses only (:meth:`_supply_cached`)."""

    on_demand = True

    def __init__(self, slides):
        assert len(slides) > 0
        self.slides = list(slides)
        if not all(getattr(s, "on_demand", False) for s in self.slides):
            raise ValueError("OnDemandSlideBatch: slides of one batch are all on-demand (OnDemandSlide); resident and host-resident "
                             "slides go into a DeviceSlideBatch")
        kinds = {bool(getattr(s, "caching", False)) for s in self.slides}
        if len(kinds) != 1:
            raise ValueError("OnDemandSlideBatch: slides of one batch are all caching (CachedOnDemandSlide) or all plain (OnDemandSlide)")
        self.caching = kinds.pop()
        dev = self.slides[0].device
        if dev.type != "cuda":
            raise _lib.PathsHipError("paths_amd runs on the GPU only: the slides of a batch live on a GPU device (no CPU fallback)")
        if any(s.device != dev for s in self.slides):
            raise ValueError("OnDemandSlideBatch: slides of one batch live on one device")
        self._derive(dev, "feature")
        # level 0 asks for every cell, row-major (reference data_utils/slide.py:257-269): the request tensors are built once
        self.cells0 = [torch.cartesian_prod(torch.arange(s.shape(0)[0], device=dev), torch.arange(s.shape(0)[1], device=dev)).reshape(-1, 2)
                       for s in self.slides]
        self._host = torch.empty((len(self.slides) + 1,), dtype=torch.int64).pin_memory()      # one read-back per level: num_out | max|x| bits
        if self.caching:        # the per-slide tables of the cache kernels: cells | n | index, and encoder rows | store | count | capacity
            self._tables_host = torch.empty((7, len(self.slides)), dtype=torch.int64).pin_memory()
        self.begin_pass()

    def begin_pass(self):
        for s in self.slides:
            s.begin_pass()
        self.grid_ptrs: List[Optional[torch.Tensor]] = [None] * self.num_levels
        self.feat_absmax = 0.0
        self.absmax_bits = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.supplied: List[torch.Tensor] = []        # the rows of every level: read in place until the pass's streams have joined

    def end_pass(self):
        self.supplied = []

    def supply(self, level: int, cells: Sequence[torch.Tensor], cap: int) -> torch.Tensor:
        """Ask slide b for ``cells[b]`` of ``level`` and put what it returns into rows [b, 0:n_b] of one ``[B, cap, D]`` buffer (the
        rest zero); ``grid_ptrs[level]`` then holds the address of every slide's first row.  Everything is enqueued on the current
        stream: the encoder's work is ordered before whatever the caller launches there next.  A caching batch fills the same buffer
        from the slides' caches and asks for the misses only (:meth:`_supply_cached`)."""
        B, D = len(self.slides), self.dim
        buf = torch.empty((B, cap, D), dtype=self.dtype, device=self.device)
        if self.caching:
            self._supply_cached(level, cells, buf)
        else:
            for b, s in enumerate(self.slides):
                n = int(cells[b].shape[0])
                assert n <= cap
                rows = s.request(level, cells[b])
                if rows is not None:
                    buf[b, :n].copy_(rows)
                if n < cap:
                    buf[b, n:].zero_()
        self.supplied.append(buf)
        # (base + b * slide stride, computed on the device: torch.tensor(list) would be a blocking upload)
        self.grid_ptrs[level] = torch.arange(B, device=self.device, dtype=torch.int64) * (cap * D * buf.element_size()) + buf.data_ptr()
        return buf

    def _supply_cached(self, level: int, cells: Sequence[torch.Tensor], buf: torch.Tensor):
        """:meth:`supply` for caching slides, all on the current stream: probe every slide's index -> ONE host read of the B
        miss counts -> ``encode`` per slide with misses, on its miss cells -> regrow the stores that need it -> fill ``buf`` (hit rows
        from the store, miss rows from the encoder and, while there is room, into the store and the index; the rest zero).  Each
        pinned table is rewritten only after a host synchronisation that follows its upload: the miss-count read here, :meth:`read_back`
        behind every supply."""
        B, cap, D = buf.shape
        with torch.cuda.device(self.device):
            tab, src, cnt, misses = _cache_probe(self.slides, level, cells, cap, D, self.gx[level], self.gy[level], self._tables_host[:3])
            enc = [s.request_misses(level, cells[b], misses[b]) for b, s in enumerate(self.slides)]
            for s, m in zip(self.slides, misses):
                s.reserve(level, int(m.shape[0]))
            host = self._tables_host[3:]
            host.copy_(torch.tensor([[0 if r is None else r.data_ptr() for r in enc],
                                     [0 if s.store[level] is None else s.store[level].data_ptr() for s in self.slides],
                                     [s.count[level] for s in self.slides], [s.capacity(level) for s in self.slides]], dtype=torch.int64))
            tab2 = torch.empty((4, B), dtype=torch.int64, device=self.device)
            tab2.copy_(host, non_blocking=True)
            p = lambda t: t.data_ptr()
            _lib.call(entry_name("paths_cache_fill", self.dtype == torch.float16), p(tab[0]), p(tab[1]), p(src), p(cnt[0]), p(tab2[0]), p(tab2[1]),
                      p(tab2[2]), p(tab2[3]), p(tab[2]), p(self.gx[level]), p(self.gy[level]), B, cap, D, p(buf), _lib.stream())
            for s, m in zip(self.slides, misses):
                s.note_stored(level, int(m.shape[0]))

    def read_back(self, num_out: Optional[torch.Tensor]) -> List[int]:
        """ONE host synchronisation with the current stream: max|x| of the rows supplied so far goes into ``feat_absmax`` (inf for an
        inf or NaN anywhere) and ``num_out`` [B] (optional) is returned as a list."""
        B = len(self.slides)
        if num_out is not None:
            self._host[:B].copy_(num_out, non_blocking=True)
        self._host[B:].copy_(self.absmax_bits, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self.feat_absmax = _lib.float_from_bits(int(self._host[B]))
        return self._host[:B].tolist() if num_out is not None else []


def any_on_demand(slides) -> bool:
    """Whether ``slides`` (a batch, or a list of slides or stand-ins) hold an on-demand slide."""
    if isinstance(slides, _SlideBatch):
        return slides.on_demand
    return any(getattr(s, "on_demand", False) for s in slides)


def _cache_probe(slides, level: int, cells: Sequence[torch.Tensor], n_max: int, D: int, gx: torch.Tensor, gy: torch.Tensor,
                 host: Optional[torch.Tensor] = None):
    """paths_cache_probe of ``cells[b]`` (int64 [n_b, 2], contiguous, n_b <= n_max) against the ``level`` index of every caching slide,
    on the current stream, and ONE host read of the miss counts.  ``host``: a pinned int64 [3, B] staging table (None: a blocking
    upload).  Returns (the device table [3, B] cells | n | index, src [B, n_max], (miss_count | status) [2, B], the per-slide miss
    cells as views [m_b, 2]).  A cell outside its grid raises PathsHipError."""
    B, dev = len(slides), slides[0].device
    rows = torch.tensor([[c.data_ptr() for c in cells], [int(c.shape[0]) for c in cells],
                         [s.cell_index(level).data_ptr() for s in slides]], dtype=torch.int64)
    assert all(c.dtype == torch.int64 and c.is_contiguous() and int(c.shape[0]) <= n_max for c in cells)
    if host is None:
        tab = rows.to(dev)
    else:
        host.copy_(rows)
        tab = torch.empty((3, B), dtype=torch.int64, device=dev)
        tab.copy_(host, non_blocking=True)
    src = torch.empty((B, n_max), dtype=torch.int32, device=dev)
    miss_cells = torch.empty((B, n_max, 2), dtype=torch.int64, device=dev)
    cnt = torch.empty((2, B), dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    _lib.call("paths_cache_probe", p(tab[0]), p(tab[1]), p(tab[2]), p(gx), p(gy), B, n_max, D, p(src), p(cnt[0]), p(miss_cells), p(cnt[1]),
              _lib.stream())
    counts, status = cnt.cpu().tolist()                     # the host read: waits for the current stream, i.e. for the probe
    bad = [b for b in range(B) if status[b]]
    if bad:
        names = ", ".join(repr(slides[b].slide_id or f"#{b}") for b in bad)
        raise _lib.PathsHipError(f"on-demand slide {names}: a cell requested at level {level} lies outside its grid")
    return tab, src, cnt, [miss_cells[b, :counts[b]] for b in range(B)]


def uncached_children(slides, trace, keep_patches, patch_size: Optional[int] = None) -> torch.Tensor:
    """The guard of :meth:`CachedOnDemandSlide.visited`: how many of the cells a pass WOULD have asked a full slide for the caches of
    ``slides`` (caching slides, or their batch) do not hold.  ``trace``: the pass's trace (``recurse(..., trace=[])``) over slides in
    the same order - e.g. of a pass run on the ``visited()`` slides under other weights.  Column 0 counts the level-0 cells; for every
    further level of the trace the existing paths_candidate_children runs on the level above's kept patches and paths_cache_probe on
    its candidates.  Returns the miss counts, int64 [B, len(trace)] on the host; all zeros: the pass saw everything the full slides
    would have shown it.  ``keep_patches``: the pass's (one entry per step of the trace); ``patch_size``: the model's (default: the
    slides').  One host read per level; the caches are left as they are."""
    slides = list(slides.slides) if isinstance(slides, _SlideBatch) else list(slides)
    if not slides or not all(getattr(s, "caching", False) for s in slides):
        raise ValueError("uncached_children: the slides are CachedOnDemandSlides")
    L, B, dev = len(trace), len(slides), slides[0].device
    if L < 1 or L > min(s.num_levels for s in slides) or L - 1 > len(keep_patches):
        raise ValueError(f"uncached_children: a trace of {L} levels does not fit the slides' levels / the {len(keep_patches)} keep_patches entries")
    ps = int(slides[0].patch_size if patch_size is None else patch_size)
    out = torch.zeros((B, L), dtype=torch.int64)
    p = lambda t: t.data_ptr()
    with torch.cuda.device(dev):
        for l in range(L):
            gx, gy = (torch.tensor([s.shape(l)[k] for s in slides], dtype=torch.int32, device=dev) for k in (0, 1))
            if l == 0:
                cells = [torch.cartesian_prod(torch.arange(s.shape(0)[0], device=dev), torch.arange(s.shape(0)[1], device=dev)).reshape(-1, 2)
                         for s in slides]
            else:
                t = trace[l - 1]
                keep_idx, keep_count = t["keep_idx"].to(torch.int32).contiguous(), t["keep_count"].to(torch.int32).contiguous()
                locs = t["locs"].to(torch.int64).contiguous()
                if keep_idx.shape[0] != B or locs.shape[0] != B:
                    raise ValueError(f"uncached_children: the trace holds {keep_idx.shape[0]} slides, {B} were given")
                ldk = int(keep_idx.shape[1])
                cand_count = torch.empty((B,), dtype=torch.int32, device=dev)
                cand_cells = torch.empty((B, 4 * ldk, 2), dtype=torch.int64, device=dev)
                cand_slot = torch.empty((B, 4 * ldk), dtype=torch.int32, device=dev)
                _lib.call("paths_candidate_children", p(keep_idx), ldk, p(keep_count), p(locs), int(locs.shape[1]), ps, p(gx), p(gy), B,
                          p(cand_count), p(cand_cells), p(cand_slot), _lib.stream())
                counts = cand_count.cpu().tolist()
                cells = [cand_cells[b, :counts[b]] for b in range(B)]
            n_max = max(1, max(int(c.shape[0]) for c in cells))
            misses = _cache_probe(slides, l, cells, n_max, slides[0].dim, gx, gy)[3]
            out[:, l] = torch.tensor([int(m.shape[0]) for m in misses])
    return out


def slide_batch(slides):
    """The batch of a list of slides: an :class:`OnDemandSlideBatch` for :class:`OnDemandSlide`s, else a :class:`DeviceSlideBatch`
    (which refuses a mix); a batch passes through."""
    if isinstance(slides, _SlideBatch):
        return slides
    slides = list(slides)
    if slides and all(getattr(s, "on_demand", False) for s in slides):
        return OnDemandSlideBatch(slides)
    return DeviceSlideBatch(slides)
