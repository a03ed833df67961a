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
about to visit (reference ``RawSlide.recurse``, data_utils/slide.py:173-198).

PACKED slides (``slide.pack()``, ``packed=True``, ``from_patches``) leave the background out: per level the kept rows
``rows[l]`` [n_l, D] behind a cell index ``index[l]`` (int32 [X, Y] on the device: the row of a cell, or -1).  Only rows that are all
+0.0 are dropped, and such a cell reads as the zero row it was, so every result is bit-identical to the dense twin's.
"""
from __future__ import annotations

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
    sfx = "_h16" if check_grid_dtype(g.dtype) == torch.float16 else ""
    flags = torch.empty((cells,), dtype=torch.uint8, device=dev)
    index = torch.empty((X, Y), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    partials = torch.empty((int(_lib.load().paths_pack_index_partials(cells)),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream()
        _lib.call("paths_pack_flags" + sfx, g.data_ptr(), cells, D, flags.data_ptr(), st)
        _lib.call("paths_pack_index", flags.data_ptr(), cells, index.data_ptr(), count.data_ptr(), partials.data_ptr(), st)
        n = int(count.item())
        rows = torch.empty((n, D), dtype=g.dtype, device=dev)
        if n > 0:
            _lib.call("paths_pack_rows" + sfx, g.data_ptr(), cells, D, index.data_ptr(), n, rows.data_ptr(), st)
    return rows, index


def _packed_slide(cls, rows, index, masks, patch_size, slide_id, subtype, **attrs):
    """A packed slide of ``cls`` around its level tables (no launch; the callers fill ``_absmax`` / ``_absmax_bits``)."""
    s = object.__new__(cls)
    s.dtype = check_grid_dtype(rows[0].dtype)
    if any(r.dtype != s.dtype for r in rows):
        raise ValueError(f"{cls.__name__}: all levels of a slide must have the same dtype")
    s.packed, s.grids = True, None
    s.rows, s.index, s.masks = list(rows), list(index), list(masks)
    s.patch_size, s.slide_id, s.subtype = patch_size, slide_id, subtype
    s._absmax_bits, s._absmax = None, None
    s.__dict__.update(attrs)
    return s


def _copy_spec(src, dst):
    if hasattr(src, "synthetic_spec"):
        dst.synthetic_spec = src.synthetic_spec
    return dst


def _masked_view(slide, masks):
    """The view behind DeviceSlide.with_masks / HostSlide.with_masks: a shallow copy of ``slide`` that carries ``masks``."""
    masks = list(masks)
    if len(masks) != slide.num_levels:
        raise ValueError(f"with_masks: one mask per level ({slide.num_levels}) expected, got {len(masks)}")
    for l, (m, own) in enumerate(zip(masks, slide.masks)):
        if not torch.is_tensor(m) or m.dtype != torch.uint8 or tuple(m.shape) != tuple(slide.shape(l)) or not m.is_contiguous():
            got = f"{m.dtype} {tuple(m.shape)}" if torch.is_tensor(m) else type(m).__name__
            raise ValueError(f"with_masks: level {l} needs a contiguous uint8 [X, Y] = {list(slide.shape(l))} tensor, got {got}")
        if m.device != own.device:
            raise ValueError(f"with_masks: the mask of level {l} lives on {m.device}, the slide's masks on {own.device}")
    view = object.__new__(type(slide))
    view.__dict__.update(slide.__dict__)
    view.masks = masks
    view.masked_view = True
    view._absmax = slide.feature_absmax()             # the recorded max|x| of the source (its cached value: no launch)
    return view


class DeviceSlide:
    host_resident = False           # the grids live in HBM (HostSlide: in pinned host memory)
    masked_view = False             # (with_masks: the same grids behind other tissue masks)
    packed = False                  # (pack() / packed=True / from_patches: ``rows`` + ``index`` instead of ``grids``)
    rows = None
    index = None

    def __init__(self, grids: Sequence[torch.Tensor], patch_size: int = 256, slide_id: str = "", subtype=None):
        """``grids``: device tensors [X, Y, D], all torch.float32 or all torch.float16 (kept as they are: no fp32 copy is made)."""
        assert len(grids) >= 1
        self.dtype = check_grid_dtype(grids[0].dtype)
        if any(g.dtype != self.dtype for g in grids):
            raise ValueError("DeviceSlide: all levels of a slide must have the same dtype")
        self.patch_size = patch_size
        self.slide_id = slide_id
        self.subtype = subtype
        self.grids: List[torch.Tensor] = []
        self.masks: List[torch.Tensor] = []
        self._absmax_bits = None          # fp32 bit pattern of max|feature| over all levels, written by the mask pass
        self._absmax: Optional[float] = None
        for g in grids:
            _lib.require_cuda(g)
            assert g.dim() == 3
            g = g.contiguous()
            X, Y, D = g.shape
            m = torch.empty((X, Y), dtype=torch.uint8, device=g.device)
            if self._absmax_bits is None:
                self._absmax_bits = torch.zeros((1,), dtype=torch.int32, device=g.device)
            _lib.call("paths_tissue_mask_absmax_h16" if self.dtype == torch.float16 else "paths_tissue_mask_absmax", g.data_ptr(), X * Y, D,
                      m.data_ptr(), self._absmax_bits.data_ptr(), _lib.stream())
            self.grids.append(g)
            self.masks.append(m)

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
        return _masked_view(self, masks)

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
        """Device memory held by the slide: grids + masks, packed rows + index + masks."""
        nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)
        return nbytes(self.rows) + nbytes(self.index) + nbytes(self.masks) if self.packed else nbytes(self.grids) + nbytes(self.masks)

    @staticmethod
    def _packed_levels(levels, patch_size: int = 256, slide_id: str = "", subtype=None) -> "DeviceSlide":
        """The packed slide of ``levels``, an iterable of (rows, index) device pairs or of dense device grids (packed here and dropped
        before the next one is asked for: peak memory is the packed slide plus one dense level).  Masks and max|x| come from the mask
        pass over the PACKED rows (the per-row flags go to their cells through the index)."""
        rows, index, masks, bits = [], [], [], None
        for lv in levels:
            r, ix = lv if isinstance(lv, tuple) else _pack_device_grid(lv)
            del lv
            _lib.require_cuda(r, ix)
            if bits is None:
                bits = torch.zeros((1,), dtype=torch.int32, device=ix.device)
            flags = None
            if r.shape[0] > 0:
                flags = torch.empty((r.shape[0],), dtype=torch.uint8, device=r.device)
                with torch.cuda.device(r.device):
                    _lib.call("paths_tissue_mask_absmax_h16" if r.dtype == torch.float16 else "paths_tissue_mask_absmax", r.data_ptr(),
                              r.shape[0], r.shape[1], flags.data_ptr(), bits.data_ptr(), _lib.stream())
            rows.append(r); index.append(ix); masks.append(_scatter_flags(flags, ix))
        return _packed_slide(DeviceSlide, rows, index, masks, patch_size, slide_id, subtype, _absmax_bits=bits)

    def pack(self) -> "DeviceSlide":
        """The packed twin (this slide is left as it is): per level the rows with any bit set, in row-major cell order, behind the cell
        index - packed on the device (csrc/pack_rows.hip).  A masked view packs to a view: its masks and recorded max|x| are kept."""
        if self.packed:
            return self
        if self.masked_view:
            pairs = [_pack_device_grid(g) for g in self.grids]
            s = _packed_slide(DeviceSlide, [r for r, _ in pairs], [ix for _, ix in pairs], self.masks, self.patch_size, self.slide_id,
                              self.subtype, _absmax=self.feature_absmax(), masked_view=True)
        else:
            s = DeviceSlide._packed_levels(self.grids, self.patch_size, self.slide_id, self.subtype)
        return _copy_spec(self, s)

    def to_dense(self) -> "DeviceSlide":
        """The dense twin: every cell without a row becomes an all-zero row again (torch indexing: a construction-time path)."""
        if not self.packed:
            return self
        s = DeviceSlide([unpack_grid(r, ix) for r, ix in zip(self.rows, self.index)], patch_size=self.patch_size, slide_id=self.slide_id,
                        subtype=self.subtype)
        return _copy_spec(self, s.with_masks(self.masks) if self.masked_view else s)

    @staticmethod
    def from_patches(coords: Sequence, features: Sequence, shapes: Sequence, device, dtype=torch.float32, patch_size: int = 256,
                     slide_id: str = "", subtype=None) -> "DeviceSlide":
        """A packed slide straight from the coords + features lists feature extractors write: ``coords[l]`` int64 [n_l, 2] cell
        coordinates (the convention of ``OnDemandSlide.encode``'s ``cells``), ``features[l]`` [n_l, D], ``shapes[l]`` = (X, Y).  Cells not
        listed are background; rows keep the given order; n_l = 0 is a level without tissue.  ValueError (before anything is launched:
        :func:`check_patches`) on a cell named twice or outside its grid, mismatched lengths, or a refused dtype; fp16 goes through
        :func:`to_float16`."""
        cells = check_patches(coords, features, shapes, dtype)
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.PathsHipError("paths_amd runs on the GPU only: a DeviceSlide lives on a GPU device (no CPU fallback)")
        levels = [(_patch_rows(f, dtype).to(device), _patch_index(c, sh).to(device)) for c, f, sh in zip(cells, features, shapes)]
        return DeviceSlide._packed_levels(levels, patch_size, slide_id, subtype)

    @staticmethod
    def from_host(grids: Sequence, device, dtype=torch.float32, packed: bool = False, **kw) -> "DeviceSlide":
        """Upload host grids (numpy or CPU tensors, e.g. ``torch.load('<slide>_<power:.3f>.pt')``) as ``dtype`` grids
        (torch.float16: converted on the host by :func:`to_float16`, which raises on values fp16 cannot hold).  ``packed``: every level
        is uploaded, packed and dropped before the next one (what :meth:`pack` of the dense slide gives)."""
        if check_grid_dtype(dtype) == torch.float16:
            up = lambda g: to_float16(g)[0].to(device)
        else:
            up = lambda g: torch.as_tensor(g, dtype=torch.float32).to(device)
        if packed:
            return DeviceSlide._packed_levels((up(g) for g in grids), **kw)
        return DeviceSlide([up(g) for g in grids], **kw)

    @staticmethod
    def from_preprocessed(root: str, slide_id: str, powers: Sequence[float], device="cuda", patch_size: int = 256,
                          subtype=None, dtype=torch.float32, packed: bool = False) -> "DeviceSlide":
        """Load the reference's preprocessed-grid files ``<root>/<slide_id>_<power:.3f>.pt`` (one ``[X, Y, D]`` float
        tensor per magnification, all-zero row = background; written by reference preprocess/preprocess.py:89,134 and
        read by preprocess/loader.py:14-18 / data_utils/slide.py:247-253) and make them resident in HBM as ``dtype`` grids
        (see :meth:`from_host`)."""
        import os
        check_grid_dtype(dtype)                 # before any file is read or the device is touched
        grids = []
        for power in powers:
            path = os.path.join(root, slide_id + f"_{power:.3f}.pt")
            assert os.path.isfile(path), f"Pre-process load: path '{path}' not found!"
            g = torch.load(path, map_location="cpu")
            assert g.dim() == 3, f"{path}: expected a [X, Y, D] grid, got {tuple(g.shape)}"
            grids.append(g.float() if dtype == torch.float32 else g)
        return DeviceSlide.from_host(grids, device, dtype=dtype, packed=packed, patch_size=patch_size, slide_id=slide_id, subtype=subtype)

    @staticmethod
    def synthetic(seed: int, slide: int, base_shape: Tuple[int, int], dim: int = 1024, num_levels: int = 5,
                  p_bg: float = 0.1, device="cuda", patch_size: int = 256, dtype=torch.float32, packed: bool = False) -> "DeviceSlide":
        """Generate the counter-based synthetic pyramid directly in HBM (paths_synth_grid; torch.float16: paths_synth_grid_h16, the same
        values rounded to nearest even)."""
        h16 = check_grid_dtype(dtype) == torch.float16
        thr = synthetic.bg_threshold(p_bg)

        def level(l):
            X, Y = base_shape[0] << l, base_shape[1] << l
            g = torch.empty((X, Y, dim), dtype=dtype, device=device)
            key = int(synthetic.slide_level_key(seed, slide, l))
            _lib.call("paths_synth_grid_h16" if h16 else "paths_synth_grid", g.data_ptr(), X, Y, dim, key, l, thr, _lib.stream())
            return g

        if packed:
            s = DeviceSlide._packed_levels((level(l) for l in range(num_levels)), patch_size, f"synthetic-{seed}-{slide}")
        else:
            s = DeviceSlide([level(l) for l in range(num_levels)], patch_size=patch_size, slide_id=f"synthetic-{seed}-{slide}")
        s.synthetic_spec = synthetic.SyntheticSlide(seed, slide, tuple(base_shape), dim, num_levels, p_bg,
                                                    feature_dtype="float16" if h16 else "float32")
        return s


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


def _pinned(g: torch.Tensor) -> torch.Tensor:
    """``g`` (CPU, contiguous) in pinned memory: itself when it already is, else a pinned copy."""
    return g if g.is_pinned() else g.pin_memory()


class HostSlide:
    """A slide whose feature grids stay in PINNED host memory (the reference keeps them in host RAM too and gathers on the CPU,
    data_utils/slide.py:320-331).  The read surface is :class:`DeviceSlide`'s; ``grids[l]`` are CPU tensors [X, Y, D] that the
    device can address (pinned = device-mapped), ``masks[l]`` are the usual uint8 [X, Y] DEVICE tensors.  Device memory per slide is
    the masks alone (0.7 MB at K = 2048 x 5 levels against 2.86 GB of grids).

    The masks and max|x| come from ONE pass of the resident slides' kernel (paths_tissue_mask_absmax[_h16]) over the grid, streamed
    in row chunks through a bounded device bounce buffer (``bounce_bytes``, or a caller-owned uint8 device tensor ``bounce`` shared by
    many slides); ``masks=`` + ``absmax=`` skip the pass for callers who cached them.  Grids that are not pinned yet are copied into
    pinned memory here: a kernel must never be handed pageable memory."""

    host_resident = True
    packed = False                  # (pack() / packed=True / from_patches: pinned ``rows`` + device ``index`` instead of ``grids``)
    rows = None
    index = None

    def __init__(self, grids: Sequence[torch.Tensor], device="cuda", patch_size: int = 256, slide_id: str = "", subtype=None,
                 masks: Optional[Sequence[torch.Tensor]] = None, absmax: Optional[float] = None, bounce_bytes: int = 64 << 20,
                 bounce: Optional[torch.Tensor] = None):
        assert len(grids) >= 1
        self.dtype = check_grid_dtype(grids[0].dtype)
        if any(g.dtype != self.dtype for g in grids):
            raise ValueError("HostSlide: all levels of a slide must have the same dtype")
        if any(g.device.type != "cpu" or g.dim() != 3 for g in grids):
            raise ValueError("HostSlide: grids are CPU tensors [X, Y, D] (DeviceSlide holds device grids)")
        if (masks is None) != (absmax is None):
            raise ValueError("HostSlide: cached masks= and absmax= come together")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PathsHipError("paths_amd runs on the GPU only: a HostSlide needs a GPU device for its masks (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.patch_size = patch_size
        self.slide_id = slide_id
        self.subtype = subtype
        self.grids: List[torch.Tensor] = [_pinned(g.contiguous()) for g in grids]
        self.masks: List[torch.Tensor] = []
        self._absmax_bits = None
        self._absmax: Optional[float] = None
        if masks is not None:
            for g, m in zip(self.grids, masks):
                _lib.require_cuda(m)
                if m.dtype != torch.uint8 or tuple(m.shape) != tuple(g.shape[:2]) or not m.is_contiguous():
                    raise ValueError("HostSlide: masks are contiguous uint8 [X, Y] device tensors, one per grid")
            self.masks = list(masks)
            self._absmax = float(absmax)
            return
        with torch.cuda.device(self.device):
            self._mask_pass(int(bounce_bytes), bounce)

    def _mask_pass(self, bounce_bytes: int, bounce: Optional[torch.Tensor]):
        # (packed: the pass streams the PACKED rows; the per-row flags go to their cells through the index)
        tables = self.rows if self.packed else [g.view(-1, g.shape[2]) for g in self.grids]
        dev, es = self.device, tables[0].element_size()
        if bounce is None:
            # (no larger than the largest grid; whole rows)
            largest = max(max(t.numel() for t in tables), self.dim) * es
            plan_mask_chunks(1, self.dim, es, bounce_bytes)                       # raises if the budget holds no row
            bounce = torch.empty((min(int(bounce_bytes), largest),), dtype=torch.uint8, device=dev)
        else:
            _lib.require_cuda(bounce)
            assert bounce.dtype == torch.uint8 and bounce.is_contiguous() and bounce.data_ptr() % 16 == 0
        self._absmax_bits = torch.zeros((1,), dtype=torch.int32, device=dev)
        name = "paths_tissue_mask_absmax_h16" if self.dtype == torch.float16 else "paths_tissue_mask_absmax"
        for l, flat in enumerate(tables):
            cells, D = flat.shape
            m = torch.empty((cells,), dtype=torch.uint8, device=dev) if cells else None
            for r0, rows in (plan_mask_chunks(cells, D, es, bounce.numel()) if cells else []):
                assert flat.is_pinned()
                chunk = bounce[:rows * D * es].view(self.dtype).view(rows, D)
                chunk.copy_(flat[r0:r0 + rows], non_blocking=True)               # same stream as the kernel: chunks follow each other
                _lib.call(name, chunk.data_ptr(), rows, D, m.data_ptr() + r0, self._absmax_bits.data_ptr(), _lib.stream())
            self.masks.append(_scatter_flags(m, self.index[l]) if self.packed else m.view(self.grids[l].shape[:2]))
        # the host must not re-use or free the bounce buffer's view of the last chunk early; the pass is once per slide
        torch.cuda.current_stream(dev).synchronize()

    masked_view = False
    with_masks = DeviceSlide.with_masks
    feature_absmax = DeviceSlide.feature_absmax
    num_levels = DeviceSlide.num_levels
    shape = DeviceSlide.shape
    dim = DeviceSlide.dim

    def host_bytes(self) -> int:
        """Pinned host memory held by the grids (packed: by the kept rows)."""
        return sum(g.numel() * g.element_size() for g in (self.rows if self.packed else self.grids))

    def resident_bytes(self) -> int:
        """Device memory held by the slide: the masks, and a packed slide's cell index."""
        return sum(t.numel() * t.element_size() for t in (self.index if self.packed else []) + self.masks)

    def to_device(self) -> DeviceSlide:
        """The equivalent resident slide (a full upload of every grid; packed: of the kept rows - the twin is packed too)."""
        if self.packed:
            s = _packed_slide(DeviceSlide, [r.to(self.device, non_blocking=True) for r in self.rows], self.index, self.masks, self.patch_size,
                              self.slide_id, self.subtype, _absmax=self.feature_absmax(), masked_view=self.masked_view)
            torch.cuda.current_stream(self.device).synchronize()
            return _copy_spec(self, s)
        s = DeviceSlide([g.to(self.device, non_blocking=True) for g in self.grids], patch_size=self.patch_size, slide_id=self.slide_id,
                        subtype=self.subtype)
        if hasattr(self, "synthetic_spec"):
            s.synthetic_spec = self.synthetic_spec
        return s

    @staticmethod
    def _packed_levels(levels, device="cuda", patch_size: int = 256, slide_id: str = "", subtype=None, masks=None, absmax=None,
                       bounce_bytes: int = 64 << 20, bounce: Optional[torch.Tensor] = None, masked_view: bool = False) -> "HostSlide":
        """The packed slide of ``levels``, an iterable of (rows, index) CPU pairs or of dense CPU grids (packed by
        :func:`pack_host_grid` and dropped before the next one is asked for).  Rows go to pinned memory, the index to the device; the
        mask pass streams the packed rows through the bounce buffer (``masks=`` + ``absmax=`` skip it)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.PathsHipError("paths_amd runs on the GPU only: a HostSlide needs a GPU device for its masks (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if (masks is None) != (absmax is None):
            raise ValueError("HostSlide: cached masks= and absmax= come together")
        rows, index = [], []
        for lv in levels:
            r, ix = lv if isinstance(lv, tuple) else pack_host_grid(lv)
            del lv
            if r.device.type != "cpu" or r.dim() != 2:
                raise ValueError("HostSlide: packed rows are CPU tensors [n, D]")
            rows.append(_pinned(r.contiguous()) if r.numel() else r)
            index.append(ix.to(device))
        s = _packed_slide(HostSlide, rows, index, [], patch_size, slide_id, subtype, device=device, masked_view=masked_view)
        if masks is not None:
            s.masks, s._absmax = list(masks), float(absmax)
        else:
            with torch.cuda.device(device):
                s._mask_pass(int(bounce_bytes), bounce)
                torch.cuda.current_stream(device).synchronize()
        return s

    def pack(self) -> "HostSlide":
        """The packed twin (this slide is left as it is), packed on the host by :func:`pack_host_grid`: the kept rows in pinned memory,
        the cell index on the device.  A masked view packs to a view: its masks and recorded max|x| are kept."""
        if self.packed:
            return self
        kw = dict(masks=self.masks, absmax=self.feature_absmax(), masked_view=True) if self.masked_view else {}
        return _copy_spec(self, HostSlide._packed_levels(self.grids, self.device, self.patch_size, self.slide_id, self.subtype, **kw))

    def to_dense(self) -> "HostSlide":
        """The dense twin in pinned memory (its masks and max|x| are this slide's: no mask pass)."""
        if not self.packed:
            return self
        s = HostSlide([unpack_grid(r, ix.cpu()) for r, ix in zip(self.rows, self.index)], device=self.device, patch_size=self.patch_size,
                      slide_id=self.slide_id, subtype=self.subtype, masks=self.masks, absmax=self.feature_absmax())
        s.masked_view = self.masked_view
        return _copy_spec(self, s)

    @staticmethod
    def from_patches(coords: Sequence, features: Sequence, shapes: Sequence, device="cuda", dtype=torch.float32, patch_size: int = 256,
                     slide_id: str = "", subtype=None, **kw) -> "HostSlide":
        """:meth:`DeviceSlide.from_patches` with the rows kept in pinned host memory (the same arguments, checks and row order)."""
        cells = check_patches(coords, features, shapes, dtype)
        levels = [(_patch_rows(f, dtype).cpu(), _patch_index(c, sh)) for c, f, sh in zip(cells, features, shapes)]
        return HostSlide._packed_levels(levels, device, patch_size, slide_id, subtype, **kw)

    @staticmethod
    def from_host(grids: Sequence, device="cuda", dtype=torch.float32, packed: bool = False, **kw) -> "HostSlide":
        """Host grids (numpy or CPU tensors) as pinned ``dtype`` grids (torch.float16: converted by :func:`to_float16`, which raises on
        values fp16 cannot hold).  Grids that already are pinned tensors of ``dtype`` are used where they are.  ``packed``: every level
        is converted, packed and dropped before the next one."""
        if check_grid_dtype(dtype) == torch.float16:
            conv = lambda g: g if (torch.is_tensor(g) and g.dtype == torch.float16) else to_float16(g)[0]
        else:
            conv = lambda g: torch.as_tensor(g, dtype=torch.float32)
        if packed:
            return HostSlide._packed_levels((conv(g) for g in grids), device, **kw)
        return HostSlide([conv(g) for g in grids], device=device, **kw)

    @staticmethod
    def from_preprocessed(root: str, slide_id: str, powers: Sequence[float], device="cuda", patch_size: int = 256,
                          subtype=None, dtype=torch.float32, packed: bool = False, **kw) -> "HostSlide":
        """The file contract of :meth:`DeviceSlide.from_preprocessed` (``<root>/<slide_id>_<power:.3f>.pt``, one [X, Y, D] float tensor
        per magnification), kept in pinned host memory.  The dtype and every path are checked before the device is touched."""
        import os
        check_grid_dtype(dtype)
        paths = [os.path.join(root, slide_id + f"_{power:.3f}.pt") for power in powers]
        for path in paths:
            if not os.path.isfile(path):
                raise FileNotFoundError(f"Pre-process load: path '{path}' not found!")
        grids = []
        for path in paths:
            g = torch.load(path, map_location="cpu")
            assert g.dim() == 3, f"{path}: expected a [X, Y, D] grid, got {tuple(g.shape)}"
            grids.append(g.float() if dtype == torch.float32 else g)
        return HostSlide.from_host(grids, device, dtype=dtype, packed=packed, patch_size=patch_size, slide_id=slide_id, subtype=subtype, **kw)

    @staticmethod
    def synthetic(seed: int, slide: int, base_shape: Tuple[int, int], dim: int = 1024, num_levels: int = 5, p_bg: float = 0.1,
                  device="cuda", patch_size: int = 256, dtype=torch.float32, packed: bool = False, **kw) -> "HostSlide":
        """The counter-based synthetic pyramid of :meth:`DeviceSlide.synthetic`, generated on the host (synthetic.SyntheticSlide.grid:
        the same bytes) straight into pinned memory."""
        h16 = check_grid_dtype(dtype) == torch.float16
        spec = synthetic.SyntheticSlide(seed, slide, tuple(base_shape), dim, num_levels, p_bg, feature_dtype="float16" if h16 else "float32")

        def level(l):
            X, Y = spec.shape(l)
            g = torch.empty((X, Y, dim), dtype=dtype, pin_memory=not packed)
            g.copy_(torch.from_numpy(spec.grid(l)))             # (fp16: the values are fp16-representable already, the cast is exact)
            return g

        if packed:
            s = HostSlide._packed_levels((level(l) for l in range(num_levels)), device, patch_size, f"synthetic-{seed}-{slide}", **kw)
        else:
            s = HostSlide([level(l) for l in range(num_levels)], device=device, patch_size=patch_size, slide_id=f"synthetic-{seed}-{slide}", **kw)
        s.synthetic_spec = spec
        return s


class DeviceSlideBatch:
    """Per-batch device tables (grid / mask base pointers and grid dims per level) built ONCE.

    ``torch.tensor(list, device=...)`` is a blocking host->device copy that also waits for everything queued on
    the stream; building these tables inside every recursion call cost ~1.5 ms of idle GPU per step.

    The slides are all :class:`DeviceSlide` or all :class:`HostSlide` (``host_resident``: ``grid_ptrs`` then hold pinned host
    addresses, which the device can dereference; the recursion stages the selected rows into HBM, paths_stage_rows).
    """

    on_demand = False               # (OnDemandSlideBatch: the rows of a level are supplied by the caller's encoder during the pass)

    def __init__(self, slides):
        assert len(slides) > 0
        self.slides = list(slides)
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
        self.packed = forms.pop()        # packed: grid_ptrs hold every slide's first packed row, index_ptrs its cell index
        self.masked = any(getattr(s, "masked_view", False) for s in self.slides)     # (level 0 then reads cleared cells as zero rows)
        dev = (self.slides[0].masks if (self.host_resident or self.packed) else self.slides[0].grids)[0].device
        L = min(s.num_levels for s in self.slides)
        self.device, self.num_levels = dev, L
        self.dim = self.slides[0].dim
        assert all(s.dim == self.dim for s in self.slides)
        self.dtype = self.slides[0].dtype            # grid dtype of the whole batch: the recursion picks its kernels by it
        if any(s.dtype != self.dtype for s in self.slides):
            raise ValueError("DeviceSlideBatch: slides of one batch must share the grid dtype (got "
                             + ", ".join(sorted({str(s.dtype) for s in self.slides})) + ")")

        def table(fn, dtype):
            return [torch.tensor([fn(s, l) for s in self.slides], device=dev, dtype=dtype) for l in range(L)]

        def grid_ptr(s, l):
            g = s.rows[l] if self.packed else s.grids[l]
            if g.numel() == 0:              # a packed level without rows: its index holds -1 only, the address is never dereferenced
                return 0
            if self.host_resident:          # a kernel that touches pageable host memory faults: only pinned grids get into the table
                assert (not g.is_cuda) and g.is_pinned() and g.is_contiguous(), "HostSlide grids must be pinned host memory"
            return g.data_ptr()

        self.grid_ptrs = table(grid_ptr, torch.int64)
        self.mask_ptrs = table(lambda s, l: s.masks[l].data_ptr(), torch.int64)
        self.index_ptrs = table(lambda s, l: s.index[l].data_ptr(), torch.int64) if self.packed else None
        self.gx = table(lambda s, l: s.shape(l)[0], torch.int32)
        self.gy = table(lambda s, l: s.shape(l)[1], torch.int32)
        self.n0 = max(s.shape(0)[0] * s.shape(0)[1] for s in self.slides)
        self.feat_absmax = max(s.feature_absmax() for s in self.slides)
        self.max_dim = [max(max(s.shape(l)) for s in self.slides) for l in range(L)]   # bound of locs // patch_size per level

    def __len__(self):
        return len(self.slides)

    def flat_tables(self) -> torch.Tensor:
        """Every per-level table in ONE byte buffer, level by level (grid pointers, mask pointers, gx, gy; packed batches: + index
        pointers), built once per batch: binding a recorded launch tape to this batch is then a single small device-to-device copy."""
        flat = getattr(self, "_flat_tables", None)
        if flat is None:
            parts = []
            for l in range(self.num_levels):
                parts += [self.grid_ptrs[l].view(torch.uint8), self.mask_ptrs[l].view(torch.uint8), self.gx[l].view(torch.uint8), self.gy[l].view(torch.uint8)]
                if self.packed:
                    parts.append(self.index_ptrs[l].view(torch.uint8))
            flat = self._flat_tables = torch.cat(parts)
        return flat

    def clone_tables(self) -> "DeviceSlideBatch":
        """The same batch with PRIVATE copies of the table tensors (a recorded launch tape addresses these, and re-points them at
        other batches: paths_amd.utils.TapedRecursion.rebind); the slides themselves are shared.  The copies are views of one flat
        buffer laid out like :meth:`flat_tables`."""
        c = object.__new__(DeviceSlideBatch)
        c.__dict__.update(self.__dict__)
        flat = self.flat_tables().clone()
        B = len(self.slides)
        c._flat_tables = flat
        c.grid_ptrs, c.mask_ptrs, c.gx, c.gy = [], [], [], []
        c.index_ptrs = [] if self.packed else None
        off = 0
        for l in range(self.num_levels):
            c.grid_ptrs.append(flat[off:off + 8 * B].view(torch.int64)); off += 8 * B
            c.mask_ptrs.append(flat[off:off + 8 * B].view(torch.int64)); off += 8 * B
            c.gx.append(flat[off:off + 4 * B].view(torch.int32)); off += 4 * B
            c.gy.append(flat[off:off + 4 * B].view(torch.int32)); off += 4 * B
            if self.packed:
                c.index_ptrs.append(flat[off:off + 8 * B].view(torch.int64)); off += 8 * B
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

    WSI reading, tissue masking of pixels and the encoder are the caller's.  Inference only."""

    on_demand = True
    host_resident = False

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

    @staticmethod
    def from_slide(slide) -> "OnDemandSlide":
        """A :class:`DeviceSlide` or :class:`HostSlide` behind the on-demand interface: ``encode`` indexes its grids (a preprocessed
        cohort replayed through this path; the twin of the tests and of tools/on_demand_time.py)."""
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

        s = OnDemandSlide([slide.shape(l) for l in range(slide.num_levels)], encode, slide.dim, dev, patch_size=slide.patch_size,
                          dtype=slide.dtype, slide_id=slide.slide_id, subtype=slide.subtype)
        if hasattr(slide, "synthetic_spec"):
            s.synthetic_spec = slide.synthetic_spec
        return s


class OnDemandSlideBatch:
    """The batch type of :class:`OnDemandSlide`, beside :class:`DeviceSlideBatch`: the static per-level tables come from the shapes
    (``gx`` / ``gy`` / ``max_dim`` / ``n0`` / ``dim`` / ``dtype``); what a resident batch knows up front and this one cannot - the rows'
    addresses (``grid_ptrs[l]``: per slide, the first of the rows supplied for level ``l``) and max|x| (``feat_absmax``, of the rows
    supplied so far) - is per-pass state, filled by :meth:`supply` as the recursion goes (paths_amd/utils.py)."""

    on_demand = True
    host_resident = False

    def __init__(self, slides):
        assert len(slides) > 0
        self.slides = list(slides)
        if not all(getattr(s, "on_demand", False) for s in self.slides):
            raise ValueError("OnDemandSlideBatch: slides of one batch are all on-demand (OnDemandSlide); resident and host-resident "
                             "slides go into a DeviceSlideBatch")
        dev = self.slides[0].device
        if dev.type != "cuda":
            raise _lib.PathsHipError("paths_amd runs on the GPU only: the slides of a batch live on a GPU device (no CPU fallback)")
        if any(s.device != dev for s in self.slides):
            raise ValueError("OnDemandSlideBatch: slides of one batch live on one device")
        L = min(s.num_levels for s in self.slides)
        self.device, self.num_levels = dev, L
        self.dim = self.slides[0].dim
        if any(s.dim != self.dim for s in self.slides):
            raise ValueError("OnDemandSlideBatch: slides of one batch share the feature width")
        self.dtype = self.slides[0].dtype
        if any(s.dtype != self.dtype for s in self.slides):
            raise ValueError("OnDemandSlideBatch: slides of one batch must share the feature dtype (got "
                             + ", ".join(sorted({str(s.dtype) for s in self.slides})) + ")")

        def table(k):
            return [torch.tensor([s.shape(l)[k] for s in self.slides], device=dev, dtype=torch.int32) for l in range(L)]

        self.gx, self.gy = table(0), table(1)
        self.n0 = max(s.shape(0)[0] * s.shape(0)[1] for s in self.slides)
        self.max_dim = [max(max(s.shape(l)) for s in self.slides) for l in range(L)]
        # level 0 asks for every cell, row-major (reference data_utils/slide.py:257-269): the request tensors are built once
        self.cells0 = [torch.cartesian_prod(torch.arange(s.shape(0)[0], device=dev), torch.arange(s.shape(0)[1], device=dev)).reshape(-1, 2)
                       for s in self.slides]
        self._host = torch.empty((len(self.slides) + 1,), dtype=torch.int64).pin_memory()      # one read-back per level: num_out | max|x| bits
        self.begin_pass()

    def __len__(self):
        return len(self.slides)

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
        stream: the encoder's work is ordered before whatever the caller launches there next."""
        B, D = len(self.slides), self.dim
        buf = torch.empty((B, cap, D), dtype=self.dtype, device=self.device)
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


def slide_batch(slides):
    """The batch of a list of slides: an :class:`OnDemandSlideBatch` for :class:`OnDemandSlide`s, else a :class:`DeviceSlideBatch`
    (which refuses a mix); a batch passes through."""
    if isinstance(slides, (DeviceSlideBatch, OnDemandSlideBatch)):
        return slides
    slides = list(slides)
    if slides and all(getattr(s, "on_demand", False) for s in slides):
        return OnDemandSlideBatch(slides)
    return DeviceSlideBatch(slides)
