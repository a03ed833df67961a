"""Heat-map export (the data consumed by reference heatmap_visualise.py:113-175) and the overlay drawn from it (:func:`render`, its
lines 148-181); figure layout - viewport, colour bar, annotations - is out of scope.

``hierarchy_from_trace`` pulls one slide's per-level patch locations / importances / selected indices (and, from a
``recurse(..., attention=True)`` trace, the special token's attention; from a ``recurse(..., rollout=True)`` trace, its attention
rollout; from the trace of :func:`paths_amd.saliency.input_gradients`, every patch's gradient x input and gradient norm) out of the
trace of :func:`paths_amd.utils.recurse`.

``importance_map`` rasterises the importances exactly like the reference's overlay code: every patch of depth d paints
``importance + 1e-4`` over its footprint, then deeper levels are folded upwards with weight 1/2 wherever they exist
(heatmap_visualise.py:147-171).  ``attention_map`` rasterises the special token's attention of one decoder layer (one head or
the mean over heads), one raster per level and no fold across levels; ``rollout_map`` does the same for the attention rollout,
``relevance_map`` for the gradient-weighted attention relevance (:func:`paths_amd.saliency.attention_relevance`),
``saliency_map`` for the gradient attributions and ``removed_map`` for the cells a member of
:func:`paths_amd.saliency.removal_curves` turned to background.  Rasters are in units of the FINEST level's patches (one
cell = one patch of the last level), i.e. level-0 pixel space divided by ``patch_size / 2**(L-1)``.

The functions above work on host records, one slide and one patch at a time, and define the contract.  :func:`rasterize` computes the
same rasters on the device for all slides of a trace at once, without the host copies (csrc/raster.hip; ``removed_map`` excepted).
:func:`render` turns one of them into 8-bit RGB pixels there: colour table, blend over a thumbnail, one outline per visited patch;
:func:`save_png` writes such an image with the standard library alone.
"""
from __future__ import annotations

import struct
import zlib
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .colormaps import colour_table


# per-row attributions a saliency trace may carry: input_gradients', integrated_gradients' and smooth_grad's
SALIENCY_KINDS = ("grad_x_input", "grad_norm", "integrated_gradients", "smooth_grad_x_input", "smooth_grad_sq")
# the joint ranks saliency.removal_curves leaves in its trace, per order
REMOVAL_RANKS = ("removal_rank_morf", "removal_rank_lerf")


def hierarchy_from_trace(trace: List[dict], slide: int) -> List[Dict[str, np.ndarray]]:
    out = []
    for lv in trace:
        n = int(lv["num_ims"][slide])
        d = {"locs": lv["locs"][slide, :n].cpu().numpy(), "importance": lv["importance"][slide, :n].cpu().numpy(),
             "parent_inds": lv["parent_inds"][slide, :n].cpu().numpy()}
        if "keep_idx" in lv:
            d["keep_inds"] = lv["keep_idx"][slide, : int(lv["keep_count"][slide])].cpu().numpy()
        if "attention" in lv:
            d["attention"] = lv["attention"][slide, :, :, :n].cpu().numpy()          # [L, H, n]
            d["attention_self"] = lv["attention_self"][slide].cpu().numpy()          # [L, H]
        if "rollout" in lv:
            d["rollout"] = lv["rollout"][slide, :n].cpu().numpy()                      # [n]
            d["rollout_self"] = float(lv["rollout_self"][slide])
        if "attention_relevance" in lv:
            d["attention_relevance"] = lv["attention_relevance"][slide, :n].cpu().numpy()  # [n]
            d["attention_relevance_self"] = float(lv["attention_relevance_self"][slide])
        for key in SALIENCY_KINDS + REMOVAL_RANKS:                  # (the attribution functions' and removal_curves' per-row entries)
            if key in lv:
                d[key] = lv[key][slide, :n].cpu().numpy()                              # [n]
        out.append(d)
    return out


def _paint(dst: np.ndarray, locs: np.ndarray, values, size: int, patch_size: int, offset: float = 0.0):
    """dst[footprint of patch i] = values[i] + offset; a footprint is size x size finest cells."""
    cells = locs // patch_size
    for (cx, cy), v in zip(cells, values):
        dst[cx * size:(cx + 1) * size, cy * size:(cy + 1) * size] = v + offset


def importance_map(levels: List[Dict[str, np.ndarray]], base_grid, patch_size: int = 256, magnification_factor: int = 2) -> np.ndarray:
    """[X0 * f, Y0 * f] float map, f = magnification_factor**(L-1); 0 where no patch was visited."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    overall = np.zeros((L,) + shape, dtype=np.float64)
    for depth, lv in enumerate(levels):
        size = magnification_factor ** (L - 1 - depth)                       # footprint of one patch, in finest cells
        _paint(overall[depth], lv["locs"], lv["importance"], size, patch_size, 1e-4)
    for depth in range(L - 2, -1, -1):                                        # heatmap_visualise.py:167-169
        m = overall[depth + 1] != 0
        overall[depth][m] = overall[depth][m] + overall[depth + 1][m] * 0.5
    return overall[0]


def attention_map(levels: List[Dict[str, np.ndarray]], base_grid, layer: int = -1, head: Optional[int] = None, patch_size: int = 256,
                  magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): the special token's attention on each patch of
    decoder layer ``layer``, head ``head`` (None: the mean over heads), painted over the patch's footprint; 0 where the level did
    not visit.  ``levels`` from :func:`hierarchy_from_trace` of a ``recurse(..., attention=True)`` trace."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if "attention" not in lv:
            raise KeyError("level %d carries no attention: run recurse(..., attention=True)" % depth)
        a = lv["attention"][layer]                                            # [H, n]
        w = a.mean(axis=0, dtype=np.float64) if head is None else a[head]
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], w, magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def rollout_map(levels: List[Dict[str, np.ndarray]], base_grid, patch_size: int = 256, magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): the special token's attention rollout on each
    patch, painted over the patch's footprint like :func:`attention_map`; 0 where the level did not visit, no fold across levels.
    ``levels`` from :func:`hierarchy_from_trace` of a ``recurse(..., rollout=True)`` trace."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if "rollout" not in lv:
            raise KeyError("level %d carries no rollout: run recurse(..., rollout=True)" % depth)
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], lv["rollout"], magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def relevance_map(levels: List[Dict[str, np.ndarray]], base_grid, patch_size: int = 256, magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): the special token's gradient-weighted attention
    relevance on each patch, painted over the patch's footprint like :func:`rollout_map`; 0 where the level did not visit, no fold
    across levels.  ``levels`` from :func:`hierarchy_from_trace` of a :func:`paths_amd.saliency.attention_relevance` trace."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if "attention_relevance" not in lv:
            raise KeyError("level %d carries no attention relevance: run saliency.attention_relevance" % depth)
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], lv["attention_relevance"], magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def saliency_map(levels: List[Dict[str, np.ndarray]], base_grid, kind: str = "grad_x_input", patch_size: int = 256,
                 magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): every patch's gradient x input (``kind``
    "grad_x_input", signed) or gradient norm ("grad_norm"), painted over the patch's footprint like :func:`rollout_map`; 0 where the
    level did not visit, no fold across levels.  ``levels`` from :func:`hierarchy_from_trace` of a
    :func:`paths_amd.saliency.input_gradients` trace.  The traces of :func:`paths_amd.saliency.integrated_gradients` and
    :func:`paths_amd.saliency.smooth_grad` also carry "integrated_gradients" (signed), "smooth_grad_x_input" (signed) and
    "smooth_grad_sq"."""
    if kind not in SALIENCY_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(repr(k) for k in SALIENCY_KINDS), kind))
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if kind not in lv:
            raise KeyError("level %d carries no %s: take the trace from saliency.input_gradients / integrated_gradients / smooth_grad"
                           % (depth, kind))
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], lv[kind], magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def removed_map(levels: List[Dict[str, np.ndarray]], base_grid, count: int, order: str = "morf", patch_size: int = 256,
                magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] uint8 map per level (f = magnification_factor**(L-1)): 1 over the footprint of every cell the member of
    :func:`paths_amd.saliency.removal_curves` that removes ``count`` patches (``out["counts"][s, slide]``) turned to background at
    that level - the patches of joint rank below ``count`` in ``order`` ("morf" / "lerf") -, 0 elsewhere; no fold across levels.
    ``levels`` from :func:`hierarchy_from_trace` of the trace removal_curves returns.  NumPy only: :func:`rasterize` has no form of
    this map (uint8, a predicate on the rank instead of a value)."""
    key = "removal_rank_" + order
    if key not in REMOVAL_RANKS:
        raise ValueError("order must be 'morf' or 'lerf', got %r" % (order,))
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if key not in lv:
            raise KeyError("level %d carries no %s: take the trace from saliency.removal_curves(order=%r or 'both')" % (depth, key, order))
        gone = (lv[key] >= 0) & (lv[key] < count)
        raster = np.zeros(shape, dtype=np.uint8)
        _paint(raster, lv["locs"][gone], np.ones(int(gone.sum()), np.uint8), magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


# ---- the same rasters on the device, a whole batch per call (csrc/raster.hip) ----------------------------------------

RASTER_KINDS = ("importance", "attention", "rollout", "attention_relevance") + SALIENCY_KINDS
MAX_RASTER_LEVELS = 8          # include/paths_hip.h: paths_raster_maps
_NO_KEY = {"attention": "level %d carries no attention: run recurse(..., attention=True)",
           "rollout": "level %d carries no rollout: run recurse(..., rollout=True)",
           "attention_relevance": "level %d carries no attention relevance: run saliency.attention_relevance"}


def _level0_grids(base_grids, B: int) -> List[tuple]:
    """One (X0, Y0) per slide from a list of pairs, a slide batch or a list of slides (``shape(0)``)."""
    items = list(getattr(base_grids, "slides", base_grids))
    if len(items) != B:
        raise ValueError("base_grids: %d grids for the %d slides of the trace" % (len(items), B))
    grids = [tuple(int(v) for v in (g.shape(0) if callable(getattr(g, "shape", None)) else g)) for g in items]
    if any(len(g) != 2 or g[0] < 1 or g[1] < 1 for g in grids):
        raise ValueError("base_grids: every grid is a pair of positive extents, got %r" % (grids,))
    return grids


def _raster_values(lv: dict, kind: str, layer: int, head: Optional[int]) -> torch.Tensor:
    """The [B, N] value rows of one level (last stride 1; a view where the record already holds them that way)."""
    if kind == "attention":
        a = lv["attention"]                                                   # [B, layers, H, N]
        v = a[:, layer].to(torch.float64).mean(dim=1) if head is None else a[:, layer, head]
    else:
        v = lv[kind]
    if v.dtype not in (torch.float32, torch.float64):
        v = v.to(torch.float32)
    return v if v.stride(-1) == 1 else v.contiguous()


def rasterize(trace: List[dict], base_grids, kind: str = "importance", *, layer: int = -1, head: Optional[int] = None, fold=None,
              offset: Optional[float] = None, patch_size: int = 256, magnification_factor: int = 2, dtype: torch.dtype = torch.float32,
              check: bool = True) -> List[torch.Tensor]:
    """The rasters of the functions above for every slide of ``trace`` at once, on the device: two kernels (csrc/raster.hip) instead of
    the per-slide host copies of :func:`hierarchy_from_trace` and the per-patch loop of ``_paint``.

    ``trace``: the per-level records with their device tensors as ``recurse(..., trace=[])`` (with ``attention=`` / ``rollout=``),
    ``saliency.input_gradients`` / ``integrated_gradients`` / ``smooth_grad`` / ``attention_relevance`` leave them.  ``base_grids``: one
    level-0 ``(X0, Y0)`` per slide, or the slide batch / list of slides itself.  ``kind``: "importance", "attention" (decoder layer
    ``layer``, head ``head`` or None = the mean over heads, taken in fp64), "rollout", "attention_relevance" or one of SALIENCY_KINDS.

    Returns one tensor per slide, with f = 2**(L-1):
      fold = w      ``[X0 f, Y0 f]``: ``value + offset`` per level, deeper levels folded upwards with weight w wherever they are non-zero
                    (:func:`importance_map`'s rule for any kind);
      fold = False  ``[L, X0 f, Y0 f]``: ``value + offset`` per level, 0 where the level did not visit (the ``*_map`` functions, stacked).
    Defaults: "importance" fold = 0.5, offset = 1e-4 (= :func:`importance_map`); every other kind fold = False, offset = 0 (= its
    ``*_map`` function).  ``dtype`` float64 gives the NumPy functions' values bit for bit, float32 (default) those rounded once.  The
    tensors are views, narrowed to each slide's extent, of one allocation padded to the batch's largest grid.

    ``check`` reads the kernels' status word (one host synchronise) and raises PathsHipError when a recorded location lies outside its
    slide's grid; with ``check=False`` such rows are skipped silently.  Only ``magnification_factor`` 2 exists: the recursion expands a
    patch into 2 x 2 children.  Host records stay with the NumPy functions: there is no CPU fallback here."""
    plan = _raster_plan(trace, base_grids, kind, layer, head, fold, offset, patch_size, magnification_factor, dtype)
    for lv in trace:                                       # last of the checks, so that the others can be met without a GPU
        _lib.require_cuda(lv["locs"], lv["num_ims"], lv[kind])
    run = _raster_run(trace, plan)
    if check:
        _raise_outside(int(run.status[0].item()), plan.L)
    return run.views


def _raster_plan(trace, base_grids, kind, layer, head, fold, offset, patch_size, magnification_factor, dtype) -> SimpleNamespace:
    """Every check of :func:`rasterize` that needs no device, and what they settle: L, B, grids, folded, w, off."""
    if kind not in RASTER_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(repr(k) for k in RASTER_KINDS), kind))
    if magnification_factor != 2:
        raise ValueError("rasterize: magnification_factor must be 2 (the recursion's child expansion is 2 x 2), got %r" % (magnification_factor,))
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("rasterize: dtype must be torch.float32 or torch.float64, got %r" % (dtype,))
    if isinstance(fold, bool) and fold:
        raise ValueError("rasterize: fold is a weight, False or None")
    if int(patch_size) < 1:
        raise ValueError("rasterize: patch_size must be positive, got %r" % (patch_size,))
    L = len(trace)
    if not 1 <= L <= MAX_RASTER_LEVELS:
        raise ValueError("rasterize: a trace of 1 to %d levels expected, got %d" % (MAX_RASTER_LEVELS, L))
    B = int(trace[0]["locs"].shape[0])
    for depth, lv in enumerate(trace):
        if kind not in lv:
            if kind in SALIENCY_KINDS:
                raise KeyError("level %d carries no %s: take the trace from saliency.input_gradients / integrated_gradients / smooth_grad"
                               % (depth, kind))
            raise KeyError(_NO_KEY[kind] % depth if kind in _NO_KEY else kind)
        if tuple(lv["locs"].shape) != (B, lv[kind].shape[-1], 2) or lv[kind].shape[0] != B or tuple(lv["num_ims"].shape) != (B,):
            raise ValueError("rasterize: level %d: locs %s, num_ims %s and %s %s do not describe the same [B, N] rows"
                             % (depth, tuple(lv["locs"].shape), tuple(lv["num_ims"].shape), kind, tuple(lv[kind].shape)))
    grids = _level0_grids(base_grids, B)
    if kind == "attention":
        for depth, lv in enumerate(trace):
            n_layers, n_heads = int(lv["attention"].shape[1]), int(lv["attention"].shape[2])
            if not -n_layers <= layer < n_layers:
                raise IndexError("rasterize: layer %d out of range for the %d decoder layers of level %d" % (layer, n_layers, depth))
            if head is not None and not 0 <= head < n_heads:
                raise IndexError("rasterize: head %d out of range for the %d heads of level %d" % (head, n_heads, depth))
    folded = (kind == "importance") if fold is None else fold is not False
    w = 0.5 if fold is None or fold is False else float(fold)
    off = (1e-4 if kind == "importance" else 0.0) if offset is None else float(offset)
    return SimpleNamespace(L=L, B=B, grids=grids, folded=folded, w=w, off=off, kind=kind, layer=layer, head=head, patch_size=int(patch_size),
                           dtype=dtype)


def _raise_outside(bits: int, L: int):
    if bits:
        raise _lib.PathsHipError("rasterize: level(s) %s hold a location outside their slide's grid (base_grids or patch_size do not "
                                 "belong to this trace)" % ", ".join(str(l) for l in range(L) if bits >> l & 1))


def _raster_run(trace: List[dict], plan: SimpleNamespace, more_status: int = 0) -> SimpleNamespace:
    """The launches of :func:`rasterize` (one paths_raster_index per level, one paths_raster_maps) on the current stream of the trace's
    device; the status word is read by the caller.  ``more_status``: further zeroed int32 words behind it, for the caller's own kernels."""
    L, B, grids, folded, w, off, kind, dtype, patch_size = (plan.L, plan.B, plan.grids, plan.folded, plan.w, plan.off, plan.kind, plan.dtype,
                                                            plan.patch_size)
    layer, head = plan.layer, plan.head
    dev = trace[0]["locs"].device
    f = 1 << (L - 1)
    GX, GY = max(g[0] for g in grids), max(g[1] for g in grids)
    with torch.cuda.device(dev):
        locs = [lv["locs"].to(torch.int64).contiguous() for lv in trace]                      # (no copies for a trace's own tensors)
        num_ims = [lv["num_ims"].to(torch.int64).contiguous() for lv in trace]
        values = [_raster_values(lv, kind, layer, head) for lv in trace]
        if len({v.dtype for v in values}) > 1:
            values = [v.to(torch.float64) for v in values]
        # index grids of all levels in one allocation, filled with -1 once; rows padded to four cells (16-byte loads at the finest level)
        ldi = [((GY << l) + 3) // 4 * 4 for l in range(L)]
        sizes = [B * (GX << l) * ldi[l] for l in range(L)]
        index = torch.full((sum(sizes),), -1, dtype=torch.int32, device=dev)
        status = torch.zeros((1 + more_status,), dtype=torch.int32, device=dev)
        ldo = (GY * f + 3) // 4 * 4
        out = torch.empty((B, GX * f, ldo) if folded else (B, L, GX * f, ldo), dtype=dtype, device=dev)
        # one host -> device copy: the per-level table, (offset, w) and the level-0 extents
        host = np.zeros(4 * L + 2 + B, dtype=np.int64)
        at = index.data_ptr()
        for l in range(L):
            host[4 * l:4 * l + 4] = (at, ldi[l], values[l].data_ptr(), values[l].stride(0))
            at += 4 * sizes[l]
        host[4 * L:4 * L + 2].view(np.float64)[:] = (off, w)
        host[4 * L + 2:].view(np.int32)[:B] = [g[0] for g in grids]
        host[4 * L + 2:].view(np.int32)[B:2 * B] = [g[1] for g in grids]
        tables = torch.from_numpy(host).to(dev)
        p_table = tables.data_ptr()
        p_offw, p_gx = p_table + 8 * 4 * L, p_table + 8 * (4 * L + 2)
        p_gy = p_gx + 4 * B
        stream = _lib.stream()
        for l in range(L):
            _lib.call("paths_raster_index", locs[l].data_ptr(), num_ims[l].data_ptr(), p_gx, p_gy, l, int(patch_size), int(locs[l].shape[1]), B,
                      GX, GY, int(host[4 * l]), ldi[l], status.data_ptr(), stream)
        _lib.call("paths_raster_maps", p_table, p_gx, p_gy, L, B, GX, GY, int(values[0].dtype == torch.float64), int(dtype == torch.float64),
                  int(folded), p_offw, out.data_ptr(), ldo, stream)
    views = [out[b, :g[0] * f, :g[1] * f] if folded else out[b, :, :g[0] * f, :g[1] * f] for b, g in enumerate(grids)]
    # (tables and index stay referenced: a caller's further kernels read them through p_table)
    return SimpleNamespace(views=views, out=out, status=status, tables=tables, index=index, p_table=p_table, p_gx=p_gx, p_gy=p_gy, GX=GX, GY=GY,
                           ldo=ldo, dev=dev)


# ---- the overlay: a raster as pixels (csrc/raster.hip: paths_render_range / paths_render_rgb) ---------------------------

MAX_CELL_PX = 64               # include/paths_hip.h: paths_render_rgb
MIN_OUTLINED_SPAN = 4          # a cell narrower than this many pixels gets no outline: it would be all outline


def _rgb_word(rgb, name: str) -> int:
    c = tuple(int(v) for v in rgb)
    if len(c) != 3 or any(not 0 <= v <= 255 for v in c):
        raise ValueError("render: %s is three integers in [0, 255], got %r" % (name, rgb))
    return c[0] | c[1] << 8 | c[2] << 16


def _per_slide(v, B: int, name: str) -> np.ndarray:
    a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
        raise ValueError("render: %s is a scalar or one value per slide (%d), got shape %r" % (name, B, tuple(a.shape)))
    if not np.isfinite(a).all():
        raise ValueError("render: %s must be finite" % name)
    return np.broadcast_to(a, (B,))


def render(trace: List[dict], base_grids, kind: str = "importance", *, level: Optional[int] = None, layer: int = -1, head: Optional[int] = None,
           fold=None, offset: Optional[float] = None, thumbnails=None, cell_px: int = 4, cmap="viridis", alpha: float = 0.5, vmin=None,
           vmax=None, center: Optional[float] = None, outline=True, outline_rgb=(0, 0, 0), background=(255, 255, 255), patch_size: int = 256,
           dtype: torch.dtype = torch.float32, check: bool = True) -> List[torch.Tensor]:
    """One uint8 RGB overlay ``[X0 f c, Y0 f c, 3]`` per slide of ``trace``, on the device (f = 2**(L-1), c = ``cell_px`` in 1..64): the
    picture reference heatmap_visualise.py:148-181 draws - the map through a colour table, at ``alpha`` over the slide where a patch was
    visited, one rectangle per visited patch and level.  The first axis is the locations' first coordinate, as in the rasters; pixel
    (u, v) shows finest cell (u // c, v // c).

    ``trace``, ``base_grids``, ``kind``, ``layer``, ``head``, ``offset``, ``patch_size``, ``dtype``: as in :func:`rasterize`, whose
    launches compute the drawn VALUE: with ``level=None`` the folded map ``rasterize(..., fold=w)``, w = ``fold`` (0.5 by default, for
    every kind); with ``level=l`` plane l of ``rasterize(..., fold=False)`` (``fold`` must then stay None).

    VISITED is a finest cell on which an index grid of a drawn level names a row (all levels for the folded map - a deeper cell without
    a level-0 parent counts, as in :func:`importance_map` -, else level l alone), never ``value != 0``.

    RANGE, per slide: ``vmin`` / ``vmax`` where given (a scalar or one value per slide); else with ``center=None`` the minimum / maximum of
    the value over the slide's visited cells (for the folded importance map the reference's rule: zeros filled with the smallest positive
    value, then autoscaled), with ``center=z`` ``z -+ max |value - z|`` (the signed kinds under a diverging table); 0, 0 for a slide
    without a visited cell.  A non-finite value on a visited cell is left out of the range and drawn as not visited; with ``check`` it
    raises PathsHipError naming the slides (the same synchronise reads :func:`rasterize`'s status), with ``check=False`` nothing more.

    COLOUR, in fp64 (fp32 values convert exactly): ``t256 = (value - vmin) / (vmax - vmin) * 256.0``, ``k = clamp(int(t256), 0, 255)``,
    k = 0 when ``vmax == vmin``; ``cmap``: "viridis", "bwr" (:mod:`paths_amd.colormaps`) or a uint8 ``[256, 3]`` array / tensor.
    BLEND, in integers: ``a = round(alpha * 255)``; a visited pixel is ``(a * colour + (255 - a) * under + 127) // 255`` per channel, any
    other pixel ``under``: the pixel of ``thumbnails[b]`` (uint8 device tensors ``[X0 f c, Y0 f c, 3]``, last strides (3, 1), any row
    stride) or ``background``.  OUTLINE: True (all levels), a sequence of levels, or False.  A cell of level l spans
    ``s = c << (L-1-l)`` pixels; where s >= 4, every pixel (u, v) inside a cell that level visited takes ``outline_rgb``, opaque and last,
    when ``min(u % s, v % s) == 0 or max(u % s, v % s) == s - 1``.

    Departures from the reference's drawing: nearest-neighbour pixels instead of a resampled image; integer blending; one-pixel outlines
    instead of anti-aliased half-point lines; no viewport crop or colour bar, which stay with whoever lays out the figure (annotation
    polygons are drawn on the returned images by :func:`paths_amd.annotations.draw`).  The tensors are views, narrowed to each slide's extent, of one allocation padded to the batch's largest grid with every row
    starting 16-byte aligned; bytes outside the slides' extents are 0.  No CPU fallback."""
    if level is not None and fold is not None:
        raise ValueError("render: fold is the weight of the folded map (level=None); a single level has none")
    if isinstance(fold, bool):
        raise ValueError("render: fold is a weight or None")
    plan = _raster_plan(trace, base_grids, kind, layer, head, False if level is not None else (0.5 if fold is None else fold), offset, patch_size,
                        2, dtype)
    L, B, grids = plan.L, plan.B, plan.grids
    if level is not None and (isinstance(level, bool) or not 0 <= int(level) < L):
        raise ValueError("render: level %r out of range for a trace of %d levels" % (level, L))
    if isinstance(cell_px, bool) or int(cell_px) != cell_px or not 1 <= int(cell_px) <= MAX_CELL_PX:
        raise ValueError("render: cell_px is an integer in [1, %d], got %r" % (MAX_CELL_PX, cell_px))
    c = int(cell_px)
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("render: alpha must lie in [0, 1], got %r" % (alpha,))
    a255 = int(round(float(alpha) * 255))
    colours = colour_table(cmap)                                         # uint8 [256, 3], or ValueError
    words = colours[:, 0].astype(np.uint32) | colours[:, 1].astype(np.uint32) << 8 | colours[:, 2].astype(np.uint32) << 16
    line, back = _rgb_word(outline_rgb, "outline_rgb"), _rgb_word(background, "background")
    if outline is True:
        outlined = list(range(L))
    elif outline is False or outline is None:
        outlined = []
    else:
        outlined = [int(l) for l in outline]
        if any(not 0 <= l < L for l in outlined):
            raise ValueError("render: outline names level(s) %s, the trace has levels 0 to %d" % ([l for l in outlined if not 0 <= l < L], L - 1))
    outline_bits = sum(1 << l for l in set(outlined) if c << (L - 1 - l) >= MIN_OUTLINED_SPAN)
    given = [None if v is None else _per_slide(v, B, name) for v, name in ((vmin, "vmin"), (vmax, "vmax"))]
    if center is not None and not np.isfinite(float(center)):
        raise ValueError("render: center must be finite, got %r" % (center,))
    f = 1 << (L - 1)
    if thumbnails is not None:
        thumbnails = list(thumbnails)
        if len(thumbnails) != B:
            raise ValueError("render: %d thumbnails for the %d slides of the trace" % (len(thumbnails), B))
        for b, (t, g) in enumerate(zip(thumbnails, grids)):
            want = (g[0] * f * c, g[1] * f * c, 3)
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != want or tuple(t.stride()[1:]) != (3, 1):
                raise ValueError("render: thumbnail %d must be a uint8 tensor %r with last strides (3, 1), got %s" % (
                    b, want, "%s %r strides %r" % (t.dtype, tuple(t.shape), tuple(t.stride())) if torch.is_tensor(t) else type(t).__name__))
    for lv in trace:                                       # last of the checks, so that the others can be met without a GPU
        _lib.require_cuda(lv["locs"], lv["num_ims"], lv[kind])
    if thumbnails is not None:
        _lib.require_cuda(*thumbnails)
        if any(t.device != trace[0]["locs"].device for t in thumbnails):
            raise _lib.PathsHipError("render: the thumbnails are not on the trace's device")

    run = _raster_run(trace, plan, more_status=B)
    dev, GX, GY = run.dev, run.GX, run.GY
    lvl = -1 if level is None else int(level)
    f64 = int(plan.dtype == torch.float64)
    with torch.cuda.device(dev):
        ldp = (GY * f * c * 3 + 15) // 16 * 16
        out = torch.empty((B, GX * f * c, ldp), dtype=torch.uint8, device=dev)
        # one host -> device copy: thumbnails [B][2], the colour words, the centre, the given range [B][2]
        host = np.zeros(2 * B + 128 + 1 + 2 * B, dtype=np.int64)
        if thumbnails is not None:
            host[:2 * B] = [v for t in thumbnails for v in (t.data_ptr(), t.stride(0))]
        host[2 * B:2 * B + 128].view(np.uint32)[:] = words
        host[2 * B + 128:2 * B + 129].view(np.float64)[:] = 0.0 if center is None else float(center)
        for j in (0, 1):
            if given[j] is not None:
                host[2 * B + 129:].view(np.float64)[j::2] = given[j]
        table = torch.from_numpy(host).to(dev)
        p_thumbs = table.data_ptr() if thumbnails is not None else None
        p_colours, p_center = table.data_ptr() + 8 * 2 * B, table.data_ptr() + 8 * (2 * B + 128)
        asked = table[2 * B + 129:].view(torch.float64).view(B, 2)
        stream = _lib.stream()
        if check or given[0] is None or given[1] is None:
            rng = torch.empty((B, 2), dtype=torch.float64, device=dev)
            partial = torch.empty((B * 64 * 3,), dtype=torch.float64, device=dev)
            _lib.call("paths_render_range", run.p_table, run.p_gx, run.p_gy, L, B, GX, GY, lvl, run.out.data_ptr(), f64, run.ldo,
                      p_center if center is not None else None, partial.data_ptr(), rng.data_ptr(), run.status.data_ptr() + 4, stream)
            for j in (0, 1):
                if given[j] is not None:
                    rng[:, j] = asked[:, j]
        else:
            rng = asked
        _lib.call("paths_render_rgb", run.p_table, run.p_gx, run.p_gy, L, B, GX, GY, lvl, run.out.data_ptr(), f64, run.ldo, rng.data_ptr(),
                  p_colours, p_thumbs, c, a255, outline_bits, line, back, out.data_ptr(), ldp, stream)
        if check:
            bits = run.status.cpu().tolist()
            _raise_outside(bits[0], L)
            if any(bits[1:]):
                raise _lib.PathsHipError("render: slide(s) %s hold a non-finite %s on a visited cell" % (
                    ", ".join(str(b) for b in range(B) if bits[1 + b]), kind))
    return [out[b, :g[0] * f * c, :g[1] * f * c * 3].unflatten(-1, (g[1] * f * c, 3)) for b, g in enumerate(grids)]


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def save_png(path, image) -> None:
    """Write a uint8 ``[H, W, 3]`` image - a device tensor (one ``.cpu()``) or a NumPy array - as an 8-bit RGB PNG: filter type 0 on every
    row, one IDAT chunk from ``zlib.compress``.  Standard library only, so that a :func:`render` result can be looked at anywhere."""
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("save_png: a uint8 [H, W, 3] image expected, got %s %r" % (a.dtype, tuple(a.shape)))
    h, w = int(a.shape[0]), int(a.shape[1])
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)                       # a filter byte (0 = None) in front of every row
    rows[:, 1:] = a.reshape(h, 3 * w)
    png = (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
           _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _png_chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(png)
