"""Tumour annotations on the device: polygon coverage of the finest raster, per-patch coverage and localisation scores of a recursion,
polygon outlines on a rendered overlay (csrc/polygons.hip; include/paths_hip.h: paths_polygon_cover / paths_polygon_outline; DESIGN 27;
the polygons reference heatmap_visualise.py:21-48, 123-135 loads and draws beside its heat map).

:class:`Polygons` holds the polygons of a batch of slides in FIXED POINT: a vertex ``(row, col)`` in level-0 pixels - the orientation
of ``heatmap.render``'s images, axis 0 is the grid's X, the first coordinate of ``locs`` - becomes the int32 pair
``round_half_even(x * f / patch_size * 65536)``, f = 2**(L-1), computed in float64: 16 fractional bits per cell of the FINEST level's
raster (``heatmap.rasterize``'s cells).  The conversion happens once, on the host; everything behind it is exact integer arithmetic,
stated in NumPy by tests/polygon_ref.py, and the kernels equal that bit for bit.  :func:`parse_camelyon17` reads the polygons of one
slide from a CAMELYON17 (ASAP) annotation file.

:func:`coverage` counts, per finest cell, the ``s x s`` sample points inside the union of the slide's polygons (even-odd rule within a
polygon); :func:`patch_cover` sums those counts over the footprint of every visited patch of a trace, :func:`localisation` turns them
into per-level, per-slide scores: how much of what the recursion visited and kept is tumour, how much of the tumour tissue it reached,
and how well a per-patch record (importance, attention rollout, ...) ranks tumour patches first.  :func:`draw` paints the polygons'
outlines on the images of ``heatmap.render``, in place.

What this is not: no ASAP exclusion groups (a group other than "Tumor" is refused, as in the reference), no annotation types other than
polygons, no anti-aliased lines, no filled drawing and no figure layout.  Refusals are ValueErrors, never clamps.  No CPU fallback.
"""
from __future__ import annotations

import math
import xml.etree.ElementTree as ET
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .eval import binary_auroc
from .heatmap import MAX_CELL_PX, MAX_RASTER_LEVELS, _level0_grids

FRACTION_BITS = 16             # include/paths_hip.h: fixed point of paths_polygon_cover / paths_polygon_outline
MAX_FINEST_CELLS = 8192        # per axis of a slide's finest raster
MAX_FIXED = 1 << 29            # |coordinate|: with the two bounds above every cross product stays below 2**61 (the header derives it)
MAX_VERTICES = 1 << 20         # per batch
SAMPLES = (1, 2, 4, 8, 16)
MAX_WIDTH = 7
MAX_STEPS = (1 << 31) - 256    # (edge, step) pairs of one paths_polygon_outline launch


def to_fixed(x, f: int, patch_size: int) -> np.ndarray:
    """float64 level-0 pixels -> ``round_half_even(x * f / patch_size * 65536)`` as float64 (integral, or non-finite where ``x`` is)."""
    return np.rint(np.asarray(x, dtype=np.float64) * f / patch_size * 65536.0)


def parse_camelyon17(path, base_power: float) -> List[np.ndarray]:
    """The polygons of one CAMELYON17 annotation file (ASAP XML) as float64 ``[n, 2]`` arrays of ``(row, col)`` level-0 pixels.

    The file gives ``<Coordinate Order X Y>`` in pixels of the 40x level with X horizontal; a slide whose level 0 is at ``base_power``
    magnification has ``m = base_power / 40`` of them per level-0 pixel, so a vertex is ``(Y * m, X * m)``.  Coordinates are taken in
    their ``Order``.  A ``<Group>`` whose name is not "Tumor" and an ``<Annotation>`` whose type is not "Polygon" raise ValueError."""
    root = ET.parse(path).getroot()
    for group in root.iter("Group"):
        if group.get("Name") != "Tumor":
            raise ValueError("parse_camelyon17: unexpected group name %r (only \"Tumor\" is read)" % (group.get("Name"),))
    m = float(base_power) / 40.0
    if not math.isfinite(m) or m <= 0:
        raise ValueError("parse_camelyon17: base_power must be a positive number, got %r" % (base_power,))
    polygons = []
    for annotation in root.iter("Annotation"):
        if annotation.get("Type") != "Polygon":
            raise ValueError("parse_camelyon17: unexpected annotation type %r (only \"Polygon\" is read)" % (annotation.get("Type"),))
        coords = list(annotation.iter("Coordinate"))
        if all(c.get("Order") is not None for c in coords):
            coords.sort(key=lambda c: int(c.get("Order")))
        polygons.append(np.array([(float(c.get("Y")) * m, float(c.get("X")) * m) for c in coords], dtype=np.float64).reshape(-1, 2))
    return polygons


class Polygons:
    """The annotation polygons of a batch of slides, in fixed point.

    ``per_slide[b]``: a list (possibly empty) of float64 ``[n, 2]`` vertex arrays, n >= 3, ``(row, col)`` in level-0 pixels, each closed
    implicitly.  ``base_grids``: one level-0 ``(X0, Y0)`` per slide, or the slide batch / list of slides itself.  ``num_levels``: L of
    the recursion whose finest raster the polygons are laid over.

    Refused (ValueError): a slide whose finest raster ``(X0 f, Y0 f)`` exceeds 8,192 cells on an axis; a polygon of fewer than 3
    vertices; non-finite coordinates; a vertex whose fixed-point value leaves [-2**29, 2**29]; more than 2**20 vertices.

    Host arrays: ``verts`` int32 ``[V, 2]``, ``poly_off`` int32 ``[P + 1]`` (polygon k owns vertices poly_off[k] .. poly_off[k+1] - 1),
    ``slide_poly`` int32 ``[B + 1]`` (slide b owns polygons slide_poly[b] .. slide_poly[b+1] - 1).  ``packed`` holds them and the
    slides' finest extents in one int32 array, each part starting at a multiple of four words (``pad_words`` marks the words between
    them, which nothing reads); :meth:`table` uploads it in one copy, once per device."""

    def __init__(self, per_slide, base_grids, num_levels: int, patch_size: int = 256):
        per_slide = [list(polys) for polys in per_slide]
        B = len(per_slide)
        L, patch_size = int(num_levels), int(patch_size)
        if B < 1 or B > 65535:
            raise ValueError("Polygons: 1 to 65535 slides expected, got %d" % B)
        if not 1 <= L <= MAX_RASTER_LEVELS:
            raise ValueError("Polygons: num_levels must lie in [1, %d], got %r" % (MAX_RASTER_LEVELS, num_levels))
        if patch_size < 1:
            raise ValueError("Polygons: patch_size must be positive, got %r" % (patch_size,))
        grids = _level0_grids(base_grids, B)
        f = 1 << (L - 1)
        large = [b for b, g in enumerate(grids) if max(g) * f > MAX_FINEST_CELLS]
        if large:
            raise ValueError("Polygons: the finest raster of slide(s) %s exceeds %d cells on an axis (grids %s x %d)" % (
                large, MAX_FINEST_CELLS, [grids[b] for b in large], f))
        verts, poly_off, slide_poly = [], [0], [0]
        for b, polys in enumerate(per_slide):
            for k, poly in enumerate(polys):
                a = np.asarray(poly, dtype=np.float64)
                if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 3:
                    raise ValueError("Polygons: polygon %d of slide %d must be an [n, 2] array of n >= 3 vertices, got shape %r" % (
                        k, b, tuple(a.shape)))
                if not np.isfinite(a).all():
                    raise ValueError("Polygons: polygon %d of slide %d holds a non-finite coordinate" % (k, b))
                fx = to_fixed(a, f, patch_size)
                if not (np.abs(fx) <= MAX_FIXED).all():
                    raise ValueError("Polygons: polygon %d of slide %d leaves the fixed-point range: a vertex lies more than %d finest "
                                     "cells from the origin" % (k, b, MAX_FIXED >> FRACTION_BITS))
                verts.append(fx.astype(np.int32))
                poly_off.append(poly_off[-1] + a.shape[0])
                if poly_off[-1] > MAX_VERTICES:
                    raise ValueError("Polygons: more than %d vertices in one batch" % MAX_VERTICES)
            slide_poly.append(len(poly_off) - 1)
        self.B, self.L, self.f, self.patch_size, self.grids = B, L, f, patch_size, grids
        self.verts = np.concatenate(verts).reshape(-1, 2) if verts else np.zeros((0, 2), dtype=np.int32)
        self.poly_off = np.array(poly_off, dtype=np.int32)
        self.slide_poly = np.array(slide_poly, dtype=np.int32)
        self.V, self.P = int(self.verts.shape[0]), len(poly_off) - 1
        # the vertex each edge ends at: the next one, the polygon's first behind its last
        self.next_vertex = np.arange(1, self.V + 1, dtype=np.int64)
        if self.P:
            self.next_vertex[self.poly_off[1:] - 1] = self.poly_off[:-1]
        parts = (("verts", self.verts.reshape(-1)), ("poly_off", self.poly_off), ("slide_poly", self.slide_poly),
                 ("gx", np.array([g[0] * f for g in grids], dtype=np.int32)), ("gy", np.array([g[1] * f for g in grids], dtype=np.int32)))
        self.at, words = {}, 0
        for name, a in parts:
            self.at[name] = words
            words += (a.size + 3) // 4 * 4
        self.packed = np.zeros(max(words, 4), dtype=np.int32)
        self.pad_words = np.ones(self.packed.shape, dtype=bool)
        for name, a in parts:
            self.packed[self.at[name]:self.at[name] + a.size] = a
            self.pad_words[self.at[name]:self.at[name] + a.size] = False
        self._tables = {}

    def slide_polygons(self, b: int) -> List[np.ndarray]:
        """The fixed-point polygons of slide ``b`` (views of ``verts``)."""
        return [self.verts[self.poly_off[k]:self.poly_off[k + 1]] for k in range(self.slide_poly[b], self.slide_poly[b + 1])]

    def finest(self, b: int):
        return self.grids[b][0] * self.f, self.grids[b][1] * self.f

    def table(self, device=None) -> torch.Tensor:
        """``packed`` on ``device`` (default: the current one): one host-to-device copy, at the first call per device."""
        if not torch.cuda.is_available():
            raise _lib.PathsHipError("paths_amd runs on the GPU only: no device for the polygon tables (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _lib.PathsHipError("paths_amd runs on the GPU only: got device %s (no CPU fallback)" % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._tables:
            self._tables[device] = torch.from_numpy(self.packed).to(device)
        return self._tables[device]

    def _pointers(self, table: torch.Tensor):
        p = table.data_ptr()
        return tuple(p + 4 * self.at[name] for name in ("verts", "poly_off", "slide_poly", "gx", "gy"))


def _check_polygons(polygons, who: str) -> Polygons:
    if not isinstance(polygons, Polygons):
        raise ValueError("%s: polygons must be an annotations.Polygons, got %s" % (who, type(polygons).__name__))
    return polygons


def coverage(polygons: Polygons, samples: int = 4, device=None, out: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """One int32 ``[X0 f, Y0 f]`` device tensor per slide: cell (x, y) holds how many of its ``s x s`` sample points, s = ``samples`` in
    {1, 2, 4, 8, 16}, lie inside the union of the slide's polygons.  Sample (i, j) of a cell sits at ``((2 i + 1) << 15) >> log2 s``
    (of 65536) from the cell's corner on each axis.  A polygon contains a point by the even-odd rule, evaluated exactly (a
    self-intersecting polygon has holes by parity; two overlapping polygons have none); a point on an edge belongs to one side by a
    half-open rule, so tiling polygons count every sample once.

    One launch for the batch (paths_polygon_cover), no atomics, no workspace: bit-identical on repeat.  The tensors are views, narrowed
    to each slide's extent, of one allocation ``[B, GX f, ld]`` padded to the batch's largest grid (``ld``: GY f rounded up to four);
    every element of it is written, 0 outside a slide's extent and for a slide without polygons.  ``out``: such an allocation of the
    caller's to write into.  ``device``: where to run (default: the current device)."""
    p = _check_polygons(polygons, "coverage")
    if isinstance(samples, bool) or samples not in SAMPLES:
        raise ValueError("coverage: samples must be one of %s, got %r" % (SAMPLES, samples))
    X, Y = max(g[0] for g in p.grids) * p.f, max(g[1] for g in p.grids) * p.f
    ld = (Y + 3) // 4 * 4
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (p.B, X, ld) or not out.is_contiguous():
            raise ValueError("coverage: out must be a contiguous int32 tensor %r" % ((p.B, X, ld),))
        _lib.require_cuda(out)
        device = out.device
    table = p.table(device)
    with torch.cuda.device(table.device):
        if out is None:
            out = torch.empty((p.B, X, ld), dtype=torch.int32, device=table.device)
        verts, poly_off, slide_poly, gx, gy = p._pointers(table)
        _lib.call("paths_polygon_cover", verts, p.V, poly_off, p.P, slide_poly, gx, gy, p.B, X, Y, int(samples), out.data_ptr(), ld, _lib.stream())
    return [out[b, :p.finest(b)[0], :p.finest(b)[1]] for b in range(p.B)]


def _rgb_word(rgb) -> int:
    c = tuple(int(v) for v in rgb)
    if len(c) != 3 or any(not 0 <= v <= 255 for v in c):
        raise ValueError("draw: rgb is three integers in [0, 255], got %r" % (rgb,))
    return c[0] | c[1] << 8 | c[2] << 16


def step_table(polygons: Polygons, cell_px: int) -> np.ndarray:
    """int64 ``[V + 1]``: entry e is the number of pixels the edges before edge e paint (edge e starts at vertex e); the last entry
    is the total.  An endpoint's pixel is ``floor(fixed * cell_px / 65536)``; an edge paints ``max(|du|, |dv|) + 1`` pixels."""
    pix = (polygons.verts.astype(np.int64) * int(cell_px)) >> FRACTION_BITS
    n = np.abs(pix[polygons.next_vertex] - pix).max(axis=1) if polygons.V else np.zeros(0, dtype=np.int64)
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(n + 1, dtype=np.int64)])


def draw(images: Sequence[torch.Tensor], polygons: Polygons, cell_px: int, rgb=(0, 0, 255), width: int = 1) -> List[torch.Tensor]:
    """Paint the outline of every polygon on the uint8 RGB images ``heatmap.render`` returned for the same slides (``[X0 f c, Y0 f c, 3]``
    device tensors with last strides (3, 1), any row stride; c = ``cell_px``: one pixel is 1 / c of a finest cell), IN PLACE; returns
    them.

    An endpoint's pixel is ``floor(fixed * c / 65536)`` per axis.  With ``n = max(|du|, |dv|)`` between the two endpoint pixels an edge
    paints k = 0 .. n at ``(u0 + floor((2 k du + n) / (2 n)), v0 + floor((2 k dv + n) / (2 n)))``, for n = 0 the pixel (u0, v0).  Each
    painted pixel is a ``width x width`` square (``width`` in 1..7, from ``(u - width // 2, v - width // 2)``: centred for odd widths),
    clipped to the slide's own extent, and takes ``rgb``, opaque.  No anti-aliasing, no fill.

    One launch for the batch (paths_polygon_outline), one thread per (edge, step); every writer of a byte writes the same value, so the
    result does not depend on their order.  Bytes no edge paints are neither read nor written.  Polygons whose edges would paint 2**31
    pixels or more in one call are refused."""
    p = _check_polygons(polygons, "draw")
    if isinstance(cell_px, bool) or int(cell_px) != cell_px or not 1 <= int(cell_px) <= MAX_CELL_PX:
        raise ValueError("draw: cell_px is an integer in [1, %d], got %r" % (MAX_CELL_PX, cell_px))
    if isinstance(width, bool) or int(width) != width or not 1 <= int(width) <= MAX_WIDTH:
        raise ValueError("draw: width is an integer in [1, %d], got %r" % (MAX_WIDTH, width))
    c, width, word = int(cell_px), int(width), _rgb_word(rgb)
    images = list(images)
    if len(images) != p.B:
        raise ValueError("draw: %d images for the %d slides of the polygons" % (len(images), p.B))
    for b, t in enumerate(images):
        want = (p.finest(b)[0] * c, p.finest(b)[1] * c, 3)
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != want or tuple(t.stride()[1:]) != (3, 1) or t.stride(0) < 3 * want[1]:
            raise ValueError("draw: image %d must be a uint8 tensor %r with last strides (3, 1), got %s" % (
                b, want, "%s %r strides %r" % (t.dtype, tuple(t.shape), tuple(t.stride())) if torch.is_tensor(t) else type(t).__name__))
    cum = step_table(p, c)
    steps = int(cum[-1])
    if steps >= MAX_STEPS:
        raise ValueError("draw: the edges paint %d pixels at cell_px %d, one call draws fewer than %d" % (steps, c, MAX_STEPS))
    _lib.require_cuda(*images)
    if any(t.device != images[0].device for t in images):
        raise _lib.PathsHipError("draw: the images are not on one device")
    if p.V == 0:
        return images
    table = p.table(images[0].device)
    with torch.cuda.device(table.device):
        # one host -> device copy: the images [B][2], then the step table as int32
        host = np.zeros(2 * p.B + (p.V + 2) // 2, dtype=np.int64)
        host[:2 * p.B] = [v for t in images for v in (t.data_ptr(), t.stride(0))]
        host[2 * p.B:].view(np.int32)[:p.V + 1] = cum
        call_table = torch.from_numpy(host).to(table.device)
        verts, poly_off, slide_poly, gx, gy = p._pointers(table)
        _lib.call("paths_polygon_outline", verts, p.V, poly_off, p.P, slide_poly, gx, gy, p.B, call_table.data_ptr() + 16 * p.B, steps,
                  call_table.data_ptr(), c, width, word, _lib.stream())
    return images


# ---- per-patch coverage and localisation scores: torch on the device, host arithmetic on the small arrays ---------------------------

def positive_count(total: int, threshold: float) -> int:
    """The smallest integer ``count`` in ``[0, total + 1]`` with ``count / total >= threshold`` in float64 (``total + 1``: none passes)."""
    total, thr = int(total), float(threshold)
    if total < 1 or math.isnan(thr):
        raise ValueError("positive_count: total %d must be positive and threshold a number" % total)
    c = min(max(int(thr * total) - 1, 0), total + 1) if math.isfinite(thr) else (0 if thr < 0 else total + 1)
    while c <= total and not c / total >= thr:
        c += 1
    while c > 0 and (c - 1) / total >= thr:
        c -= 1
    return c


def _check_samples(samples, who: str) -> int:
    if isinstance(samples, bool) or samples not in SAMPLES:
        raise ValueError("%s: samples must be one of %s, got %r" % (who, SAMPLES, samples))
    return int(samples)


def _pooled(cover: Sequence[torch.Tensor], L: int, who: str):
    """(grids, [P_0 .. P_{L-1}]): the level-0 grids the finest counts imply and, per level, int32 ``[B, GX << l, GY << l]`` sums of
    the counts over each cell of that level (integer 2 x 2 sum pooling from the finest level up), padded to the batch's largest grid."""
    cover = list(cover)
    if not 1 <= L <= MAX_RASTER_LEVELS:
        raise ValueError("%s: a trace of 1 to %d levels expected, got %d" % (who, MAX_RASTER_LEVELS, L))
    f = 1 << (L - 1)
    for b, t in enumerate(cover):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.shape[0] % f or t.shape[1] % f:
            raise ValueError("%s: cover[%d] must be an int32 tensor [X0 * %d, Y0 * %d] as annotations.coverage returns, got %s" % (
                who, b, f, f, "%s %r" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    if not cover:
        raise ValueError("%s: cover is empty" % who)
    grids = [(t.shape[0] // f, t.shape[1] // f) for t in cover]
    GX, GY = max(g[0] for g in grids), max(g[1] for g in grids)
    finest = torch.zeros((len(cover), GX * f, GY * f), dtype=torch.int32, device=cover[0].device)
    for b, t in enumerate(cover):
        finest[b, :t.shape[0], :t.shape[1]] = t
    levels = [finest]
    for l in range(L - 2, -1, -1):
        q = levels[0]
        levels.insert(0, q.view(q.shape[0], q.shape[1] // 2, 2, q.shape[2] // 2, 2).sum(dim=(2, 4), dtype=torch.int32))
    return grids, levels


def _patch_cover(trace, grids, levels, patch_size: int, who: str) -> List[torch.Tensor]:
    B, dev = levels[0].shape[0], levels[0].device
    if int(trace[0]["locs"].shape[0]) != B:
        raise ValueError("%s: cover holds %d slides, the trace %d" % (who, B, int(trace[0]["locs"].shape[0])))
    gx = torch.tensor([g[0] for g in grids], dtype=torch.int64, device=dev)
    gy = torch.tensor([g[1] for g in grids], dtype=torch.int64, device=dev)
    out, outside = [], []
    for l, (lv, pooled) in enumerate(zip(trace, levels)):
        locs, N = lv["locs"].to(torch.int64), int(lv["locs"].shape[1])
        valid = torch.arange(N, device=dev)[None, :] < lv["num_ims"].to(torch.int64)[:, None]
        cx = torch.div(locs[..., 0], patch_size, rounding_mode="floor")
        cy = torch.div(locs[..., 1], patch_size, rounding_mode="floor")
        ok = (cx >= 0) & (cy >= 0) & (cx < (gx << l)[:, None]) & (cy < (gy << l)[:, None])
        outside.append((valid & ~ok).any())
        use = valid & ok
        idx = torch.where(use, cx * pooled.shape[2] + cy, torch.zeros_like(cx))
        out.append(pooled.reshape(B, -1).gather(1, idx) * use.to(torch.int32))
    bits = torch.stack(outside).cpu().tolist()
    if any(bits):
        raise _lib.PathsHipError("%s: level(s) %s hold a location outside their slide's grid (cover or patch_size do not belong to this "
                                 "trace)" % (who, ", ".join(str(l) for l, bad in enumerate(bits) if bad)))
    return out


def patch_cover(trace: List[dict], cover: Sequence[torch.Tensor], samples: int, patch_size: int = 256) -> List[torch.Tensor]:
    """Per level of ``trace`` an int32 ``[B, N]`` device tensor: for every visited row the sum of the finest counts of ``cover``
    (:func:`coverage` with the same ``samples``) over the row's footprint of ``2**(L-1-l)`` squared finest cells; rows of padding hold
    0.  The total a patch of level l can reach is ``(samples << (L-1-l))**2``.  Integer 2 x 2 sum pooling and a gather, in torch, on the
    device.  A recorded location outside its slide's grid raises PathsHipError as ``heatmap.rasterize`` does (one host synchronise)."""
    _check_samples(samples, "patch_cover")
    grids, levels = _pooled(cover, len(trace), "patch_cover")
    return _patch_cover(trace, grids, levels, int(patch_size), "patch_cover")


def localisation(trace: List[dict], slides, cover: Sequence[torch.Tensor], samples: int, threshold: float = 0.5, scores: str = "importance",
                 patch_size: int = 256) -> List[List[Dict[str, object]]]:
    """``result[l][b]``, per level and slide, a dict of

      visited      the rows the level visited (``num_ims``);
      visited_pos  how many of them are POSITIVE: ``count / total >= threshold`` in float64, count from :func:`patch_cover`, total =
                   ``(samples << (L-1-l))**2`` (the comparison is turned into the smallest passing integer once, :func:`positive_count`);
      kept_pos     the positives among ``keep_idx[:keep_count]`` on a level that selects, None on one that does not;
      tissue_pos   the cells of the slide's own tissue mask at that level whose coverage is positive (any sample inside a polygon);
      recall       ``visited_pos / tissue_pos``, nan when ``tissue_pos`` is 0;
      auroc        ``eval.binary_auroc`` of ``trace[l][scores][b]`` against the positive flag over the visited rows.

    ``slides``: the slides of the trace (a list or a batch), for their tissue masks; slides whose level grids are not
    ``(X0 << l, Y0 << l)``, or which hold no masks, are refused (ValueError naming them)."""
    s = _check_samples(samples, "localisation")
    L = len(trace)
    grids, levels = _pooled(cover, L, "localisation")
    B = len(grids)
    slide_list = list(getattr(slides, "slides", slides))
    if len(slide_list) != B:
        raise ValueError("localisation: %d slides for the %d slides of cover" % (len(slide_list), B))
    odd = [b for b, sl in enumerate(slide_list) if getattr(sl, "masks", None) is None or len(sl.masks) < L
           or any(tuple(sl.masks[l].shape) != (grids[b][0] << l, grids[b][1] << l) for l in range(L))]
    if odd:
        raise ValueError("localisation: slide(s) %s do not hold tissue masks of (X0 << l, Y0 << l) cells at every level: tissue_pos is "
                         "not defined for them" % ", ".join(str(b) for b in odd))
    for l, lv in enumerate(trace):
        if scores not in lv:
            raise KeyError("localisation: level %d carries no %s" % (l, scores))
    counts = _patch_cover(trace, grids, levels, int(patch_size), "localisation")
    tissue = torch.stack([((sl.masks[l] != 0) & (levels[l][b, :grids[b][0] << l, :grids[b][1] << l] > 0)).sum()
                          for l in range(L) for b, sl in enumerate(slide_list)]).cpu().numpy().reshape(L, B)
    result = []
    for l, lv in enumerate(trace):
        need = positive_count((s << (L - 1 - l)) ** 2, threshold)
        positive = counts[l].cpu().numpy() >= need
        num = lv["num_ims"].cpu().numpy()
        values = lv[scores].detach().to(torch.float64).cpu().numpy()
        keep = (lv["keep_idx"].cpu().numpy(), lv["keep_count"].cpu().numpy()) if "keep_idx" in lv else None
        row = []
        for b in range(B):
            n = int(num[b])
            pos = positive[b, :n]
            t = int(tissue[l, b])
            row.append({"visited": n, "visited_pos": int(pos.sum()),
                        "kept_pos": None if keep is None else int(positive[b][keep[0][b, :int(keep[1][b])]].sum()),
                        "tissue_pos": t, "recall": float(pos.sum()) / t if t else float("nan"),
                        "auroc": binary_auroc(values[b, :n], pos)})
        result.append(row)
    return result
