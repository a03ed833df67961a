"""From decoded pixels to encoder input on the device, and back to the feature rows an on-demand slide hands the recursion
(csrc/tiles.hip; include/paths_hip.h: paths_grey_histogram .. paths_scatter_rows; the contract is tests/tiles_ref.py, bit
for bit).  What the reference does in preprocess/preprocess.py:27-110 and data_utils/slide.py:80-161 (``RawSlide``) between the WSI
reader and the encoder, stated once:

grey      ``g = (4899 R + 9617 G + 1868 B + 8192) >> 14``: OpenCV's 8-bit RGB2GRAY, which the reference reaches through tiatoolbox's
          ``OtsuTissueMasker``;
threshold :func:`otsu_from_histogram` over ONE 256-bin histogram of all images given to the fit, jointly (:func:`grey_histogram`);
tissue    a pixel is tissue when ``g < t`` (strict: the reference's own quirk); a tile is tissue when ``count / size >
          tissue_threshold`` in float64 over the lattice ``(i s + s // 2, j s + s // 2)``, ``s = stride`` (:func:`tile_tissue`;
          :func:`passing_count` turns the comparison into the smallest passing integer once, the kernel compares integers);
input     ``[m, 3, P, P]`` for the tissue tiles in request order, ``table[c][v]`` for byte ``v`` of channel ``c``
          (:func:`encoder_input`; :func:`to_tensor_table` is ``to_tensor``, :func:`normalize_table` is ``to_tensor`` followed by
          ``Normalize``, both built here with torch, so the kernel's result is torch's by construction);
resize    with ``resize=S`` (and ``crop=C``, default ``S``) the input is ``[m, 3, C, C]``: the tile's BYTES resized to ``S x S`` as Pillow
          resizes an 8-bit image (antialiased bicubic or bilinear, integer coefficients, a byte image between the horizontal and the
          vertical pass), the centre ``C x C`` of it (torchvision's ``CenterCrop``), then the same table - what ``Resize(S)`` ->
          ``CenterCrop(C)`` -> ``ToTensor`` -> ``Normalize`` of timm's and torchvision's transforms give for the decoded tile, byte for
          byte (csrc/tile_resize.hip; :func:`resize_coefficients`, :func:`crop_offset`; the contract is tests/resize_ref.py);
rows      ``[n, dim]`` in the slide's dtype: the encoder's row of a tissue tile, all +0.0 for every other tile
          (:func:`scatter_rows`).

Images are uint8 ``[rows, cols, 3]`` RGB in the orientation of ``heatmap.render``'s thumbnails: axis 0 is the grid's X, cell
``(x, y)`` of a level covers rows ``x P .. x P + P - 1`` and columns ``y P .. y P + P - 1``.  Tiles are a uint8 ``[n, P, P, 3]``
device tensor or a pair ``(addresses, stride)`` - int64 ``[n]`` device addresses of the tiles' first bytes and their row stride in
bytes - so a decoder's batch and windows into a resident level image (:class:`LevelImages`) go through the same kernels.  Addresses
and strides are multiples of 16, ``P % 16 == 0``, ``16 <= P <= 1024``, ``n <= 65,536``: anything else is refused (ValueError), never
approximated.

:class:`TileEncoder` puts the pieces behind the ``encode(level, cells)`` contract of ``OnDemandSlide`` / ``CachedOnDemandSlide``.

Out of scope: reading and decoding WSI files, any resampling (the reference's mask of a resampled low-power read belongs to the WSI
reader; here the lattice samples the tile's own pixels), resizes other than the one above (torch's own uint8 resize, which is within
one byte of it; a float resize; non-square images; nearest, lanczos and box filters; ``RandomResizedCrop`` and every other training
augmentation: they stay inside the caller's ``model``), the encoder network, ``RawSlide``'s per-load joint fit and its
halve-the-threshold fallback, tiles in pinned host memory, training."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .data_utils.slide import check_grid_dtype

MAX_TILES = 65536            # include/paths_hip.h: PATHS_TILES_MAX
MAX_PATCH = 1024             # PATHS_TILE_MAX_P
MAX_IMAGES = 1024            # PATHS_HIST_MAX_IMAGES
MAX_RESIZE = 1024           # PATHS_RESIZE_MAX
MAX_TAPS = 17                # PATHS_RESIZE_MAX_TAPS
INPUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
INTERPOLATIONS = {"bicubic": 2.0, "bilinear": 1.0}       # the filters' supports

Tissue = namedtuple("Tissue", "counts flags order m slots tiles")


class _Tiles:
    """Checked tiles: ``n`` tiles of ``P`` pixels, rows ``stride`` bytes apart; :meth:`table` builds the device table [n][2], once."""

    def __init__(self, n, P, stride, step, addresses, keep):
        self.n, self.P, self.stride, self.step, self.addresses, self.keep = n, P, stride, step, addresses, keep
        self._table = None

    def table(self) -> torch.Tensor:
        if self._table is None:
            self._table = self._build()
        return self._table

    def _build(self) -> torch.Tensor:
        _lib.require_cuda(self.keep)
        self.device = self.keep.device
        with torch.cuda.device(self.device):
            a = self.addresses
            if a is None:
                a = torch.arange(self.n, dtype=torch.int64, device=self.device) * self.step + self.keep.data_ptr()
            return torch.stack([a, torch.full_like(a, self.stride)], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------
# host side: threshold, passing count, tables
# ------------------------------------------------------------------------------------------------
def otsu_from_histogram(counts) -> int:
    """Otsu's threshold of a 256-bin histogram: with ``gmin`` / ``gmax`` the occupied extremes, the first ``t`` in ``[gmin, gmax - 1]``
    that maximises ``w0 w1 (s0 / w0 - s1 / w1)^2`` for the classes ``{g <= t}`` / ``{g > t}`` (``w`` the count, ``s`` the sum of values:
    exact integers converted to float64, every operation rounded separately); ``gmin`` when ``gmin == gmax``."""
    c = [int(v) for v in (counts.cpu().tolist() if torch.is_tensor(counts) else np.asarray(counts).tolist())]
    if len(c) != 256 or any(v < 0 for v in c) or not any(c):
        raise ValueError("otsu_from_histogram: counts are 256 non-negative numbers of pixels, not all zero")
    occupied = [g for g in range(256) if c[g]]
    gmin, gmax = occupied[0], occupied[-1]
    if gmin == gmax:
        return gmin
    total, total_s = sum(c), sum(g * v for g, v in enumerate(c))
    best, best_t, w0, s0 = -1.0, gmin, 0, 0
    for t in range(gmin, gmax):
        w0 += c[t]
        s0 += t * c[t]
        w1, s1 = total - w0, total_s - s0                            # (w0 >= 1 from gmin on, w1 >= 1 up to gmax - 1)
        d = float(s0) / float(w0) - float(s1) / float(w1)
        var = float(w0) * float(w1) * (d * d)
        if var > best:
            best, best_t = var, t
    return best_t


def passing_count(size: int, tissue_threshold: float) -> int:
    """The smallest integer ``count`` in ``[0, size + 1]`` with ``count / size > tissue_threshold`` evaluated in float64 as reference
    preprocess.py:46,60 does (``size + 1``: no count passes)."""
    size, thr = int(size), float(tissue_threshold)
    if size < 1 or math.isnan(thr):
        raise ValueError(f"passing_count: size {size} must be positive and tissue_threshold a number")
    c = min(max(int(thr * size) - 1, 0), size + 1) if math.isfinite(thr) else (0 if thr < 0 else size + 1)
    while c <= size and not c / size > thr:
        c += 1
    while c > 0 and (c - 1) / size > thr:
        c -= 1
    return c


def _input_dtype(dtype) -> torch.dtype:
    if dtype not in INPUT_DTYPES:
        raise ValueError(f"the encoder input is float32, float16 or bfloat16, got {dtype}")
    return dtype


def to_tensor_table(dtype=torch.float16) -> torch.Tensor:
    """``[3, 256]`` (CPU): ``v / 255`` in fp32, then cast - what ``to_tensor`` gives for byte ``v``."""
    v = torch.arange(256, dtype=torch.float32).div(255)
    return v.expand(3, 256).to(_input_dtype(dtype)).contiguous()


def normalize_table(mean: Sequence[float], std: Sequence[float], dtype=torch.float16) -> torch.Tensor:
    """``[3, 256]`` (CPU): ``(v / 255 - mean[c]) / std[c]`` in fp32, then cast - ``to_tensor`` followed by ``Normalize(mean, std)``."""
    if len(mean) != 3 or len(std) != 3 or any(float(s) == 0 for s in std):
        raise ValueError("normalize_table: mean and std are three numbers each, no std zero")
    v = torch.arange(256, dtype=torch.float32).div(255).expand(3, 256)
    m = torch.tensor([float(x) for x in mean], dtype=torch.float32).view(3, 1)
    s = torch.tensor([float(x) for x in std], dtype=torch.float32).view(3, 1)
    return v.sub(m).div(s).to(_input_dtype(dtype)).contiguous()


def _bicubic(x: float) -> float:
    a, x = -0.5, abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def resize_coefficients(P: int, S: int, interpolation: str = "bicubic"):
    """``(bounds, coef, taps)`` (CPU): int32 ``[S, 2]`` = (lo, cnt) and int32 ``[S, taps]`` with 22 fractional bits, zero at and beyond
    ``cnt`` - Pillow's ``precompute_coeffs`` and ``normalize_coeffs_8bpc`` for one axis from ``P`` to ``S`` pixels, in Python floats.
    Output ``i`` is ``clip((2^21 + sum_t px[lo_i + t] coef_i[t]) >> 22, 0, 255)``.  Raises if a row's sum could leave int32 or a
    coefficient the kernel's 24-bit multiplier (neither happens for these filters)."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation is one of {sorted(INTERPOLATIONS)}, got {interpolation!r}")
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in (P, S)) or S > MAX_RESIZE or P > 4 * S:
        raise ValueError(f"resize_coefficients: P and S are positive integers, S <= {MAX_RESIZE}, P <= 4 S; got {P!r}, {S!r}")
    f, support = (_bicubic if interpolation == "bicubic" else _bilinear), INTERPOLATIONS[interpolation]
    scale = P / S
    fs = max(scale, 1.0)
    support = support * fs
    taps = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds, coef = [], []
    for i in range(S):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), P) - lo
        w = [f((t + lo - center + 0.5) * ss) for t in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
        if not 0 < cnt <= taps or 255 * sum(abs(v) for v in k) + (1 << 21) >= 1 << 31 or any(abs(v) >= 1 << 23 for v in k):
            raise ValueError(f"resize_coefficients: row {i} of {P} -> {S} ({interpolation}) leaves the kernel's integer range")
        bounds.append((lo, cnt))
        coef.append(k + [0] * (taps - cnt))
    return torch.tensor(bounds, dtype=torch.int32), torch.tensor(coef, dtype=torch.int32), taps


def crop_offset(S: int, C: int) -> int:
    """Where torchvision's ``CenterCrop(C)`` starts in ``S`` pixels: ``int(round((S - C) / 2.0))``, half to even, on both axes."""
    return int(round((int(S) - int(C)) / 2.0))


# ------------------------------------------------------------------------------------------------
# argument checks (all of them before any launch, none of them needs a GPU)
# ------------------------------------------------------------------------------------------------
def check_patch(patch_size, stride=None) -> int:
    P = patch_size
    if isinstance(P, bool) or not isinstance(P, int) or P % 16 != 0 or not 16 <= P <= MAX_PATCH:
        raise ValueError(f"patch_size must be a multiple of 16 in [16, {MAX_PATCH}], got {patch_size!r}")
    if stride is not None and (isinstance(stride, bool) or not isinstance(stride, int) or stride < 1 or P % stride != 0):
        raise ValueError(f"stride must be a positive integer that divides patch_size {P}, got {stride!r}")
    return P


def _check_resize(P: int, resize, crop, interpolation):
    """``(P, S, C)`` of a resize, or ValueError: what csrc/tile_resize.hip takes."""
    for name, v in (("resize", resize), ("crop", crop)):
        if isinstance(v, bool) or not isinstance(v, int) or not 16 <= v <= MAX_RESIZE:
            raise ValueError(f"{name} must be an integer in [16, {MAX_RESIZE}], got {v!r}")
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation is one of {sorted(INTERPOLATIONS)}, got {interpolation!r}")
    if isinstance(P, bool) or not isinstance(P, int) or P < 1:
        raise ValueError(f"the tile's size must be a positive integer, got {P!r}")
    if crop % 16 != 0:
        raise ValueError(f"crop must be a multiple of 16 (an output row is whole 16-byte stores), got {crop}")
    if crop > resize:
        raise ValueError(f"crop ({crop}) must not exceed resize ({resize})")
    if P > 4 * resize:
        raise ValueError(f"a {P}-pixel tile is more than 4 times resize ({resize}): at most {MAX_TAPS} taps")
    return P, resize, crop


def _resize_args(P: int, resize, crop, interpolation):
    """None without a resize, else the checked ``(S, C, interpolation)``; ``crop`` defaults to ``resize``."""
    if resize is None:
        if crop is not None:
            raise ValueError(f"crop ({crop!r}) needs resize: the centre crop follows the resize")
        if interpolation not in INTERPOLATIONS:
            raise ValueError(f"interpolation is one of {sorted(INTERPOLATIONS)}, got {interpolation!r}")
        return None
    return _check_resize(P, resize, resize if crop is None else crop, interpolation)[1:] + (interpolation,)


_resize_tables = {}


def _device_resize_tables(P: int, S: int, interpolation: str, device):
    """The device copies of :func:`resize_coefficients`, built once per shape, filter and device."""
    key = (P, S, interpolation, str(device))
    if key not in _resize_tables:
        bounds, coef, taps = resize_coefficients(P, S, interpolation)
        _resize_tables[key] = (bounds.to(device), coef.to(device), taps)
    return _resize_tables[key]


def _check_image(t, who: str):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1 \
            or tuple(t.stride()[1:]) != (3, 1):
        raise ValueError(f"{who} must be a uint8 tensor [rows, cols, 3] with last strides (3, 1), got "
                         + (f"{t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}" if torch.is_tensor(t) else type(t).__name__))
    if t.stride(0) % 16 != 0 or t.stride(0) < 3 * t.shape[1] or t.data_ptr() % 16 != 0:
        raise ValueError(f"{who}: the address and the row stride ({t.stride(0)} bytes) must be multiples of 16 (pad the rows)")
    if t.shape[0] * t.shape[1] >= 1 << 31:
        raise ValueError(f"{who}: {t.shape[0]} x {t.shape[1]} pixels are more than one image may hold (2^31)")


def _tiles(tiles, patch_size: Optional[int], who: str) -> _Tiles:
    """A batch tensor or an ``(addresses, stride)`` pair, checked: every refusal that needs no device.  Tiles that were checked
    before (``Tissue.tiles``) pass through, so a caller with several chunks of one request builds the device table once."""
    if isinstance(tiles, _Tiles):
        if patch_size is not None and int(patch_size) != tiles.P:
            raise ValueError(f"{who}: the tiles are {tiles.P} pixels wide, patch_size is {patch_size}")
        return tiles
    if torch.is_tensor(tiles):
        t = tiles
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1] != t.shape[2] or t.shape[3] != 3 or tuple(t.stride()[2:]) != (3, 1):
            raise ValueError(f"{who}: tiles must be a uint8 tensor [n, P, P, 3] with last strides (3, 1), got {t.dtype} {tuple(t.shape)} "
                             f"strides {tuple(t.stride())}")
        n, P = int(t.shape[0]), check_patch(int(t.shape[1]))
        if patch_size is not None and int(patch_size) != P:
            raise ValueError(f"{who}: the tiles are {P} pixels wide, patch_size is {patch_size}")
        stride, step, keep = int(t.stride(1)), int(t.stride(0)), t
        if t.data_ptr() % 16 != 0 or (n > 1 and step % 16 != 0):
            raise ValueError(f"{who}: the address of every tile must be a multiple of 16 (tile stride {step} bytes)")
        addresses = None
    else:
        try:
            addresses, stride = tiles
        except (TypeError, ValueError):
            raise ValueError(f"{who}: tiles are a uint8 tensor [n, P, P, 3] or a pair (addresses, stride)") from None
        if patch_size is None:
            raise ValueError(f"{who}: patch_size is required with an (addresses, stride) pair")
        P = check_patch(patch_size)
        if not torch.is_tensor(addresses) or addresses.dtype != torch.int64 or addresses.dim() != 1 or isinstance(stride, bool) \
                or not isinstance(stride, int):
            raise ValueError(f"{who}: (addresses, stride) is an int64 tensor [n] and an int")
        n, keep, step = int(addresses.shape[0]), addresses, 0
    if stride % 16 != 0 or stride < 3 * P:
        raise ValueError(f"{who}: the row stride ({stride} bytes) must be a multiple of 16 and at least {3 * P} (pad the rows)")
    if not 1 <= n <= MAX_TILES:
        raise ValueError(f"{who}: {n} tiles; one call takes 1 to {MAX_TILES}")
    return _Tiles(n, P, stride, step, addresses, keep)


# ------------------------------------------------------------------------------------------------
# the five entry points
# ------------------------------------------------------------------------------------------------
def grey_histogram(images) -> torch.Tensor:
    """int64 ``[256]`` on the device: the number of pixels of every grey value over all ``images`` jointly (uint8 ``[rows, cols, 3]``
    device tensors with last strides (3, 1); address and row stride multiples of 16).  Bit-identical on repeat; no host read."""
    images = [images] if torch.is_tensor(images) else list(images)
    if not 1 <= len(images) <= MAX_IMAGES:
        raise ValueError(f"grey_histogram: {len(images)} images; one call takes 1 to {MAX_IMAGES}")
    for i, t in enumerate(images):
        _check_image(t, f"grey_histogram: image {i}")
    _lib.require_cuda(*images)
    dev = images[0].device
    if any(t.device != dev for t in images):
        raise _lib.PathsHipError("grey_histogram: the images are on different devices")
    with torch.cuda.device(dev):
        table = torch.tensor([[t.data_ptr(), t.stride(0), t.shape[0], t.shape[1]] for t in images], dtype=torch.int64).to(dev)
        ws = int(_lib.load().paths_grey_histogram_workspace(len(images)))
        partials = torch.empty((ws // 4,), dtype=torch.int32, device=dev)
        counts = torch.empty((256,), dtype=torch.int64, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)       # (never set here: what it reports was refused above)
        _lib.call("paths_grey_histogram", table.data_ptr(), len(images), partials.data_ptr(), counts.data_ptr(), status.data_ptr(), _lib.stream())
    return counts


def otsu_threshold(images) -> int:
    """:func:`otsu_from_histogram` of :func:`grey_histogram`: one 2-KB host read."""
    return otsu_from_histogram(grey_histogram(images).cpu())


def _check_threshold(threshold) -> int:
    if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or not 0 <= int(threshold) <= 256:
        raise ValueError(f"threshold is a grey value, an integer in [0, 256], got {threshold!r}")
    return int(threshold)


def tile_tissue(tiles, threshold: int, tissue_threshold: float = 0.1, stride: int = 4, patch_size: Optional[int] = None) -> Tissue:
    """The tissue decision of ``n`` tiles: ``counts`` int32 ``[n]`` (lattice pixels with ``g < threshold``), ``flags`` uint8 ``[n]``
    (``counts / size > tissue_threshold``), ``order`` int32 ``[n]`` whose first ``m`` entries name the tissue tiles in request order,
    ``m`` (an int: the call's one host read), ``slots`` int32 ``[n]``, the position of a tile in ``order`` or -1, and ``tiles``: the
    checked tiles with their device table, which :func:`encoder_input` takes in place of the tiles themselves.  ``patch_size``
    is required with an ``(addresses, stride)`` pair.  An address in such a pair that is no multiple of 16 raises ValueError."""
    threshold = _check_threshold(threshold)
    if isinstance(tiles, _Tiles):
        check_patch(tiles.P, stride)
    elif not torch.is_tensor(tiles) and patch_size is not None:                  # (a batch tensor brings its own P: _tiles checks it)
        check_patch(patch_size, stride)
    elif torch.is_tensor(tiles) and tiles.dim() == 4:
        check_patch(int(tiles.shape[1]), stride)
    t = _tiles(tiles, patch_size, "tile_tissue")
    need = passing_count((t.P // stride) ** 2, tissue_threshold)
    table = t.table()
    with torch.cuda.device(t.device):
        counts = torch.empty((t.n,), dtype=torch.int32, device=t.device)
        flags = torch.empty((t.n,), dtype=torch.uint8, device=t.device)
        order = torch.empty((t.n,), dtype=torch.int32, device=t.device)
        slots = torch.empty((t.n,), dtype=torch.int32, device=t.device)
        m_status = torch.empty((2,), dtype=torch.int32, device=t.device)
        stream = _lib.stream()
        _lib.call("paths_tile_tissue", table.data_ptr(), t.n, t.P, stride, threshold, need, counts.data_ptr(), flags.data_ptr(), stream)
        _lib.call("paths_tile_compact", flags.data_ptr(), counts.data_ptr(), t.n, order.data_ptr(), m_status.data_ptr(), slots.data_ptr(),
                  m_status.data_ptr() + 4, stream)
        m, status = m_status.cpu().tolist()
    if status:
        raise ValueError("tile_tissue: a tile address is not a multiple of 16 (such a tile is never read: its count is -1)")
    return Tissue(counts, flags, order, int(m), slots, t)


def encoder_input(tiles, order: torch.Tensor, first: int, count: int, table: torch.Tensor, patch_size: Optional[int] = None, *,
                  resize: Optional[int] = None, crop: Optional[int] = None, interpolation: str = "bicubic") -> torch.Tensor:
    """``[count, 3, P, P]`` in ``table``'s dtype: tiles ``order[first .. first + count)`` through ``table`` (``[3, 256]`` fp32, fp16 or
    bf16 on the tiles' device).  Every element is written; entries of ``order`` outside the range are not read.

    ``resize=S``: ``[count, 3, C, C]`` instead, ``C = crop`` (default ``S``) - the tiles' bytes resized to ``S x S`` as Pillow does
    (``interpolation``: "bicubic" or "bilinear", antialiased), centre-cropped, then through ``table``; one launch, the ``P x P`` float
    tensor is never formed.  ``16 <= crop <= resize <= 1024``, ``crop % 16 == 0``, ``P <= 4 resize``."""
    if not torch.is_tensor(table) or tuple(table.shape) != (3, 256) or table.dtype not in INPUT_DTYPES or not table.is_contiguous():
        raise ValueError("encoder_input: table is a contiguous [3, 256] tensor in float32, float16 or bfloat16")
    t = _tiles(tiles, patch_size, "encoder_input")
    resized = _resize_args(t.P, resize, crop, interpolation)
    first, count = int(first), int(count)
    if not torch.is_tensor(order) or order.dtype != torch.int32 or tuple(order.shape) != (t.n,) or not order.is_contiguous():
        raise ValueError(f"encoder_input: order is a contiguous int32 tensor [{t.n}]")
    if first < 0 or count < 1 or first + count > t.n:
        raise ValueError(f"encoder_input: [first, first + count) = [{first}, {first + count}) is outside the {t.n} tiles")
    tiles_table = t.table()
    _lib.require_cuda(order, table)
    if order.device != t.device or table.device != t.device:
        raise _lib.PathsHipError("encoder_input: order and table must be on the tiles' device")
    with torch.cuda.device(t.device):
        if resized is not None:
            S, C, interpolation = resized
            bounds, coef, taps = _device_resize_tables(t.P, S, interpolation, t.device)
            out = torch.empty((count, 3, C, C), dtype=table.dtype, device=t.device)
            _lib.call("paths_tiles_resize_to_input", tiles_table.data_ptr(), t.n, order.data_ptr(), first, count, t.P, S, C, bounds.data_ptr(),
                      coef.data_ptr(), taps, table.data_ptr(), table.element_size(), out.data_ptr(), _lib.stream())
            return out
        out = torch.empty((count, 3, t.P, t.P), dtype=table.dtype, device=t.device)
        _lib.call("paths_tiles_to_input", tiles_table.data_ptr(), t.n, order.data_ptr(), first, count, t.P, table.data_ptr(), table.element_size(),
                  out.data_ptr(), _lib.stream())
    return out


def scatter_rows(encoded: Optional[torch.Tensor], slots: torch.Tensor, n: int, dim: int, dtype=torch.float32) -> torch.Tensor:
    """``[n, dim]`` in ``dtype`` (fp32 or fp16): row ``k`` is ``encoded[slots[k]]`` cast once where ``slots[k] >= 0``, else +0.0.
    ``encoded``: ``[m, dim]`` fp32 or fp16, or None when no tile is tissue.  Every row is written."""
    dtype = check_grid_dtype(dtype)
    n, dim = int(n), int(dim)
    if not 1 <= n <= MAX_TILES or dim < 4 or dim % 4 != 0:
        raise ValueError(f"scatter_rows: n ({n}) is 1 to {MAX_TILES} and dim ({dim}) a positive multiple of 4")
    if not torch.is_tensor(slots) or slots.dtype != torch.int32 or tuple(slots.shape) != (n,) or not slots.is_contiguous():
        raise ValueError(f"scatter_rows: slots is a contiguous int32 tensor [{n}]")
    m = 0
    if encoded is not None and int(encoded.shape[0]) > 0:
        if encoded.dim() != 2 or int(encoded.shape[1]) != dim or encoded.dtype not in (torch.float32, torch.float16) or int(encoded.shape[0]) > n:
            raise ValueError(f"scatter_rows: encoded is [m <= {n}, {dim}] in float32 or float16, got {encoded.dtype} {tuple(encoded.shape)}")
        m = int(encoded.shape[0])
    _lib.require_cuda(slots, encoded)
    with torch.cuda.device(slots.device):
        if m and (not encoded.is_contiguous() or encoded.data_ptr() % 16 != 0):
            encoded = encoded.clone(memory_format=torch.contiguous_format)
        out = torch.empty((n, dim), dtype=dtype, device=slots.device)
        _lib.call("paths_scatter_rows", encoded.data_ptr() if m else None, int(m and encoded.dtype == torch.float16), m, slots.data_ptr(), n, dim,
                  int(dtype == torch.float16), out.data_ptr(), _lib.stream())
    return out


# ------------------------------------------------------------------------------------------------
# readers and the encoder
# ------------------------------------------------------------------------------------------------
class LevelImages:
    """A reader over RESIDENT level images: ``images[l]`` is the uint8 ``[X_l P, Y_l P, 3]`` device image of level ``l`` (last strides
    (3, 1); address and row stride multiples of 16).  ``read(level, cells)`` returns the windows of the cells as an ``(addresses,
    stride)`` pair and copies nothing.  The twin of the tests and of tools/tiles_time.py."""

    def __init__(self, images, patch_size: int = 256):
        self.patch_size = check_patch(patch_size)
        self.images = list(images)
        for l, t in enumerate(self.images):
            _check_image(t, f"LevelImages: image {l}")
            if t.shape[0] % self.patch_size or t.shape[1] % self.patch_size:
                raise ValueError(f"LevelImages: image {l} is {t.shape[0]} x {t.shape[1]} pixels, no whole number of {self.patch_size}-pixel cells")

    def shape(self, level: int):
        t = self.images[level]
        return int(t.shape[0]) // self.patch_size, int(t.shape[1]) // self.patch_size

    def __call__(self, level: int, cells: torch.Tensor):
        t, P = self.images[level], self.patch_size
        c = cells.to(t.device)
        return c[:, 0] * (P * t.stride(0)) + c[:, 1] * (3 * P) + t.data_ptr(), int(t.stride(0))


class TileEncoder:
    """``encode(level, cells)`` of :class:`~paths_amd.data_utils.slide.OnDemandSlide` / ``CachedOnDemandSlide`` from pixels:
    ``read(level, cells)`` returns the cells' tiles (uint8 ``[n, P, P, 3]`` on the device, or an ``(addresses, stride)`` pair); the
    tiles with tissue (``threshold``: the grey threshold, e.g. of :meth:`fit`; ``tissue_threshold``, ``stride``: :func:`tile_tissue`)
    go through ``table`` (default :func:`to_tensor_table` in ``input_dtype``) into ``model`` in chunks of at most ``batch`` tiles,
    under ``torch.no_grad()``; ``model`` returns ``[count, dim]`` in fp32 or fp16.  The call returns ``[n, dim]`` in ``dtype``, the
    all-zero row for every tile without tissue - and for a tissue tile whose embedding is exactly zero, as in the reference.

    ``resize`` / ``crop`` / ``interpolation``: the resize and centre crop of :func:`encoder_input`; ``model`` then receives ``[count,
    3, crop, crop]`` (an encoder that wants 224: ``resize=224``).  The tissue decision still looks at the tile's own pixels; the
    device coefficient tables are built once per shape, filter and device, at the first call.

    It works on the current stream and costs one host read (of ``m``) per call; ``model`` is not called when ``m == 0``.  ``stats``
    counts, per level, the requested tiles, the tissue tiles and the model calls."""

    def __init__(self, read: Callable, model: Callable, dim: int, threshold: int, patch_size: int = 256, tissue_threshold: float = 0.1,
                 stride: int = 4, table: Optional[torch.Tensor] = None, input_dtype=torch.float16, batch: int = 256, dtype=torch.float32,
                 resize: Optional[int] = None, crop: Optional[int] = None, interpolation: str = "bicubic"):
        if not callable(read) or not callable(model):
            raise ValueError("TileEncoder: read(level, cells) and model(input) must be callable")
        self.read, self.model = read, model
        self.patch_size = check_patch(patch_size, stride)
        self.stride, self.threshold = stride, _check_threshold(threshold)
        self.tissue_threshold = float(tissue_threshold)
        passing_count((self.patch_size // stride) ** 2, self.tissue_threshold)
        self.dtype = check_grid_dtype(dtype)
        if isinstance(dim, bool) or int(dim) < 4 or int(dim) % 4 != 0:
            raise ValueError(f"TileEncoder: dim must be a positive multiple of 4 (got {dim})")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"TileEncoder: batch must be a positive integer (got {batch!r})")
        self.dim, self.batch = int(dim), batch
        if table is None:
            table = to_tensor_table(input_dtype)
        elif not torch.is_tensor(table) or tuple(table.shape) != (3, 256) or table.dtype not in INPUT_DTYPES:
            raise ValueError("TileEncoder: table is a [3, 256] tensor in float32, float16 or bfloat16")
        self.table = table.contiguous()
        resized = _resize_args(self.patch_size, resize, crop, interpolation)
        self.resize, self.crop, self.interpolation = resized if resized is not None else (None, None, interpolation)
        if resized is not None:
            resize_coefficients(self.patch_size, self.resize, interpolation)     # (the range check, before any launch)
        self.stats = {"requested": {}, "tissue": {}, "model_calls": {}}

    @classmethod
    def fit(cls, images, read: Callable, model: Callable, dim: int, **kw) -> "TileEncoder":
        """A TileEncoder whose grey threshold is Otsu's over ``images`` jointly (thumbnails of the slide, uint8 ``[rows, cols, 3]`` on
        the device): one histogram pass and one 2-KB host read, once per slide."""
        return cls(read, model, dim, otsu_threshold(images), **kw)

    def _count(self, key: str, level: int, more: int):
        self.stats[key][level] = self.stats[key].get(level, 0) + more

    def __call__(self, level: int, cells: torch.Tensor) -> torch.Tensor:
        tiles = self.read(level, cells)
        n = int(cells.shape[0])
        got = int(tiles.shape[0]) if torch.is_tensor(tiles) else int(tiles[0].shape[0]) if isinstance(tiles, (tuple, list)) and len(tiles) == 2 \
            and torch.is_tensor(tiles[0]) else -1
        if got != n:
            raise ValueError(f"TileEncoder: read(level {level}) must return the tiles of the {n} cells asked, got {got if got >= 0 else type(tiles).__name__}")
        ts = tile_tissue(tiles, self.threshold, self.tissue_threshold, self.stride, self.patch_size)
        self._count("requested", level, n)
        self._count("tissue", level, ts.m)
        self._count("model_calls", level, 0)
        dev = ts.order.device
        encoded = None
        if ts.m:
            if self.table.device != dev:
                self.table = self.table.to(dev)
            with torch.no_grad():
                for first in range(0, ts.m, self.batch):
                    count = min(self.batch, ts.m - first)
                    rows = self.model(encoder_input(ts.tiles, ts.order, first, count, self.table, resize=self.resize, crop=self.crop,
                                                    interpolation=self.interpolation))
                    self._count("model_calls", level, 1)
                    if not torch.is_tensor(rows) or tuple(rows.shape) != (count, self.dim) or rows.dtype not in (torch.float32, torch.float16) \
                            or rows.device != dev:
                        raise ValueError(f"TileEncoder: model must return [{count}, {self.dim}] rows in float32 or float16 on {dev}, got "
                                         + (f"{rows.dtype} {tuple(rows.shape)} on {rows.device}" if torch.is_tensor(rows) else type(rows).__name__))
                    if ts.m <= self.batch:
                        encoded = rows
                    else:
                        if encoded is None:
                            encoded = torch.empty((ts.m, self.dim), dtype=rows.dtype, device=dev)
                        encoded[first:first + count].copy_(rows)
        return scatter_rows(encoded, ts.slots, n, self.dim, self.dtype)
