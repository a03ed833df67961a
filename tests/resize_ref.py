"""NumPy restatement of the resize in front of the encoder (include/paths_hip.h: paths_tiles_resize_to_input; paths_amd.pixels:
resize_coefficients, crop_offset, encoder_input(resize=...)) as plain array code.  Deliberately independent of paths_amd.pixels.

It is Pillow's ``ImagingResample`` for 8-bit images - ``precompute_coeffs``, ``normalize_coeffs_8bpc``, the horizontal pass into a
BYTE image, then the vertical pass - followed by torchvision's ``CenterCrop`` and the table lookup of tests/tiles_ref.py:
what ``Resize(S, bicubic | bilinear)`` -> ``CenterCrop(C)`` -> ``ToTensor`` -> ``Normalize`` gives for a decoded square tile.
tests/test_cpu_tile_resize.py holds it to Pillow bit for bit where Pillow is installed.

A tile is uint8 [P, P, 3] RGB; coefficients are computed in Python floats (float64), every operation as written."""
import math

import numpy as np

PRECISION_BITS = 22                     # Pillow: 32 - 8 - 2
FILTERS = ("bicubic", "bilinear")


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def coefficients(P, S, interpolation="bicubic"):
    """bounds int32 [S, 2] = (lo, cnt), k int32 [S, taps], taps: one axis from P input to S output pixels."""
    f, fsupport = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}[interpolation]
    scale = P / S
    fs = max(scale, 1.0)
    support = fsupport * fs
    taps = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds, k = np.zeros((S, 2), np.int32), np.zeros((S, taps), np.int32)
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
        bounds[i] = (lo, cnt)
        for t, v in enumerate(w):
            k[i, t] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, k, taps


def one_pass(image, bounds, k):
    """One pass along axis 0: uint8 [A, ...] -> uint8 [S, ...] (int64 sums; they fit int32, see the CPU test)."""
    src = np.asarray(image).astype(np.int64)
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for i, (lo, cnt) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t in range(cnt):
            acc = acc + src[lo + t] * int(k[i, t])
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)                   # (>> of a negative int64: arithmetic)
    return out


def resize_u8(tile, S, interpolation="bicubic"):
    """uint8 [S, S, 3] from a square uint8 [P, P, 3] tile: the horizontal pass into a byte image [P, S, 3], then the vertical one."""
    tile = np.asarray(tile)
    assert tile.dtype == np.uint8 and tile.ndim == 3 and tile.shape[0] == tile.shape[1]
    bounds, k, _ = coefficients(tile.shape[0], S, interpolation)
    h = one_pass(tile.transpose(1, 0, 2), bounds, k).transpose(1, 0, 2)
    return one_pass(h, bounds, k)


def crop_offset(S, C):
    """torchvision's CenterCrop: int(round((S - C) / 2.0)), Python's round (half to even)."""
    return int(round((S - C) / 2.0))


def resized_input(tiles, order, first, count, table, S, C, interpolation="bicubic"):
    """float32 [count, 3, C, C]: table[c][byte c] of the centre crop of the resized tiles order[first .. first + count)."""
    off = crop_offset(S, C)
    out = np.empty((count, 3, C, C), np.float32)
    for q, t in enumerate(np.asarray(order)[first:first + count]):
        o = resize_u8(np.asarray(tiles)[t], S, interpolation)[off:off + C, off:off + C]
        for c in range(3):
            out[q, c] = table[c][o[..., c]]
    return out
