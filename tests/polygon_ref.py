"""NumPy contract of the annotation kernels (csrc/polygons.hip: paths_polygon_cover / paths_polygon_outline; paths_amd/annotations.py).

Coordinates are integers with 16 fractional bits per FINEST cell, ``(row, col)`` with the row along the grid's X.  Everything here is
int64 arithmetic on them, so "equal" means bit for bit.

coverage   cell (x, y) holds how many of its s x s sample points p = ((x << 16) + o_i, (y << 16) + o_j), o_i = ((2 i + 1) << 15) >> log2 s,
           lie inside the union of the polygons.  Polygon k contains p by the even-odd rule over its edges a -> b (closed implicitly): an
           edge counts when (a.r > p.r) != (b.r > p.r) and, with d = b.r - a.r and t = (p.c - a.c) d - (p.r - a.r) (b.c - a.c), t < 0 if
           d > 0 else t > 0.
outline    an endpoint's pixel is floor(fixed * cell_px / 65536) per axis; with n = max(|du|, |dv|) the edge paints k = 0 .. n at
           (u0 + floor((2 k du + n) / (2 n)), v0 + floor((2 k dv + n) / (2 n))), for n = 0 the pixel (u0, v0); a painted pixel is the
           square of ``width`` pixels from (u - width // 2, v - width // 2), clipped to the image, in ``rgb``.
"""
import numpy as np

ONE = 1 << 16


def fixed(x, f: int, patch_size: int) -> np.ndarray:
    """Level-0 pixels -> fixed point: round_half_even(x * f / patch_size * 65536) in float64, as int64."""
    x = np.asarray(x, dtype=np.float64)
    return np.rint(x * f / patch_size * 65536.0).astype(np.int64)


def sample_offsets(s: int) -> np.ndarray:
    assert s in (1, 2, 4, 8, 16), s
    shift = s.bit_length() - 1
    return np.array([((2 * i + 1) << 15) >> shift for i in range(s)], dtype=np.int64)


def sample_points(cells: int, s: int) -> np.ndarray:
    """The ``cells * s`` sample coordinates of one axis, cell by cell."""
    return ((np.arange(cells, dtype=np.int64)[:, None] << 16) + sample_offsets(s)[None, :]).reshape(-1)


def contains(poly: np.ndarray, pr: np.ndarray, pc: np.ndarray) -> np.ndarray:
    """bool [len(pr), len(pc)]: polygon ``poly`` (int [n, 2]) contains the point (pr[i], pc[j])."""
    poly = np.asarray(poly, dtype=np.int64)
    pr, pc = np.asarray(pr, dtype=np.int64), np.asarray(pc, dtype=np.int64)
    inside = np.zeros((len(pr), len(pc)), dtype=bool)
    n = len(poly)
    for e in range(n):
        (ar, ac), (br, bc) = poly[e], poly[(e + 1) % n]
        rows = np.nonzero((ar > pr) != (br > pr))[0]
        if rows.size == 0:
            continue
        d = br - ar
        t = (pc[None, :] - ac) * d - (pr[rows, None] - ar) * (bc - ac)
        inside[rows] ^= (t < 0) if d > 0 else (t > 0)
    return inside


def coverage(polys, X: int, Y: int, s: int) -> np.ndarray:
    """int32 [X, Y]: the samples of every cell inside the union of ``polys`` (a list of int [n, 2] arrays; may be empty)."""
    pr, pc = sample_points(X, s), sample_points(Y, s)
    inside = np.zeros((X * s, Y * s), dtype=bool)
    for poly in polys:
        inside |= contains(poly, pr, pc)
    return inside.reshape(X, s, Y, s).sum(axis=(1, 3)).astype(np.int32)


def edge_pixels(a, b, cell_px: int):
    """int64 (u [n + 1], v [n + 1]): the pixels edge a -> b paints, in order."""
    u0, v0 = (int(a[0]) * cell_px) >> 16, (int(a[1]) * cell_px) >> 16
    du, dv = ((int(b[0]) * cell_px) >> 16) - u0, ((int(b[1]) * cell_px) >> 16) - v0
    n = max(abs(du), abs(dv))
    if n == 0:
        return np.array([u0], dtype=np.int64), np.array([v0], dtype=np.int64)
    k = np.arange(n + 1, dtype=np.int64)
    return u0 + (2 * k * du + n) // (2 * n), v0 + (2 * k * dv + n) // (2 * n)


def draw(image: np.ndarray, polys, cell_px: int, rgb=(0, 0, 255), width: int = 1) -> np.ndarray:
    """Paint the outlines of ``polys`` on ``image`` (uint8 [H, W, 3], the slide's own extent) in place."""
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and 1 <= width <= 7
    H, W = image.shape[:2]
    for poly in polys:
        n = len(poly)
        for e in range(n):
            u, v = edge_pixels(poly[e], poly[(e + 1) % n], cell_px)
            for i in range(width):
                for j in range(width):
                    uu, vv = u - width // 2 + i, v - width // 2 + j
                    ok = (uu >= 0) & (uu < H) & (vv >= 0) & (vv < W)
                    image[uu[ok], vv[ok]] = rgb
    return image


def step_counts(verts: np.ndarray, poly_off, cell_px: int) -> np.ndarray:
    """int64 [V]: n + 1 of the edge that starts at each vertex."""
    verts = np.asarray(verts, dtype=np.int64)
    out = np.zeros(len(verts), dtype=np.int64)
    for k in range(len(poly_off) - 1):
        v0, v1 = int(poly_off[k]), int(poly_off[k + 1])
        for e in range(v0, v1):
            out[e] = len(edge_pixels(verts[e], verts[e + 1 if e + 1 < v1 else v0], cell_px)[0])
    return out
