"""NumPy restatement of the overlay kernels (include/paths_hip.h: paths_render_range / paths_render_rgb; paths_amd.heatmap.render) as
plain array code: the value raster from tests/raster_ref.py, the visited masks from the hierarchy, then range, colour index, table,
blend and outline.  Deliberately independent of paths_amd.heatmap and paths_amd.colormaps.

A hierarchy is tests/raster_ref.py's: a list of L levels ``{"locs": [n, 2], "values": [n]}`` of ONE slide with level-0 grid
``base_grid``; f = 2**(L-1); an image is uint8 [X0 f c, Y0 f c, 3] for ``cell_px`` c."""
import numpy as np

from tests import raster_ref as R


def bwr():
    """blue -> white -> red as paths_amd/colormaps.py's docstring defines it."""
    table = np.zeros((256, 3), np.uint8)
    for k in range(256):
        table[k] = (k * 255 // 127, k * 255 // 127, 255) if k <= 127 else (255, (255 - k) * 255 // 127, (255 - k) * 255 // 127)
    return table


def visited_masks(levels, base_grid, patch_size=256):
    """bool [L, X0 f, Y0 f]: finest cells under a patch level l visited."""
    L = len(levels)
    f = 1 << (L - 1)
    x, y = np.meshgrid(np.arange(base_grid[0] * f), np.arange(base_grid[1] * f), indexing="ij")
    out = np.zeros((L,) + x.shape, dtype=bool)
    for l, lv in enumerate(levels):
        s = L - 1 - l
        index, _ = R.index_grid(lv["locs"], (base_grid[0] << l, base_grid[1] << l), patch_size)
        out[l] = index[x >> s, y >> s] >= 0
    return out


def value_range(value, visited, center=None):
    """(vmin, vmax) in float64 over the visited cells with a finite value; (0, 0) without one."""
    v = np.asarray(value, np.float64)[visited & np.isfinite(value)]
    if v.size == 0:
        return 0.0, 0.0
    if center is None:
        return float(v.min() + 0.0), float(v.max() + 0.0)                    # (+ 0.0: a -0 extreme reads +0)
    z = np.float64(center)
    m = np.abs(v - z).max()
    return float(z - m), float(z + m)


def colour_index(value, vmin, vmax):
    """k = clamp(int((value - vmin) / (vmax - vmin) * 256.0), 0, 255) in float64; 0 where vmax == vmin."""
    v = np.asarray(value, np.float64)
    if vmax == vmin:
        return np.zeros(v.shape, np.int64)
    with np.errstate(all="ignore"):
        t256 = (v - np.float64(vmin)) / (np.float64(vmax) - np.float64(vmin)) * np.float64(256.0)
    t256 = np.where(np.isnan(t256), 0.0, t256)
    return np.clip(np.trunc(np.clip(t256, -1.0, 256.0)), 0, 255).astype(np.int64)


def compose(value, visited, drawn, cell_px, table, alpha=0.5, vmin=None, vmax=None, center=None, outline=(), outline_rgb=(0, 0, 0),
            background=(255, 255, 255), thumbnail=None):
    """value [X, Y] (values outside the visited cells are not looked at), visited bool [L, X, Y], drawn: the levels whose union is the
    visited set of the picture.  Returns (image, (vmin, vmax), a visited cell held a non-finite value)."""
    L, X, Y = visited.shape
    c = int(cell_px)
    named = visited[list(drawn)].any(axis=0)
    value = np.where(named, np.asarray(value, np.float64), 0.0)
    finite = np.isfinite(value)
    bad = bool((named & ~finite).any())
    vis = named & finite
    lo, hi = value_range(value, vis, center)
    lo = lo if vmin is None else float(vmin)
    hi = hi if vmax is None else float(vmax)
    k = colour_index(np.where(vis, value, lo), lo, hi)
    up = lambda a: np.repeat(np.repeat(a, c, axis=0), c, axis=1)
    colour = up(np.asarray(table, np.uint8)[k]).astype(np.int64)                                  # [X c, Y c, 3]
    under = (np.broadcast_to(np.asarray(background, np.int64), (X * c, Y * c, 3)) if thumbnail is None
             else np.asarray(thumbnail).astype(np.int64))
    assert under.shape == (X * c, Y * c, 3)
    a = int(round(float(alpha) * 255))
    image = np.where(up(vis)[..., None], (a * colour + (255 - a) * under + 127) // 255, under)
    u, v = np.meshgrid(np.arange(X * c), np.arange(Y * c), indexing="ij")
    for l in sorted(set(outline)):
        s = c << (L - 1 - l)
        if s < 4:
            continue
        edge = (np.minimum(u % s, v % s) == 0) | (np.maximum(u % s, v % s) == s - 1)
        image = np.where((up(visited[l]) & edge)[..., None], np.asarray(outline_rgb, np.int64), image)
    return image.astype(np.uint8), (lo, hi), bad


def render(levels, base_grid, level=None, fold=0.5, offset=0.0, dtype=np.float32, patch_size=256, outline=None, **kw):
    """The picture of one slide: the folded map (``level`` None, weight ``fold``) or plane ``level`` of tests/raster_ref.py's raster in
    ``dtype``; ``outline`` None = all levels.  Returns compose()'s triple."""
    L = len(levels)
    visited = visited_masks(levels, base_grid, patch_size)
    if level is None:
        value, drawn = R.raster(levels, base_grid, offset=offset, fold=fold, patch_size=patch_size, dtype=dtype), range(L)
    else:
        value, drawn = R.raster(levels, base_grid, offset=offset, patch_size=patch_size, dtype=dtype)[level], [level]
    return compose(value, visited, drawn, outline=range(L) if outline is None else outline, **kw)
