"""NumPy restatement of the two raster kernels (include/paths_hip.h: paths_raster_index / paths_raster_maps) as a GATHER: every finest
cell looks up, per level, the row that covers it.  Deliberately independent of paths_amd.heatmap, whose painting loops it is compared
with in tests/test_cpu_raster.py.

A hierarchy is a list of L levels, each ``{"locs": [n, 2] integer pixels, "values": [n] float32 / float64}`` for ONE slide with level-0
grid ``base_grid``; f = 2**(L-1)."""
import numpy as np


def index_grid(locs, grid, patch_size=256):
    """int32 [grid]: the row whose cell is (x, y), -1 where there is none; of two rows on one cell the later one wins; rows with a
    negative location or a cell outside ``grid`` are skipped and counted.  Returns (index, skipped)."""
    index = np.full(grid, -1, dtype=np.int32)
    skipped = 0
    for i, (px, py) in enumerate(np.asarray(locs).reshape(-1, 2).tolist()):
        cx, cy = px // patch_size, py // patch_size
        if px < 0 or py < 0 or cx >= grid[0] or cy >= grid[1]:
            skipped += 1
            continue
        index[cx, cy] = max(index[cx, cy], i)
    return index, skipped


def level_planes(levels, base_grid, offset=0.0, patch_size=256):
    """float64 [L, X0 f, Y0 f]: plane l holds ``values_l[idx] + offset`` where level l visited the cell, 0 elsewhere.  The sum is
    rounded in the VALUE's type (float32 values: a float32 add of the float32-rounded offset) and then widened."""
    L = len(levels)
    f = 1 << (L - 1)
    x, y = np.meshgrid(np.arange(base_grid[0] * f), np.arange(base_grid[1] * f), indexing="ij")
    planes = np.zeros((L,) + x.shape, dtype=np.float64)
    for l, lv in enumerate(levels):
        s = L - 1 - l
        index, _ = index_grid(lv["locs"], (base_grid[0] << l, base_grid[1] << l), patch_size)
        idx = index[x >> s, y >> s]
        values = np.asarray(lv["values"])
        assert values.dtype in (np.float32, np.float64)
        if values.size:
            shifted = values + values.dtype.type(offset)
            assert shifted.dtype == values.dtype
            planes[l] = np.where(idx >= 0, shifted[np.maximum(idx, 0)].astype(np.float64), 0.0)
    return planes


def fold_planes(planes, w):
    """float64 [X, Y]: from l = L-2 down to 0, v_l += w * v_{l+1} wherever the (folded) v_{l+1} != 0; returns v_0."""
    v = np.array(planes, dtype=np.float64)
    for l in range(v.shape[0] - 2, -1, -1):
        m = v[l + 1] != 0
        v[l] = np.where(m, v[l] + v[l + 1] * np.float64(w), v[l])
    return v[0]


def raster(levels, base_grid, offset=0.0, fold=None, patch_size=256, dtype=np.float64):
    """The planes form (fold None) or the fold form (fold = w), rounded once to ``dtype``."""
    planes = level_planes(levels, base_grid, offset, patch_size)
    return (planes if fold is None else fold_planes(planes, fold)).astype(dtype)
