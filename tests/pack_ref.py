"""NumPy contract of the packed (tissue-only) slide form (paths_amd/data_utils/slide.py: pack_host_grid; csrc/pack_rows.hip).

A row is KEPT iff any of its bits is set: only rows that are all +0.0 are dropped (a -0.0 element is a set bit, and a row whose
elements cancel to a zero sum is kept although its tissue mask is 0).  Kept rows are ranked in row-major cell order: the rank is
the exclusive prefix sum of the kept flags."""
import numpy as np


def _bits(grid: np.ndarray) -> np.ndarray:
    assert grid.dtype in (np.float32, np.float16) and grid.ndim == 3
    return np.ascontiguousarray(grid).view(np.uint32 if grid.dtype == np.float32 else np.uint16)


def kept_flags(grid: np.ndarray) -> np.ndarray:
    """uint8 [X * Y]: 1 iff any bit of the cell's row is set."""
    X, Y, _ = grid.shape
    return (_bits(grid).reshape(X * Y, -1) != 0).any(axis=1).astype(np.uint8)


def pack(grid: np.ndarray):
    """grid [X, Y, D] -> (rows [n, D], index int32 [X, Y], n)."""
    X, Y, D = grid.shape
    kept = kept_flags(grid).astype(bool)
    rank = np.cumsum(kept) - kept                     # exclusive prefix sum, row-major
    index = np.where(kept, rank, -1).astype(np.int32).reshape(X, Y)
    rows = np.ascontiguousarray(grid).reshape(X * Y, D)[kept]
    return rows, index, int(kept.sum())


def unpack(rows: np.ndarray, index: np.ndarray) -> np.ndarray:
    X, Y = index.shape
    out = np.zeros((X * Y, rows.shape[1]), dtype=rows.dtype)
    flat = index.reshape(-1)
    out[flat >= 0] = rows[flat[flat >= 0]]
    return out.reshape(X, Y, rows.shape[1])


def tissue_mask(grid: np.ndarray) -> np.ndarray:
    """uint8 [X, Y]: the fp32 row sum != 0 (the child filter's rule; NOT the kept rule)."""
    return (grid.astype(np.float32).sum(axis=2) != 0).astype(np.uint8)


def case_grids(dtype, shape=(5, 7), D=128, seed=0):
    """The levels every pack test runs, as a dict name -> grid [X, Y, D]: a mixed level with a zero-sum row (kept, mask 0) and a row of
    -0.0 only (kept), an all-background level, a level without a zero row and a single-cell grid."""
    rng = np.random.default_rng(seed)
    X, Y = shape
    mixed = rng.standard_normal((X, Y, D)).astype(np.float32).astype(dtype)
    bg = rng.random((X, Y)) < 0.5
    bg.reshape(-1)[[0, -1]] = [True, False]           # (the first cell dropped, the last kept: both ends of the scan)
    mixed[bg] = 0
    if X * Y >= 4:
        cells = np.flatnonzero(bg.reshape(-1))
        zs, nz = (int(cells[1]), int(cells[2])) if cells.size >= 3 else (1, 2)
        flat = mixed.reshape(X * Y, D)
        flat[zs] = 0
        flat[zs, 3], flat[zs, 77 % D] = 1.5, -1.5     # elements cancel: sum exactly 0, mask 0, but the row is kept
        flat[nz] = -0.0                               # all -0.0: every sign bit set, kept
    full = rng.standard_normal((X, Y, D)).astype(np.float32).astype(dtype)
    full[full == 0] = 1
    return {"mixed": mixed, "all_background": np.zeros((X, Y, D), dtype=dtype), "no_background": full,
            "single_cell": full[:1, :1].copy(), "single_cell_background": np.zeros((1, 1, D), dtype=dtype)}
