"""NumPy statement of the contracts of the two row-cache kernels behind CachedOnDemandSlide (include/paths_hip.h: paths_cache_probe,
paths_cache_fill / _h16), for the CPU and GPU tests.

Both functions WRITE INTO the output arrays they are given, like the kernels: what the contract leaves untouched keeps the caller's
fill, so a test that pre-fills the device buffers with the same sentinel can compare every byte.  Per-slide arguments are lists of
length B: ``cells[b]`` int64 [n_b, 2], ``index[b]`` int32 [X_b, Y_b], ``enc[b]`` [m_b, D] (None where nothing was encoded),
``store[b]`` [capacity_b, D] with ``count[b]`` rows in use."""
import numpy as np

SRC_NONE = -(1 << 31)         # PATHS_CACHE_SRC_NONE: a cell outside its grid


def check_args(B: int, n_max: int, D: int) -> int:
    return 0 if (B > 0 and n_max > 0 and D > 0 and D % 4 == 0) else -1


def probe(cells, n, index, src, miss_count, miss_cells, status):
    """src [B, n_max] int32, miss_count [B] int32, miss_cells [B, n_max, 2] int64, status [B] int32.  Hit: the store row; the j-th
    miss in request order: -1 - j, its coordinates in miss_cells[b, j]; a cell outside the grid: SRC_NONE and status[b] = 1 (else 0)."""
    n_max = src.shape[1]
    for b in range(len(cells)):
        X, Y = index[b].shape
        j, bad = 0, 0
        for i in range(max(0, min(int(n[b]), n_max))):
            cx, cy = int(cells[b][i, 0]), int(cells[b][i, 1])
            if not (0 <= cx < X and 0 <= cy < Y):
                src[b, i], bad = SRC_NONE, 1
            elif index[b][cx, cy] >= 0:
                src[b, i] = index[b][cx, cy]
            else:
                src[b, i] = -1 - j
                miss_cells[b, j] = (cx, cy)
                j += 1
        miss_count[b] = j
        status[b] = bad
    return src, miss_count, miss_cells, status


def fill(cells, n, src, miss_count, enc, store, count, capacity, index, out):
    """out [B, n_max, D]; store[b] and index[b] are updated in place.  Returns the new counts (the caller's to advance)."""
    n_max = out.shape[1]
    new_count = []
    for b in range(len(cells)):
        X, Y = index[b].shape
        nb = max(0, min(int(n[b]), n_max))
        cnt, cap, m = max(0, int(count[b])), int(capacity[b]), int(miss_count[b])
        for i in range(nb):
            s = int(src[b, i])
            if 0 <= s < min(cnt, cap):
                out[b, i] = store[b][s]
            elif s < 0 and s != SRC_NONE and -1 - s < m:
                j = -1 - s
                out[b, i] = enc[b][j]
                if cnt + j < cap:
                    store[b][cnt + j] = enc[b][j]
                    cx, cy = int(cells[b][i, 0]), int(cells[b][i, 1])
                    if 0 <= cx < X and 0 <= cy < Y:
                        index[b][cx, cy] = cnt + j
            else:
                out[b, i] = 0
        out[b, nb:] = 0
        new_count.append(cnt + max(0, min(m, cap - cnt)))
    return new_count
