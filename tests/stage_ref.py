"""NumPy restatement of the row-staging contract (include/paths_hip.h: paths_stage_rows), for the CPU and GPU tests.

Addresses are modelled as byte offsets into one flat ``memory`` array; ``ZERO_ROW`` stands for the zero row's address (an entry equal
to it is padding: never followed, never changed)."""
import numpy as np


def check_args(row_ptrs, rows: int, row_bytes: int, stage, zero_row) -> int:
    """The entry point's argument check: 0, or -1 (null pointer, no rows, row_bytes not a positive multiple of 16)."""
    if row_ptrs is None or stage is None or zero_row is None:
        return -1
    if rows <= 0 or row_bytes <= 0 or row_bytes % 16 != 0:
        return -1
    return 0


def stage_rows(memory: np.ndarray, row_ptrs: np.ndarray, row_bytes: int, stage_addr: int, zero_row: int):
    """``memory``: uint8 [bytes] (the source rows live in it at the addresses of ``row_ptrs``); returns (stage uint8 [rows, row_bytes],
    new row_ptrs).  Rows of padding entries are left as they were in the stage buffer: they are returned as zeros here and callers
    compare valid rows only."""
    row_ptrs = np.asarray(row_ptrs, dtype=np.int64)
    rows = row_ptrs.shape[0]
    assert check_args(row_ptrs, rows, row_bytes, stage_addr, zero_row) == 0
    stage = np.zeros((rows, row_bytes), dtype=np.uint8)
    out = row_ptrs.copy()
    for m in range(rows):
        src = int(row_ptrs[m])
        if src == zero_row:
            continue
        stage[m] = memory[src:src + row_bytes]
        out[m] = stage_addr + m * row_bytes
    return stage, out
