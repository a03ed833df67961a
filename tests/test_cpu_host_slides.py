"""Host-resident slides, host side (no GPU needed): the NumPy restatement of the row-staging contract, the chunk planner of the mask
pass, and the checks that must come before the device is touched."""
import os
import types

import numpy as np
import pytest
import torch

from paths_amd.data_utils import slide as S
from tests import stage_ref


@pytest.mark.parametrize("row_bytes", [4096, 2048, 512])
def test_stage_reference_copies_valid_rows_and_keeps_padding(row_bytes):
    rng = np.random.default_rng(row_bytes)
    n_src, rows = 40, 23
    memory = rng.integers(0, 256, size=(n_src + 1) * row_bytes, dtype=np.uint8)
    zero_row = n_src * row_bytes                          # (an address like any other; its row is never read)
    pick = rng.permutation(n_src)[:rows]                  # out of order, no duplicates needed for the contract but allowed:
    pick[5] = pick[2]                                     # the same source row twice
    ptrs = pick.astype(np.int64) * row_bytes
    pad = np.array([0, 7, 8, rows - 1])
    ptrs[pad] = zero_row
    stage_addr = 1 << 40
    stage, out = stage_ref.stage_rows(memory, ptrs, row_bytes, stage_addr, zero_row)
    valid = np.setdiff1d(np.arange(rows), pad)
    for m in valid:
        np.testing.assert_array_equal(stage[m], memory[ptrs[m]:ptrs[m] + row_bytes])
        assert out[m] == stage_addr + m * row_bytes
    assert (out[pad] == zero_row).all() and not stage[pad].any()
    np.testing.assert_array_equal(stage[5], stage[2])


def test_stage_reference_argument_check():
    ok = np.zeros(4, np.int64)
    assert stage_ref.check_args(ok, 4, 4096, 1, 2) == 0
    assert stage_ref.check_args(ok, 4, 4100, 1, 2) == -1          # row_bytes % 16
    assert stage_ref.check_args(ok, 4, 0, 1, 2) == -1
    assert stage_ref.check_args(ok, 0, 4096, 1, 2) == -1
    assert stage_ref.check_args(None, 4, 4096, 1, 2) == -1
    assert stage_ref.check_args(ok, 4, 4096, None, 2) == -1
    assert stage_ref.check_args(ok, 4, 4096, 1, None) == -1


@pytest.mark.parametrize("cells,D,itemsize,budget", [
    (1024, 1024, 4, 64 << 20),          # a grid smaller than one chunk
    (512 * 512, 1024, 4, 64 << 20),     # whole chunks
    (1000, 256, 2, 100_000),            # a last partial chunk, budget not a multiple of the row
    (7, 64, 4, 256),                    # one row per chunk
    (5, 64, 4, 1 << 30),
])
def test_chunk_planner_covers_every_row_once_within_the_budget(cells, D, itemsize, budget):
    plan = S.plan_mask_chunks(cells, D, itemsize, budget)
    assert all(rows >= 1 and rows * D * itemsize <= budget for _, rows in plan)
    covered = np.zeros(cells, np.int64)
    nxt = 0
    for r0, rows in plan:
        assert r0 == nxt                                           # in order, no gaps
        covered[r0:r0 + rows] += 1
        nxt = r0 + rows
    assert nxt == cells and (covered == 1).all()
    if cells * D * itemsize <= budget:
        assert plan == [(0, cells)]
    assert all(rows == plan[0][1] for _, rows in plan[:-1])        # only the last chunk is partial


def test_chunk_planner_rejects_a_budget_below_one_row():
    with pytest.raises(ValueError):
        S.plan_mask_chunks(100, 1024, 4, 4095)
    with pytest.raises(ValueError):
        S.plan_mask_chunks(100, 1024, 4, 0)
    assert S.plan_mask_chunks(100, 1024, 4, 4096) == [(i, 1) for i in range(100)]


def test_batch_rejects_mixed_resident_and_host_slides():
    """The kind check comes first: stand-ins are enough, no table is built."""
    res = types.SimpleNamespace(host_resident=False)
    host = types.SimpleNamespace(host_resident=True)
    with pytest.raises(ValueError, match="all resident"):
        S.DeviceSlideBatch([res, host])
    with pytest.raises(ValueError, match="all resident"):
        S.DeviceSlideBatch([host, host, res])
    assert S.DeviceSlide.host_resident is False and S.HostSlide.host_resident is True


def test_from_preprocessed_checks_dtype_and_files_before_the_device(tmp_path):
    with pytest.raises(NotImplementedError):
        S.HostSlide.from_preprocessed(str(tmp_path), "s0", [0.625, 1.25], dtype=torch.bfloat16)
    with pytest.raises(FileNotFoundError):
        S.HostSlide.from_preprocessed(str(tmp_path), "s0", [0.625, 1.25])
    # one of two files present: still refused, and before anything is loaded
    torch.save(torch.zeros(2, 2, 8), os.path.join(str(tmp_path), "s0_0.625.pt"))
    with pytest.raises(FileNotFoundError, match="1.250"):
        S.HostSlide.from_preprocessed(str(tmp_path), "s0", [0.625, 1.25])


def test_host_slide_refuses_device_free_construction_errors_first():
    g = torch.zeros(2, 2, 8)
    with pytest.raises(NotImplementedError):
        S.HostSlide([g.to(torch.bfloat16)])
    with pytest.raises(ValueError):
        S.HostSlide([g, g.half()])
    with pytest.raises(ValueError):
        S.HostSlide([g.reshape(4, 8)])
    with pytest.raises(ValueError):                                # cached masks need the cached absmax with them
        S.HostSlide([g], masks=[torch.zeros(2, 2, dtype=torch.uint8)])
