"""Packed (tissue-only) slides, host side: pack_host_grid against its NumPy contract (tests/pack_ref.py), the round trip through the dense
form, and the refusals of from_patches, which must come before the device is touched (no GPU needed)."""
import numpy as np
import pytest
import torch

from paths_amd.data_utils import slide as S
from tests import pack_ref as R

DTYPES = {"float32": (np.float32, torch.float32), "float16": (np.float16, torch.float16)}


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", ["mixed", "all_background", "no_background", "single_cell", "single_cell_background"])
def test_pack_host_grid_matches_the_contract(name, dtype):
    npd, _ = DTYPES[dtype]
    g = R.case_grids(npd, (5, 7), 128)[name]
    rows, index = S.pack_host_grid(torch.from_numpy(g))
    ref_rows, ref_index, n = R.pack(g)
    assert index.dtype == torch.int32 and tuple(index.shape) == g.shape[:2] and rows.dtype == torch.from_numpy(g).dtype
    assert tuple(rows.shape) == (n, 128) and rows.is_contiguous()
    np.testing.assert_array_equal(index.numpy(), ref_index)
    bits = np.uint32 if npd == np.float32 else np.uint16
    np.testing.assert_array_equal(rows.numpy().view(bits), ref_rows.view(bits))
    if name == "all_background" or name == "single_cell_background":
        assert n == 0 and (ref_index == -1).all()
    if name == "no_background":
        assert n == g.shape[0] * g.shape[1] and np.array_equal(ref_index.reshape(-1), np.arange(n))


def test_the_kept_rule_is_not_the_tissue_mask():
    g = R.case_grids(np.float32, (5, 7), 128)["mixed"]
    kept, mask = R.kept_flags(g).astype(bool), R.tissue_mask(g).reshape(-1).astype(bool)
    flat = g.reshape(-1, 128)
    zero_sum = kept & ~mask & (flat != 0).any(axis=1)
    neg_zero = kept & ~(flat != 0).any(axis=1)
    assert zero_sum.sum() == 1 and neg_zero.sum() == 1, "the case grid holds one zero-sum row and one row of -0.0 only"
    assert np.signbit(flat[neg_zero]).all()
    assert not (mask & ~kept).any(), "every tissue row is kept"
    _, index = S.pack_host_grid(torch.from_numpy(g))
    assert (index.reshape(-1).numpy()[zero_sum | neg_zero] >= 0).all()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_pack_then_unpack_is_the_grid_bit_for_bit(dtype):
    npd, _ = DTYPES[dtype]
    bits = np.uint32 if npd == np.float32 else np.uint16
    for name, g in R.case_grids(npd, (5, 7), 128).items():
        rows, index = S.pack_host_grid(torch.from_numpy(g))
        back = S.unpack_grid(rows, index).numpy()
        ref = g.copy()
        # a dropped row is all +0.0 and comes back as +0.0; every kept row keeps its bits, -0.0 included
        np.testing.assert_array_equal(back.view(bits), ref.view(bits), err_msg=name)
        np.testing.assert_array_equal(R.unpack(*R.pack(g)[:2]).view(bits), ref.view(bits), err_msg=name)


def _patches(n=4, D=8, dtype=torch.float32):
    coords = [torch.tensor([[0, 0], [1, 2], [2, 1], [0, 3]][:n], dtype=torch.int64), torch.zeros((0, 2), dtype=torch.int64)]
    feats = [torch.ones((n, D), dtype=dtype), torch.zeros((0, D), dtype=dtype)]
    return coords, feats, [(3, 4), (6, 8)]


def test_check_patches_accepts_a_level_without_tissue_and_keeps_the_order():
    coords, feats, shapes = _patches()
    cells = S.check_patches(coords, feats, shapes, torch.float32)
    assert [c.tolist() for c in cells] == [[0, 6, 9, 3], []]
    index = S._patch_index(cells[0], shapes[0])
    assert index.dtype == torch.int32 and index.reshape(-1).tolist() == [0, -1, -1, 3, -1, -1, 1, -1, -1, 2, -1, -1]
    assert (S._patch_index(cells[1], shapes[1]) == -1).all()


@pytest.mark.parametrize("cls", [S.DeviceSlide, S.HostSlide])
@pytest.mark.parametrize("what", ["duplicate", "outside", "negative", "length", "levels", "bfloat16", "float64"])
def test_from_patches_refuses_before_the_device_is_touched(cls, what, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("from_patches reached the device before its checks")

    monkeypatch.setattr(S._lib, "call", no_launch)
    monkeypatch.setattr(S._lib, "load", no_launch)
    coords, feats, shapes = _patches()
    dtype = torch.float32
    if what == "duplicate":
        coords[0][3] = coords[0][1]
    elif what == "outside":
        coords[0][2, 1] = 4                  # y = 4 in a 3 x 4 grid
    elif what == "negative":
        coords[0][0, 0] = -1
    elif what == "length":
        feats[0] = feats[0][:3]
    elif what == "levels":
        shapes = shapes[:1]
    elif what == "bfloat16":
        dtype = torch.bfloat16
    elif what == "float64":
        dtype = torch.float64
    with pytest.raises(ValueError):
        cls.from_patches(coords, feats, shapes, "cuda", dtype=dtype)


def test_batches_refuse_a_mix_of_packed_and_dense_slides():
    class Fake:
        host_resident, masked_view, dtype, dim, num_levels = False, False, torch.float32, 8, 1

        def __init__(self, packed):
            self.packed = packed

    with pytest.raises(ValueError, match="packed"):
        S.DeviceSlideBatch([Fake(True), Fake(False)])


def test_existing_slides_are_not_packed():
    assert S.DeviceSlide.packed is False and S.HostSlide.packed is False
    assert S.DeviceSlide.rows is None and S.DeviceSlide.index is None
