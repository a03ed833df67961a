"""fp16 feature grids, host side: the synthetic fp16 pyramid, the host conversion helper and the dtype checks that must run before
any file is read or the device is touched (no GPU needed)."""
import numpy as np
import pytest
import torch

from paths_amd import synthetic as syn
from paths_amd.data_utils import slide as S


def _cells(spec, level):
    X, Y = spec.shape(level)
    xs, ys = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    return xs.reshape(-1), ys.reshape(-1)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_synthetic_float16_rows_are_rne_rounded_fp32_rows(level):
    spec16 = syn.SyntheticSlide(7, 3, (4, 6), dim=64, num_levels=3, feature_dtype="float16")
    spec32 = syn.SyntheticSlide(7, 3, (4, 6), dim=64, num_levels=3)
    x, y = _cells(spec16, level)
    f32 = syn.cell_features(7, 3, level, x, y, 64, 0.1)
    got16 = spec16.rows(level, x, y)
    assert got16.dtype == np.float32
    np.testing.assert_array_equal(got16, f32.astype(np.float16).astype(np.float32))
    # the default is the generator's fp32 values, bit for bit
    assert spec32.feature_dtype == "float32"
    np.testing.assert_array_equal(spec32.rows(level, x, y), f32)
    # rounding moved values (the test is not vacuous) but kept every background row at zero and every tissue row nonzero
    assert (got16 != f32).any()
    bg = spec16.is_background(level, x, y)
    assert not got16[bg].any() and (got16[~bg] != 0).any(axis=1).all()
    np.testing.assert_array_equal(spec16.grid(level).reshape(-1, 64), got16)


def test_synthetic_feature_dtype_is_checked():
    with pytest.raises(NotImplementedError):
        syn.SyntheticSlide(0, 0, (2, 2), feature_dtype="bfloat16")
    with pytest.raises(ValueError):
        syn.SyntheticSlide(0, 0, (2, 2), feature_dtype="float64")


def test_to_float16_rounds_and_reports_the_error():
    g = np.random.default_rng(0).standard_normal((3, 5, 16)).astype(np.float32)
    g[1, 2] = 0.0                                             # a background row stays background
    h, err = S.to_float16(g)
    assert h.dtype == torch.float16 and h.shape == (3, 5, 16)
    ref = torch.from_numpy(g).to(torch.float16)
    assert torch.equal(h, ref)
    assert err == float((ref.float() - torch.from_numpy(g)).abs().max()) and 0 < err < 2e-3
    h2, err2 = S.to_float16(ref)                              # fp16 input: unchanged, exact
    assert torch.equal(h2, ref) and err2 == 0.0
    # chunked conversion gives the same answer
    h3, err3 = S.to_float16(g, chunk_rows=4)
    assert torch.equal(h3, ref) and err3 == err


@pytest.mark.parametrize("bad", [70000.0, -65505.0, float("inf"), float("-inf"), float("nan")])
def test_to_float16_refuses_values_out_of_range(bad):
    g = np.ones((2, 2, 8), np.float32)
    g[1, 0, 3] = bad
    with pytest.raises(ValueError):
        S.to_float16(g)


def test_to_float16_keeps_the_largest_finite_value():
    g = np.full((1, 1, 4), 65504.0, np.float32)
    h, err = S.to_float16(g)
    assert float(h.max()) == 65504.0 and err == 0.0


def test_to_float16_refuses_a_tissue_row_that_rounds_to_zero():
    g = np.ones((2, 3, 8), np.float32)
    g[1, 1] = 0.0
    g[1, 1, 5] = 1e-9                                         # nonzero in fp32, zero in fp16: the cell would become background
    with pytest.raises(ValueError, match="tissue row 4"):
        S.to_float16(g)
    g[1, 1, 6] = 1e-3                                         # one value survives: still tissue, accepted
    h, _ = S.to_float16(g)
    assert (h[1, 1] != 0).any()


def test_bfloat16_is_rejected_before_any_io(tmp_path):
    # the root does not exist: reaching the file system would fail differently; the device ("cuda") is never touched on this host
    with pytest.raises(NotImplementedError):
        S.DeviceSlide.from_preprocessed(str(tmp_path / "missing"), "slide", [20.0], device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        S.DeviceSlide.from_preprocessed(str(tmp_path / "missing"), "slide", [20.0], device="cuda", dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        S.DeviceSlide.from_host([np.zeros((2, 2, 4), np.float32)], "cuda", dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        S.DeviceSlide([torch.zeros((2, 2, 4), dtype=torch.bfloat16)])
    with pytest.raises(NotImplementedError):
        S.DeviceSlide.synthetic(0, 0, (2, 2), dim=8, num_levels=1, device="cuda", dtype=torch.bfloat16)


def test_from_preprocessed_fp16_checks_values_before_the_device(tmp_path):
    # a file that fp16 cannot hold is refused on the host, before any upload
    torch.save(torch.full((2, 2, 8), 1e6), str(tmp_path / "s_20.000.pt"))
    with pytest.raises(ValueError):
        S.DeviceSlide.from_preprocessed(str(tmp_path), "s", [20.0], device="cuda", dtype=torch.float16)


class _FakeSlide:
    def __init__(self, dtype):
        self.grids = [torch.zeros((2, 2, 8), dtype=dtype)]
        self.num_levels, self.dim, self.dtype = 1, 8, dtype


def test_batch_refuses_mixed_dtypes():
    with pytest.raises(ValueError, match="share the grid dtype"):
        S.DeviceSlideBatch([_FakeSlide(torch.float32), _FakeSlide(torch.float16)])
