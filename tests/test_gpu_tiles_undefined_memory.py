"""What the pixel kernels may look at (include/paths_hip.h, "pixels to encoder input"): image bytes behind a row's pixels and tile bytes
outside the P x 3P window are never read, workspaces and outputs are never read on entry.  The criterion is tests/poison.py's: the
defined outputs are bit-identical whatever such memory held - the padding of every row, the neighbouring tiles of a batch that is
addressed in part, the entries of ``order`` beyond m, and every torch.empty of the package."""
import numpy as np
import pytest
import torch

from tests import poison as PZ
from tests import tiles_ref as TR
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _padded(dev, image, pad, pattern, seed):
    rows, cols = image.shape[:2]
    stride = (3 * cols + pad + 15) // 16 * 16
    whole = PZ.fill_(torch.empty((rows, stride), dtype=torch.uint8, device=dev), pattern, seed)
    view = whole[:, :3 * cols].unflatten(1, (cols, 3))
    view.copy_(torch.from_numpy(np.ascontiguousarray(image)).to(dev))
    return view


@pytest.mark.parametrize("P, stride", [(16, 4), (48, 3), (64, 1)])
def test_pixel_kernels_do_not_depend_on_padding_or_on_what_their_buffers_held(dev, P, stride):
    from paths_amd import pixels
    rng = np.random.default_rng(P)
    X, Y = 3, 4
    image = rng.integers(0, 256, (X * P, Y * P, 3), dtype=np.uint8)
    image[:P] //= 3
    image[P:2 * P, 3 * P:] = 240                                                 # cells (1, 3) and (0, 2): background
    image[:P, 2 * P:3 * P] = 255
    thumb = rng.integers(0, 256, (21, 37, 3), dtype=np.uint8)                    # a ragged row end: 37 columns
    cells = torch.tensor([[2, 1], [0, 0], [1, 3], [0, 2], [2, 3]], device=dev)   # five of the twelve cells: the others are neighbours
    t = TR.otsu(TR.histogram([image, thumb]))
    table = pixels.normalize_table((0.5, 0.4, 0.3), (0.2, 0.25, 0.3), torch.float16).to(dev)
    want = TR.tissue(TR.cell_tiles(image, P, cells.cpu().numpy()), t, 0.1, stride)
    assert 0 < want[3] < 5

    def fn(pattern):
        im = _padded(dev, image, 48, pattern, 1)
        th = _padded(dev, thumb, 16, pattern, 2)
        with PZ.poisoned_empty(pattern, seed=3):
            counts = pixels.grey_histogram([im, th])
            assert pixels.otsu_from_histogram(counts) == t
            source = pixels.LevelImages([im], patch_size=P)(0, cells)
            ts = pixels.tile_tissue(source, t, 0.1, stride, patch_size=P)
            order = ts.order.clone()
            order[ts.m:] = {"Z": 0, "F": 3, "H": 1 << 30}[pattern]              # entries beyond m: never read
            x = pixels.encoder_input(source, order, 0, ts.m, table, patch_size=P)
            rows = pixels.scatter_rows(x.flatten(1)[:, :132], ts.slots, 5, 132, torch.float32)
        return {"histogram": counts, "counts": ts.counts, "flags": ts.flags, "order": ts.order[:ts.m], "slots": ts.slots, "input": x, "rows": rows}

    res = PZ.assert_independent(fn, f"pixels P {P} stride {stride}")
    assert np.array_equal(res["histogram"].cpu().numpy(), TR.histogram([image, thumb]))
    assert res["counts"].cpu().numpy().tolist() == want[0].tolist() and res["slots"].cpu().numpy().tolist() == want[4].tolist()
