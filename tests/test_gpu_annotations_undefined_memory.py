"""What the annotation kernels may look at (include/paths_hip.h, "annotation polygons"): the words between the packed vertex, offset
and range arrays are never read, the coverage allocation is never read on entry and written in full, and an outline touches no byte it
does not paint.  The criterion is tests/poison.py's: the defined outputs are bit-identical whatever such memory held.  poison.py leaves
integer tensors alone, so the integer buffers are filled here: the pad words and the output hold counts and coordinates, never addresses."""
import numpy as np
import pytest
import torch

from tests import poison as PZ
from tests import polygon_ref as PR
from tests.test_gpu_annotations import L, OUTLINE_GRIDS, outline_polygons, random_images
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PAD_WORD = {"Z": 0, "F": 123456789, "H": -(1 << 31)}
OUT_WORD = {"Z": 0, "F": 777, "H": -1}


@pytest.mark.parametrize("s, cell_px, width", [(4, 4, 1), (16, 1, 3)])
def test_annotation_kernels_do_not_depend_on_padding_or_on_what_their_output_held(dev, s, cell_px, width):
    from paths_amd import annotations as A
    host = {}

    def fn(pattern):
        p = A.Polygons(outline_polygons(), OUTLINE_GRIDS, L)
        assert p.pad_words.any()
        p.packed[p.pad_words] = PAD_WORD[pattern]                               # before the first upload
        X, Y = max(g[0] for g in p.grids) << (L - 1), max(g[1] for g in p.grids) << (L - 1)
        out = torch.full((p.B, X, (Y + 3) // 4 * 4), OUT_WORD[pattern], dtype=torch.int32, device=dev)
        host["image"], base, views = random_images(dev, p, cell_px, 9, 42)
        with PZ.poisoned_empty(pattern, seed=5):
            A.coverage(p, s, out=out)
            with torch.cuda.device(dev):
                fresh = A.coverage(p, s)                                         # an allocation of the package's own
            A.draw(views, p, cell_px, width=width)
        host["p"] = p
        return {"cover": out, "fresh": fresh[0]._base if fresh[0]._base is not None else fresh[0], "image": base}

    res = PZ.assert_independent(fn, f"annotations s {s} cell_px {cell_px} width {width}")
    p = host["p"]
    assert PZ.same_bits(res["cover"], res["fresh"])
    for b in range(p.B):
        x, y = p.finest(b)
        assert np.array_equal(res["cover"][b, :x, :y].cpu().numpy(), PR.coverage(p.slide_polygons(b), x, y, s))
    assert (res["image"].cpu().numpy() != host["image"]).any()
