"""The resize in front of the encoder on the GPU (paths_amd.pixels.encoder_input(resize=...), csrc/tile_resize.hip) against
tests/resize_ref.py bit for bit: every shape at which the kernel takes another path, all three element types, tiles as a batch
and as windows into a mosaic whose rows carry 0xA5 padding, sub-ranges of ``order``, under poisoned allocations; the unresized
kernel as the identity's twin; then OnDemandSlide over a TileEncoder(resize=28, crop=16) against a resident twin built on the host
over ALL cells."""
import functools

import numpy as np
import pytest
import torch

from tests import poison as PZ
from tests import resize_ref as RR
from tests import tiles_ref as TR
from tests.helpers import build_model
from tests.test_gpu_half_grids import assert_same_recursion
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PAD_BYTE = 0xA5
KINDS = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (P, S, C): crop offset 6 | three pieces of columns, offset 4 | upscale | 3 x down, 13 taps (bicubic) | identity | odd S, offset 0 by
# half-to-even, 17 taps | several bands: 8 of 28 rows with 16-bit elements, 9 of 25 and 24 in fp32, whose count does not divide the rows |
# bands of a few rows in more than 64 KiB of LDS
SHAPES = [(32, 28, 16), (64, 56, 48), (16, 24, 16), (48, 16, 16), (32, 32, 32), (64, 17, 16), (256, 224, 224), (1024, 256, 256)]
POISON = [123456, -3, 1 << 30]                      # entries of ``order`` outside [first, first + count): never read


def padded(dev, image, pad, fill=PAD_BYTE):
    """``image`` (uint8 [rows, cols, 3]) on the device inside rows that carry at least ``pad`` more bytes of ``fill``."""
    rows, cols = image.shape[:2]
    stride = (3 * cols + pad + 15) // 16 * 16
    whole = torch.full((rows, stride), fill, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 16 == 0
    view = whole[:, :3 * cols].unflatten(1, (cols, 3))
    view.copy_(torch.from_numpy(np.ascontiguousarray(image)).to(dev))
    return view


def windows(dev, tiles, pad, per_row=3):
    """The tiles as windows into one padded mosaic image (white where the last grid row has no tile): the (addresses, stride) pair of
    pixels.LevelImages, and what keeps it alive."""
    from paths_amd import pixels
    n, P = tiles.shape[:2]
    image = np.full(((n + per_row - 1) // per_row * P, per_row * P, 3), 255, np.uint8)
    cells = np.stack([np.arange(n) // per_row, np.arange(n) % per_row], axis=1)
    for k, (x, y) in enumerate(cells):
        image[x * P:(x + 1) * P, y * P:(y + 1) * P] = tiles[k]
    im = padded(dev, image, pad)
    return pixels.LevelImages([im], patch_size=P)(0, torch.from_numpy(cells).to(dev)), im


def make_tiles(n, P, seed):
    """Random tiles with a block of 0 / 255 noise and a 255 block inside a 0 block (both passes clip at both ends); the last tile is
    constant."""
    rng = np.random.default_rng(seed)
    tiles = rng.integers(0, 256, (n, P, P, 3), dtype=np.uint8)
    tiles[:, 1:P // 2, 2:P // 2 + 3] = rng.integers(0, 2, (n, P // 2 - 1, P // 2 + 1, 3), dtype=np.uint8) * 255
    tiles[:, P // 2:, : P // 2] = 0
    tiles[:, P // 2 + P // 8: P - P // 8, P // 8: P // 2 - P // 8] = 255
    if n > 1:
        tiles[n - 1] = (17, 201, 255)
    return tiles


@functools.lru_cache(maxsize=None)
def case(P, S, C, interpolation):
    """The tiles of a shape and the cropped bytes the contract gives for them, uint8 [n, C, C, 3]: computed once, never written."""
    n = 1 if P == 1024 else 3 if P == 256 else 5
    tiles = make_tiles(n, P, P + S + C)
    off = RR.crop_offset(S, C)
    want = np.stack([RR.resize_u8(t, S, interpolation)[off:off + C, off:off + C] for t in tiles])
    tiles.setflags(write=False)
    want.setflags(write=False)
    return tiles, want


def through(table, cropped):
    """float32 [m, 3, C, C]: table[c][byte c] of cropped uint8 [m, C, C, 3]."""
    return np.stack([table[c][cropped[..., c]] for c in range(3)], axis=1)


def same_values(got, want):
    """A device tensor holds exactly the float32-representable values of ``want`` (signs of zeros included)."""
    g = got.float().cpu().numpy()
    return g.shape == want.shape and np.array_equal(g, want) and np.array_equal(np.signbit(g), np.signbit(want))


# ------------------------------------------------------------------------------------------------
# 1. bit for bit against the contract
# ------------------------------------------------------------------------------------------------
# (bilinear at (1024, 256, 256) has 9 taps and fits 64 KiB: the path of (256, 224, 224) once more)
CASES = [s + (f,) for s in SHAPES for f in ("bicubic", "bilinear") if (s[0], f) != (1024, "bilinear")]


@pytest.mark.parametrize("P, S, C, interpolation", CASES, ids=["%d-%d-%d-%s" % c for c in CASES])
def test_resized_input_equals_the_contract(dev, P, S, C, interpolation):
    from paths_amd import pixels
    tiles, cropped = case(P, S, C, interpolation)
    n = len(tiles)
    perm = list(np.random.default_rng(S).permutation(n))
    batch = torch.from_numpy(tiles.copy()).to(dev)
    source, keep = windows(dev, tiles, 48 if P == 48 else 16)
    if n > 1:
        assert (cropped[n - 1] == np.array([17, 201, 255], np.uint8)).all(), "a constant tile stays constant"
    ranges = [(0, n)] if n == 1 else [(0, n), (1, 2), (n - 1, 1)]
    for dtype in KINDS:
        table = pixels.normalize_table(MEAN, STD, dtype)
        ref = TR.normalize_table(MEAN, STD, KINDS[dtype])
        d_table = table.to(dev)
        for first, count in ranges:
            order = np.array((POISON * n)[:n], np.int32)
            order[first:first + count] = perm[first:first + count]
            d_order = torch.from_numpy(order).to(dev)
            want = through(ref, cropped[order[first:first + count]])
            for pattern, src in (("H", source), ("F", batch)):
                with PZ.poisoned_empty(pattern):
                    got = pixels.encoder_input(src, d_order, first, count, d_table, patch_size=P, resize=S, crop=C, interpolation=interpolation)
                    again = pixels.encoder_input(src, d_order, first, count, d_table, patch_size=P, resize=S, crop=C, interpolation=interpolation)
                assert got.dtype == dtype and tuple(got.shape) == (count, 3, C, C) and got.is_contiguous()
                assert same_values(got, want), (dtype, first, count, pattern)       # (H fills the output with NaN: every element was written)
                assert PZ.same_bits(got, again), "a second call writes the same bytes"
            if n > 1 and (first, count) == (0, n):
                last = perm.index(n - 1)
                assert all(bool((got[last, c] == table[c, v]).all()) for c, v in enumerate((17, 201, 255)))
    del keep


def test_crop_defaults_to_resize_and_to_tensor_table(dev):
    from paths_amd import pixels
    tiles, cropped = case(32, 32, 32, "bilinear")
    order = torch.arange(len(tiles), dtype=torch.int32, device=dev)
    got = pixels.encoder_input(torch.from_numpy(tiles.copy()).to(dev), order, 0, len(tiles), pixels.to_tensor_table(torch.float32).to(dev), resize=32,
                               interpolation="bilinear")
    assert same_values(got, through(TR.to_tensor_table("float32"), cropped))


# ------------------------------------------------------------------------------------------------
# 2. indices that name nothing
# ------------------------------------------------------------------------------------------------
def test_an_order_entry_outside_the_tiles_gives_the_black_tile(dev):
    from paths_amd import pixels
    tiles, cropped = case(32, 28, 16, "bicubic")
    n = len(tiles)
    table = pixels.normalize_table(MEAN, STD, torch.float16)
    ref = TR.normalize_table(MEAN, STD, "float16")
    order = torch.tensor([2, -1, 0, n, 1 << 30][:n], dtype=torch.int32, device=dev)
    with PZ.poisoned_empty("H"):
        got = pixels.encoder_input(torch.from_numpy(tiles.copy()).to(dev), order, 0, n, table.to(dev), resize=28, crop=16).cpu()
    black = through(ref, np.zeros((1, 16, 16, 3), np.uint8))[0]
    for i, k in enumerate(order.cpu().tolist()):
        want = through(ref, cropped[k:k + 1])[0] if 0 <= k < n else black
        assert np.array_equal(got[i].float().numpy(), want), (i, k)
        if not 0 <= k < n:
            assert all(bool((got[i, c] == table[c, 0]).all()) for c in range(3)) and bool((got[i] != 0).all())


# ------------------------------------------------------------------------------------------------
# 3. the identity is the unresized kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolation", ["bicubic", "bilinear"])
@pytest.mark.parametrize("P", [16, 48, 64])
def test_resize_to_the_tiles_own_size_equals_the_unresized_kernel(dev, P, interpolation):
    from paths_amd import pixels
    tiles = make_tiles(4, P, P)
    order = torch.tensor([3, 1, 0, 2], dtype=torch.int32, device=dev)
    source, keep = windows(dev, tiles, 16)
    for dtype in KINDS:
        table = pixels.normalize_table(MEAN, STD, dtype).to(dev)
        plain = pixels.encoder_input(source, order, 0, 4, table, patch_size=P)
        with PZ.poisoned_empty("H"):
            got = pixels.encoder_input(source, order, 0, 4, table, patch_size=P, resize=P, crop=P, interpolation=interpolation)
        assert PZ.same_bits(got, plain), dtype
    del keep


# ------------------------------------------------------------------------------------------------
# 4. end to end: OnDemandSlide over a TileEncoder(resize=28, crop=16) against a resident twin built on the host over all cells
# ------------------------------------------------------------------------------------------------
P0, S0, C0, DIM, KEEP, LEVELS = 32, 28, 16, 128, [12, 12], 3
PICK = np.sort(np.random.default_rng(78).choice(3 * C0 * C0, DIM, replace=False))


def level_images(grid, seed):
    """Random dark pixels with bright specks (the cubic overshoots), about a third of the cells of every level painted white."""
    rng = np.random.default_rng(seed)
    images = []
    for l in range(LEVELS):
        X, Y = grid[0] << l, grid[1] << l
        im = rng.integers(0, 150, (X * P0, Y * P0, 3), dtype=np.uint8)
        im[rng.random(im.shape[:2]) < 0.02] = 255
        blank = rng.random((X, Y)) < 1 / 3
        if l == 0:
            blank[0, 0] = False
        im[np.repeat(np.repeat(blank, P0, axis=0), P0, axis=1)] = 255
        images.append(im)
    return images


def pick_model(x):
    """A fixed linear map of the [count, 3, 16, 16] input - 128 of its elements: exact, and independent of the batch it is called with."""
    assert tuple(x.shape[1:]) == (3, C0, C0)
    return x.flatten(1)[:, torch.from_numpy(PICK).to(x.device)]


def host_level(image, threshold, table):
    """The grid [X, Y, DIM] of one level over ALL its cells by the two contracts: tests/tiles_ref.py decides the tissue on the tile's
    own pixels, tests/resize_ref.py gives the input of the tissue tiles."""
    tiles = TR.cell_tiles(image, P0)
    _, _, order, m, slots = TR.tissue(tiles, threshold)
    encoded = RR.resized_input(tiles, order, 0, m, table, S0, C0).reshape(m, -1)[:, PICK] if m else None
    return TR.scatter_rows(encoded, slots, DIM, np.float32).reshape(image.shape[0] // P0, image.shape[1] // P0, DIM)


def test_on_demand_over_resized_pixels_is_bitwise_the_host_twin(dev):
    from paths_amd import pixels
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, OnDemandSlide
    paths_model = build_model(dev, 0, {"model_config": {"patch_embed_dim": DIM}, "num_levels": LEVELS}, top_k_patches=KEEP)[1]
    od, twins, encoders, calls = [], [], [], []
    ref_table = TR.to_tensor_table("float16")
    for j, (grid, seed) in enumerate(zip([(3, 5), (2, 2)], [1, 2])):
        images = level_images(grid, seed)
        on_dev = [padded(dev, im, 16 if l % 2 == 0 else 48) for l, im in enumerate(images)]
        t = TR.otsu(TR.histogram(images[:1]))

        def model(x, j=j):
            calls.append((j, int(x.shape[0])))
            return pick_model(x)

        enc = pixels.TileEncoder.fit(on_dev[:1], pixels.LevelImages(on_dev, patch_size=P0), model, DIM, patch_size=P0, batch=40, resize=S0, crop=C0)
        assert enc.threshold == t
        shapes = [(grid[0] << l, grid[1] << l) for l in range(LEVELS)]
        od.append(OnDemandSlide(shapes, enc, DIM, dev, slide_id=f"resized-{j}"))
        twins.append(DeviceSlide.from_host([torch.from_numpy(host_level(im, t, ref_table)) for im in images], dev))
        encoders.append(enc)

    def run(slides):
        trace = []
        with torch.no_grad():
            out = putils.recurse(paths_model, slides, KEEP, LEVELS, trace=trace)
        torch.cuda.synchronize()
        return trace, out

    tb, ob = run(twins)
    assert int(ob["status"].item()) == 0
    with PZ.poisoned_empty("H"):
        ta, oa = run(od)
    assert int(oa["status"].item()) == 0
    assert_same_recursion(ta, tb, oa, ob)
    for j, (s, e) in enumerate(zip(od, encoders)):
        req, tis = e.stats["requested"], e.stats["tissue"]
        assert [req[l] for l in range(LEVELS)] == [int(s.requested[l].shape[0]) for l in range(LEVELS)]
        assert req[0] == s.shapes[0][0] * s.shapes[0][1] and 0 < sum(tis.values()) < sum(req.values()), "fewer model rows than requested cells"
        assert sum(n for k, n in calls if k == j) == sum(tis.values()) and all(n <= 40 for _, n in calls)
        assert e.stats["model_calls"] == {l: -(-tis[l] // 40) for l in range(LEVELS)}
