"""CPU-only tests of the pixel side (paths_amd.pixels, csrc/tiles.hip's entry points): Otsu's threshold against a brute-force
between-class variance on the pixels themselves, the integer form of the tissue comparison, the lookup tables against the torch
expressions they stand for, the C surface, every refusal that happens before a launch, and the NumPy restatement
(tests/tiles_ref.py) against the same yardsticks.  No kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tiles_ref as TR

DTYPES = [(torch.float32, "float32"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16")]


# ------------------------------------------------------------------------------------------------
# Otsu
# ------------------------------------------------------------------------------------------------
def _brute(g):
    """{t: n0 n1 (mean0 - mean1)^2} for every t that splits the pixels into two non-empty classes, from the pixels themselves."""
    g = np.asarray(g).reshape(-1)
    out = {}
    for t in range(int(g.min()), int(g.max())):
        lo, hi = g[g <= t], g[g > t]
        out[t] = float(len(lo)) * float(len(hi)) * (np.mean(lo.astype(np.float64)) - np.mean(hi.astype(np.float64))) ** 2
    return out


def _images():
    rng = np.random.default_rng(11)
    yield "random", rng.integers(0, 256, (40, 52, 3), dtype=np.uint8)
    yield "narrow", rng.integers(90, 140, (33, 17, 3), dtype=np.uint8)
    both = np.where(rng.random((64, 48, 1)) < 0.35, rng.normal(70, 12, (64, 48, 3)), rng.normal(215, 9, (64, 48, 3)))
    yield "bimodal", np.clip(both, 0, 255).astype(np.uint8)
    skew = np.where(rng.random((50, 50, 1)) < 0.04, rng.normal(30, 5, (50, 50, 3)), rng.normal(240, 4, (50, 50, 3)))
    yield "skewed", np.clip(skew, 0, 255).astype(np.uint8)


def test_otsu_reaches_the_brute_force_maximum():
    from paths_amd import pixels
    for name, im in _images():
        g = TR.grey(im)
        counts = TR.histogram([im])
        assert counts.sum() == g.size and np.array_equal(counts, np.bincount(g.reshape(-1), minlength=256))
        var = _brute(g)
        best = max(var.values())
        for t in (pixels.otsu_from_histogram(counts), pixels.otsu_from_histogram(torch.from_numpy(counts)), TR.otsu(counts)):
            assert int(g.min()) <= t < int(g.max()), name
            assert var[t] >= best * (1 - 1e-12), f"{name}: t = {t} reaches {var[t]!r}, the maximum is {best!r}"
        assert pixels.otsu_from_histogram(counts) == TR.otsu(counts), name
    # the joint histogram of several images is the histogram of their pixels together
    ims = [im for _, im in _images()]
    joint = np.concatenate([TR.grey(im).reshape(-1) for im in ims])
    t = pixels.otsu_from_histogram(TR.histogram(ims))
    var = _brute(joint)
    assert var[t] >= max(var.values()) * (1 - 1e-12)


def test_otsu_two_valued_constant_and_ties():
    from paths_amd import pixels
    rng = np.random.default_rng(5)
    for a, b, share in ((10, 200, 0.5), (0, 255, 0.1), (99, 100, 0.7), (3, 250, 0.999)):
        g = np.where(rng.random(5000) < share, a, b)
        g[:2] = (a, b)
        counts = np.bincount(g, minlength=256)
        var = _brute(g)
        assert len({round(v / max(var.values()), 9) for v in var.values()}) == 1, "every t between the two values splits them alike"
        # among exact ties the first is taken
        assert pixels.otsu_from_histogram(counts) == a == TR.otsu(counts)
    for v in (0, 17, 255):
        counts = np.zeros(256, np.int64)
        counts[v] = 1234
        assert pixels.otsu_from_histogram(counts) == v == TR.otsu(counts)
    # a symmetric histogram: t = 1 and t = 2 give the same classes' statistics mirrored, t = 1 comes first
    counts = np.zeros(256, np.int64)
    counts[[0, 1, 3, 4]] = (5, 7, 7, 5)
    assert TR.between_class(counts, 1) == TR.between_class(counts, 2) > TR.between_class(counts, 0)
    assert pixels.otsu_from_histogram(counts) == 1 == TR.otsu(counts)
    # counts far beyond 2^31 stay exact integers until the one conversion
    big = np.zeros(256, np.int64)
    big[[20, 220]] = (3 << 40, 1 << 41)
    assert pixels.otsu_from_histogram(big) == 20
    for bad in (np.zeros(256), np.ones(255), -np.ones(256)):
        with pytest.raises(ValueError, match="otsu_from_histogram"):
            pixels.otsu_from_histogram(bad)


def test_grey_is_opencvs_integer_formula():
    assert TR.grey(np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1]])).tolist() == [0, 255, 76, 150, 29, 1]
    assert 4899 + 9617 + 1868 == 1 << 14


# ------------------------------------------------------------------------------------------------
# the integer form of count / size > tissue_threshold
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [16, 64, 4096])
@pytest.mark.parametrize("thr", [0.1, 0.0, 0.5])
def test_passing_count_is_the_float64_comparison(size, thr):
    from paths_amd import pixels
    need = pixels.passing_count(size, thr)
    assert need == TR.passing_count(size, thr)
    for count in range(size + 1):
        s = np.ones(size, np.int64)
        s[count:] = 0
        assert (s.sum() / s.size > thr) == (count >= need), (count, size, thr)         # (the reference's own expression)


def test_passing_count_edges():
    from paths_amd import pixels
    assert pixels.passing_count(16, 0.1) == 2 and pixels.passing_count(4096, 0.1) == 410 and pixels.passing_count(64, 0.0) == 1
    assert pixels.passing_count(16, -0.5) == 0 and pixels.passing_count(16, 1.0) == 17 and pixels.passing_count(16, 0.9999) == 16
    assert pixels.passing_count(10, float("inf")) == 11 and pixels.passing_count(10, float("-inf")) == 0
    for size, thr in ((10, 0.3), (10, 0.7), (49, 1 / 7), (1, 0.0), (1, 0.5)):
        assert pixels.passing_count(size, thr) == TR.passing_count(size, thr)
    with pytest.raises(ValueError):
        pixels.passing_count(0, 0.1)
    with pytest.raises(ValueError):
        pixels.passing_count(16, float("nan"))


# ------------------------------------------------------------------------------------------------
# lookup tables
# ------------------------------------------------------------------------------------------------
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("dtype, kind", DTYPES, ids=[k for _, k in DTYPES])
def test_tables_equal_the_torch_expressions_on_every_byte(dtype, kind):
    from paths_amd import pixels
    image = torch.arange(256, dtype=torch.uint8).view(16, 16, 1).expand(16, 16, 3).contiguous()      # HWC, every byte in every channel
    x = image.permute(2, 0, 1).float().div(255)                                                      # to_tensor
    want = x.to(dtype).reshape(3, 256)
    got = pixels.to_tensor_table(dtype)
    assert got.dtype == dtype and tuple(got.shape) == (3, 256) and got.is_contiguous()
    assert torch.equal(got.view(torch.int16 if dtype != torch.float32 else torch.int32), want.contiguous().view(torch.int16 if dtype != torch.float32 else torch.int32))
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    want_n = x.sub(mean).div(std).to(dtype).reshape(3, 256)                                          # Normalize
    got_n = pixels.normalize_table(MEAN, STD, dtype)
    assert got_n.dtype == dtype and torch.equal(got_n.float(), want_n.float()) and not torch.signbit(got_n[got_n == 0]).any()
    # the NumPy restatement gives the same values
    assert np.array_equal(TR.to_tensor_table(kind), got.float().numpy())
    assert np.array_equal(TR.normalize_table(MEAN, STD, kind), got_n.float().numpy())


def test_tables_refuse_other_dtypes_and_shapes():
    from paths_amd import pixels
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        pixels.to_tensor_table(torch.float64)
    with pytest.raises(ValueError, match="normalize_table"):
        pixels.normalize_table((0.5, 0.5), STD)
    with pytest.raises(ValueError, match="normalize_table"):
        pixels.normalize_table(MEAN, (1.0, 0.0, 1.0))


# ------------------------------------------------------------------------------------------------
# the NumPy restatement on cases small enough to check by hand
# ------------------------------------------------------------------------------------------------
def test_ref_tissue_compaction_and_rows():
    P = 16
    tiles = np.full((5, P, P, 3), 255, np.uint8)
    at = TR.lattice(P, 4)
    assert at.tolist() == [2, 6, 10, 14]
    tiles[1, 2, 2] = tiles[1, 6, 10] = 0                      # two lattice pixels: 2 / 16 > 0.1
    tiles[2, 2, 2] = 0                                        # one: 1 / 16 <= 0.1
    tiles[3, 3, 3] = tiles[3, 0, 0] = tiles[3, 15, 15] = 0    # dark pixels beside the lattice count nothing
    tiles[4] = 99                                             # g == 99 everywhere
    counts, flags, order, m, slots = TR.tissue(tiles, 100)
    assert counts.tolist() == [0, 2, 1, 0, 16] and flags.tolist() == [0, 1, 0, 0, 1]
    assert order.tolist() == [1, 4] and m == 2 and slots.tolist() == [-1, 0, -1, -1, 1]
    assert TR.tissue(tiles, 99)[0].tolist() == [0, 2, 1, 0, 0], "g == t is background: the comparison is strict"
    assert TR.tissue_counts(tiles, 100, 1).tolist() == [0, 2, 1, 3, 256]
    table = TR.to_tensor_table("float16")
    x = TR.encoder_input(tiles, order, 1, 1, table)
    assert x.shape == (1, 3, P, P) and (x == np.float32(np.float16(99 / 255))).all()
    rows = TR.scatter_rows(np.array([[1.5, 2.5, 0, 0], [3, 4, 5, 65520.0]], np.float32), slots, 4, np.float16)
    assert rows.dtype == np.float16 and rows[1].tolist() == [1.5, 2.5, 0, 0] and rows[4, :3].tolist() == [3, 4, 5] and np.isinf(rows[4, 3])
    assert not rows[[0, 2, 3]].any() and not np.signbit(rows[0]).any()
    image = np.arange(2 * P * 3 * P * 3, dtype=np.uint32).astype(np.uint8).reshape(2 * P, 3 * P, 3)
    assert np.array_equal(TR.cell_tiles(image, P)[4], image[P:2 * P, P:2 * P]) and np.array_equal(TR.cell_tiles(image, P, [[1, 2]])[0], image[P:, 2 * P:])


# ------------------------------------------------------------------------------------------------
# the C surface and every refusal in front of a launch
# ------------------------------------------------------------------------------------------------
ENTRIES = (("paths_grey_histogram", 6), ("paths_tile_tissue", 9), ("paths_tile_compact", 8), ("paths_tiles_to_input", 10), ("paths_scatter_rows", 9))


def test_header_declares_and_library_exports_the_tile_entry_points():
    from paths_amd import _lib
    assert _lib.ABI_VERSION == 3
    for name, nargs in ENTRIES:
        assert name in _lib.DECLARATIONS, f"{name} is not declared in include/paths_hip.h"
        res, args = _lib.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    res, args = _lib.DECLARATIONS["paths_grey_histogram_workspace"]
    assert res is ctypes.c_int64 and len(args) == 1
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name, _ in ENTRIES) and lib.paths_abi_version() == 3
    assert lib.paths_grey_histogram_workspace(3) == (3 * 64 * 256 + 3) * 4 and lib.paths_grey_histogram_workspace(0) == 0
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    table = text[text.index(" * pixels to encoder input"):text.index("#ifndef PATHS_HIP_H")]
    for name, _ in ENTRIES:
        assert name + " " in table, f"{name} has no line in the header's undefined-memory table"
    assert "outside the P x 3P window" in table and "beyond m" in table
    import __graft_entry__ as g
    assert "tiles.hip" in g.SOURCES


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)
    hist = lambda images=A, n=1, partials=A, counts=A, status=A: lib.paths_grey_histogram(images, n, partials, counts, status, None)
    for kw, word in ((dict(n=0), b"n_images = 0"), (dict(n=1025), b"n_images = 1025"), (dict(images=None), b"null"), (dict(counts=None), b"null"),
                     (dict(status=None), b"null"), (dict(counts=A + 4), b"alignment"), (dict(status=A + 2), b"alignment")):
        assert hist(**kw) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())
    tis = lambda tiles=A, n=4, P=64, s=4, t=100, need=26, counts=A, flags=A: lib.paths_tile_tissue(tiles, n, P, s, t, need, counts, flags, None)
    for kw, word in ((dict(n=0), b"n = 0"), (dict(n=65537), b"n = 65537"), (dict(P=8), b"P = 8"), (dict(P=40), b"P = 40"), (dict(P=1040), b"P = 1040"),
                     (dict(s=0), b"stride = 0"), (dict(s=3), b"stride = 3"), (dict(s=128), b"stride = 128"), (dict(t=-1), b"threshold"),
                     (dict(t=257), b"threshold"), (dict(need=-1), b"pass_count"), (dict(need=258), b"pass_count"), (dict(tiles=None), b"null"),
                     (dict(flags=None), b"null"), (dict(counts=A + 2), b"alignment")):
        assert tis(**kw) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())
    com = lambda flags=A, counts=A, n=4, order=A, m=A, slot=A, status=A: lib.paths_tile_compact(flags, counts, n, order, m, slot, status, None)
    for kw, word in ((dict(n=0), b"n = 0"), (dict(n=65537), b"n = 65537"), (dict(order=None), b"null"), (dict(status=None), b"null"), (dict(m=A + 2), b"alignment")):
        assert com(**kw) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())
    inp = lambda tiles=A, n=8, order=A, first=2, count=3, P=32, table=A, eb=2, out=A: lib.paths_tiles_to_input(tiles, n, order, first, count, P, table, eb, out, None)
    for kw, word in ((dict(n=0), b"n = 0"), (dict(P=24), b"P = 24"), (dict(first=-1), b"first"), (dict(count=0), b"first"), (dict(first=6), b"first"),
                     (dict(eb=1), b"elem_bytes = 1"), (dict(eb=8), b"elem_bytes = 8"), (dict(table=None), b"null"), (dict(out=None), b"null"),
                     (dict(out=A + 8), b"alignment")):
        assert inp(**kw) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())
    sca = lambda enc=A, ef=0, m=2, slot=A, n=4, dim=128, of=0, out=A: lib.paths_scatter_rows(enc, ef, m, slot, n, dim, of, out, None)
    for kw, word in ((dict(n=0), b"n = 0"), (dict(m=5), b"m = 5"), (dict(m=-1), b"m = -1"), (dict(dim=0), b"dim = 0"), (dict(dim=6), b"dim = 6"),
                     (dict(enc=None), b"null"), (dict(slot=None), b"null"), (dict(out=None), b"null"), (dict(out=A + 8), b"alignment"),
                     (dict(enc=A + 8), b"alignment")):
        assert sca(**kw) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())


def _batch(n, P, row_bytes=None, dtype=torch.uint8):
    """A CPU tensor [n, P, P, 3] whose rows are row_bytes apart."""
    row_bytes = row_bytes or 3 * P
    return torch.zeros((n, P, row_bytes), dtype=dtype)[:, :, :3 * P].unflatten(2, (P, 3))


def test_tile_encoder_refuses_before_any_launch(monkeypatch):
    from paths_amd import _lib, pixels
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    model = lambda x: x.flatten(1)[:, :128]
    read = lambda level, cells: _batch(int(cells.shape[0]), 16)
    cells = torch.zeros((3, 2), dtype=torch.int64)
    for bad in (20, 8, 0, 1040, 16.0, True):
        with pytest.raises(ValueError, match="patch_size must be a multiple of 16"):
            pixels.TileEncoder(read, model, 128, 100, patch_size=bad)
    for P, s in ((48, 5), (16, 32), (64, 0), (64, -4), (64, 2.0)):
        with pytest.raises(ValueError, match="stride must be a positive integer that divides patch_size"):
            pixels.TileEncoder(read, model, 128, 100, patch_size=P, stride=s)
    for kw, word in ((dict(dim=6), "dim"), (dict(threshold=300), "threshold"), (dict(threshold=99.5), "threshold"), (dict(batch=0), "batch"),
                     (dict(dtype=torch.float64), "feature grids"), (dict(input_dtype=torch.float64), "float32, float16 or bfloat16"),
                     (dict(table=torch.zeros(256, 3)), "table"), (dict(tissue_threshold=float("nan")), "tissue_threshold")):
        args = dict(dim=128, threshold=100, patch_size=16)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            pixels.TileEncoder(read, model, **args)
    enc = lambda read: pixels.TileEncoder(read, model, 128, 100, patch_size=16)
    # a row stride that is no multiple of 16, a tile stride that is none, a misaligned first byte
    with pytest.raises(ValueError, match=r"row stride \(52 bytes\) must be a multiple of 16"):
        enc(lambda level, cells: _batch(3, 16, 52))(0, cells)
    with pytest.raises(ValueError, match=r"row stride \(40 bytes\)"):
        enc(lambda level, cells: (torch.zeros(3, dtype=torch.int64), 40))(0, cells)
    with pytest.raises(ValueError, match="address of every tile must be a multiple of 16"):
        enc(lambda level, cells: torch.zeros((4096,), dtype=torch.uint8).as_strided((3, 16, 16, 3), (776, 48, 3, 1)))(0, cells)
    whole = torch.zeros((3 * 16 * 48 + 16,), dtype=torch.uint8)
    off = (-whole.data_ptr()) % 16 + 8
    with pytest.raises(ValueError, match="address of every tile must be a multiple of 16"):
        enc(lambda level, cells: whole[off:off + 3 * 16 * 48].view(3, 16, 16, 3))(0, cells)
    # more tiles than one call takes
    many = torch.zeros((65537, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="65537 tiles; one call takes 1 to 65536"):
        enc(lambda level, cells: (torch.zeros(65537, dtype=torch.int64), 48))(0, many)
    # tiles of another width, another dtype, fewer tiles than cells, no tiles at all
    with pytest.raises(ValueError, match="32 pixels wide, patch_size is 16"):
        enc(lambda level, cells: _batch(3, 32))(0, cells)
    with pytest.raises(ValueError, match="uint8 tensor"):
        enc(lambda level, cells: _batch(3, 16, dtype=torch.int16))(0, cells)
    with pytest.raises(ValueError, match="the tiles of the 3 cells asked, got 2"):
        enc(lambda level, cells: _batch(2, 16))(0, cells)
    with pytest.raises(ValueError, match="the tiles of the 3 cells asked"):
        enc(lambda level, cells: None)(0, cells)
    # and last, with everything else in order, the device
    with pytest.raises(_lib.PathsHipError, match="GPU only"):
        enc(read)(0, cells)
    with pytest.raises(_lib.PathsHipError, match="GPU only"):
        enc(lambda level, cells: (torch.zeros(3, dtype=torch.int64), 64))(0, cells)
    assert launched == []


def test_public_functions_refuse_before_any_launch(monkeypatch):
    from paths_amd import _lib, pixels
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    image = lambda rows, cols, pad=0: torch.zeros((rows, 3 * cols + pad), dtype=torch.uint8)[:, :3 * cols].unflatten(1, (cols, 3))
    for bad, word in ((image(16, 17), "row stride"), (image(16, 16).to(torch.int32), "uint8"), (torch.zeros((16, 16, 4), dtype=torch.uint8)[..., :3], "strides"),
                      (torch.zeros((16, 48), dtype=torch.uint8), "uint8 tensor")):
        with pytest.raises(ValueError, match=word):
            pixels.grey_histogram([bad])
    with pytest.raises(ValueError, match="0 images"):
        pixels.grey_histogram([])
    with pytest.raises(_lib.PathsHipError, match="GPU only"):
        pixels.grey_histogram([image(16, 16), image(32, 20, pad=4)])
    with pytest.raises(ValueError, match="patch_size is required"):
        pixels.tile_tissue((torch.zeros(3, dtype=torch.int64), 48), 100)
    with pytest.raises(ValueError, match="stride must be a positive integer that divides"):
        pixels.tile_tissue(_batch(3, 48), 100, stride=5)
    with pytest.raises(ValueError, match="threshold"):
        pixels.tile_tissue(_batch(3, 48), -1)
    with pytest.raises(ValueError, match="LevelImages: image 1 is 40 x 32"):
        pixels.LevelImages([image(16, 32), image(40, 32)], patch_size=8 * 2)
    order, table = torch.zeros(3, dtype=torch.int32), pixels.to_tensor_table(torch.float32)
    for kw, word in ((dict(first=2, count=2), "outside the 3 tiles"), (dict(count=0), "outside the 3 tiles"), (dict(order=order.long()), "order"),
                     (dict(order=order[:2]), "order"), (dict(table=table.double()), "table"), (dict(table=table.t()), "table")):
        args = dict(order=order, first=0, count=3, table=table)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            pixels.encoder_input(_batch(3, 16), **args)
    slots = torch.zeros(4, dtype=torch.int32)
    for args, word in (((None, slots, 4, 6), "dim"), ((None, slots, 5, 8), "slots"), ((torch.zeros(2, 12), slots, 4, 8), "encoded"),
                       ((torch.zeros(5, 8), slots, 4, 8), "encoded"), ((torch.zeros(2, 8, dtype=torch.bfloat16), slots, 4, 8), "encoded")):
        with pytest.raises(ValueError, match=word):
            pixels.scatter_rows(*args)
    with pytest.raises(ValueError, match="feature grids"):
        pixels.scatter_rows(None, slots, 4, 8, torch.float64)
    assert launched == []


def test_level_images_names_windows_and_copies_nothing():
    from paths_amd import pixels
    P = 16
    whole = torch.zeros((2 * P, 3 * P * 3 + 16 + 15), dtype=torch.uint8)
    shift = (-whole.data_ptr()) % 16
    im = whole.view(-1)[shift:shift + 2 * P * (3 * P * 3 + 16)].view(2 * P, 3 * P * 3 + 16)[:, :3 * P * 3].unflatten(1, (3 * P, 3))
    assert im.stride(0) == 160 and im.data_ptr() % 16 == 0
    r = pixels.LevelImages([im], patch_size=P)
    assert r.shape(0) == (2, 3)
    addresses, stride = r(0, torch.tensor([[0, 0], [1, 2], [0, 1]]))
    assert stride == 160 and addresses.dtype == torch.int64
    assert (addresses - im.data_ptr()).tolist() == [0, P * 160 + 2 * 48, 48]
