"""CPU-only tests of the resize in front of the encoder (paths_amd.pixels: resize_coefficients, crop_offset, encoder_input(resize=...);
csrc/tile_resize.hip's entry point): the NumPy contract (tests/resize_ref.py) against Pillow bit for bit and against torch's uint8
antialias resize within one byte, literals that pin the contract where Pillow is absent, the Python side against the contract, every
refusal in front of a launch, and the C surface.  No kernel runs here."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import resize_ref as RR

CASES = [(32, 28), (64, 56), (16, 24), (48, 16), (32, 32), (256, 224)]
FILTERS = ["bicubic", "bilinear"]


def noisy_tile(P, seed):
    """Random bytes with a block of 0 / 255 noise and a 255 block inside a 0 block: the cubic overshoots at such edges, so both passes
    clip at both ends (:func:`unclipped_range`)."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (P, P, 3), dtype=np.uint8)
    t[1:P // 2, 2:P // 2 + 3] = rng.integers(0, 2, (P // 2 - 1, P // 2 + 1, 3), dtype=np.uint8) * 255
    t[P // 2:, : P // 2] = 0
    t[P // 2 + P // 8: P - P // 8, P // 8: P // 2 - P // 8] = 255
    return t


def unclipped_range(image, S, interpolation):
    """The smallest and largest value of one pass along axis 0 BEFORE its clip."""
    bounds, k, _ = RR.coefficients(image.shape[0], S, interpolation)
    sums = [((1 << 21) + sum(image[lo + t].astype(np.int64) * int(k[i, t]) for t in range(cnt))) >> 22 for i, (lo, cnt) in enumerate(bounds)]
    return int(np.min(sums)), int(np.max(sums))


# ------------------------------------------------------------------------------------------------
# the contract against Pillow and torch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("P, S", CASES)
def test_the_contract_is_pillows_resize_bit_for_bit(P, S, interpolation):
    Image = pytest.importorskip("PIL.Image")
    tile = noisy_tile(P, P + S)
    want = np.asarray(Image.fromarray(tile).resize((S, S), Image.BICUBIC if interpolation == "bicubic" else Image.BILINEAR))
    got = RR.resize_u8(tile, S, interpolation)
    assert got.dtype == np.uint8 and got.shape == (S, S, 3) and np.array_equal(got, want)
    if P == S:
        assert np.array_equal(got, tile), "the identity"
    elif interpolation == "bicubic":                             # (the bilinear weights are not negative: nothing to clip)
        bounds, k, _ = RR.coefficients(P, S, interpolation)
        across = tile.transpose(1, 0, 2)                         # (the horizontal pass runs along axis 1: axis 0 of the transpose)
        for image in (across, RR.one_pass(across, bounds, k).transpose(1, 0, 2)):
            lo, hi = unclipped_range(image, S, interpolation)
            assert lo < 0 and hi > 255, "both clips act"


@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("P, S", CASES)
def test_the_contract_is_within_one_byte_of_torchs_uint8_resize(P, S, interpolation):
    tile = noisy_tile(P, P + S)
    x = torch.from_numpy(tile).permute(2, 0, 1)[None].contiguous()
    theirs = torch.nn.functional.interpolate(x, size=(S, S), mode=interpolation, antialias=True)[0].permute(1, 2, 0).numpy()
    d = np.abs(RR.resize_u8(tile, S, interpolation).astype(np.int32) - theirs.astype(np.int32))
    print(f"{P} -> {S} {interpolation}: {100 * float((d != 0).mean()):.2f} % of the bytes differ from torch's, max {int(d.max())}")
    assert int(d.max()) <= 1


def test_the_sums_of_the_contract_fit_int32_and_the_products_24_bits():
    for P, S in CASES + [(64, 17), (1024, 256), (16, 1024)]:
        for interpolation in FILTERS:
            _, k, _ = RR.coefficients(P, S, interpolation)
            assert 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 1 << 31 and int(np.abs(k).max()) < 1 << 23


# ------------------------------------------------------------------------------------------------
# literals
# ------------------------------------------------------------------------------------------------
def test_literals_of_the_contract():
    assert RR.coefficients(256, 224, "bicubic")[2] == 7 and RR.coefficients(256, 224, "bilinear")[2] == 5
    assert RR.coefficients(48, 16, "bicubic")[2] == 13 and RR.coefficients(16, 24, "bicubic")[2] == 5
    bounds, k, taps = RR.coefficients(32, 32, "bicubic")
    for i in range(32):
        assert np.count_nonzero(k[i]) == 1 and k[i].sum() == 1 << 22 and bounds[i, 0] + int(np.argmax(k[i])) == i, "the identity: one coefficient"
    assert RR.crop_offset(28, 16) == 6 and RR.crop_offset(17, 16) == 0 and RR.crop_offset(19, 16) == 2 and RR.crop_offset(224, 224) == 0
    # two rows of bicubic 32 -> 28, as tests/resize_ref.py gave them after it equalled Pillow
    bounds, k, taps = RR.coefficients(32, 28, "bicubic")
    assert taps == 7 and k.shape == (28, 7) and bounds.shape == (28, 2)
    assert bounds[0].tolist() == [0, 3] and k[0].tolist() == [3739072, 581941, -126709, 0, 0, 0, 0]
    assert bounds[13].tolist() == [13, 5] and k[13].tolist() == [-123985, 569430, 3658688, 142921, -52750, 0, 0]
    assert k[0].sum() == k[13].sum() == 1 << 22
    # a constant tile stays constant; a table lookup follows the crop
    tile = np.full((32, 32, 3), 201, np.uint8)
    assert (RR.resize_u8(tile, 28) == 201).all()
    table = np.arange(768, dtype=np.float32).reshape(3, 256)
    x = RR.resized_input(tile[None], [0], 0, 1, table, 28, 16)
    assert x.shape == (1, 3, 16, 16) and [float(x[0, c, 0, 0]) for c in range(3)] == [201.0, 457.0, 713.0]


# ------------------------------------------------------------------------------------------------
# the Python side
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolation", FILTERS)
def test_resize_coefficients_equal_the_contract(interpolation):
    from paths_amd import pixels
    for P, S in CASES + [(64, 17), (16, 64), (1024, 256)]:
        bounds, coef, taps = pixels.resize_coefficients(P, S, interpolation)
        want = RR.coefficients(P, S, interpolation)
        assert taps == want[2] and bounds.dtype == coef.dtype == torch.int32 and bounds.device.type == coef.device.type == "cpu"
        assert tuple(bounds.shape) == (S, 2) and tuple(coef.shape) == (S, taps) and bounds.is_contiguous() and coef.is_contiguous()
        assert np.array_equal(bounds.numpy(), want[0]) and np.array_equal(coef.numpy(), want[1])
    for S, C in ((28, 16), (17, 16), (19, 16), (224, 224), (256, 224), (21, 16)):
        assert pixels.crop_offset(S, C) == RR.crop_offset(S, C)


def _batch(n, P):
    return torch.zeros((n, P, P, 3), dtype=torch.uint8)


def test_every_refusal_comes_before_any_launch(monkeypatch):
    from paths_amd import _lib, pixels
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    order, table = torch.zeros(3, dtype=torch.int32), pixels.to_tensor_table(torch.float16)
    model, read = (lambda x: x.flatten(1)[:, :128]), (lambda level, cells: _batch(int(cells.shape[0]), 64))
    bad = ((dict(resize=28.0), "resize must be an integer"), (dict(resize=True), "resize must be an integer"), (dict(resize=8), "resize must be an integer"),
           (dict(resize=1040), "resize must be an integer"), (dict(resize="224"), "resize must be an integer"),
           (dict(resize=32, crop=16.0), "crop must be an integer"), (dict(resize=32, crop=0), "crop must be an integer"),
           (dict(resize=32, crop=24), "crop must be a multiple of 16"), (dict(resize=32, crop=48), r"crop \(48\) must not exceed resize \(32\)"),
           (dict(resize=20), "crop must be a multiple of 16"),                                   # (crop defaults to resize)
           (dict(resize=15, crop=16), "resize must be an integer"), (dict(resize=16, crop=16, interpolation="lanczos"), "interpolation"),
           (dict(resize=48, interpolation="nearest"), "interpolation"), (dict(interpolation="box"), "interpolation"),
           (dict(crop=16), "needs resize"))
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            pixels.encoder_input(_batch(3, 64), order, 0, 3, table, **kw)
        with pytest.raises(ValueError, match=word):
            pixels.TileEncoder(read, model, 128, 100, patch_size=64, **kw)
    # a tile more than four times the resize
    with pytest.raises(ValueError, match=r"256-pixel tile is more than 4 times resize \(48\)"):
        pixels.encoder_input(_batch(3, 256), order, 0, 3, table, resize=48)
    with pytest.raises(ValueError, match="more than 4 times resize"):
        pixels.TileEncoder(read, model, 128, 100, patch_size=256, resize=48, crop=16)
    for args in ((0, 16), (16, 0), (16, 2048), (80, 16), (16.0, 16), (True, 16)):
        with pytest.raises(ValueError, match="resize_coefficients"):
            pixels.resize_coefficients(*args)
    with pytest.raises(ValueError, match="interpolation"):
        pixels.resize_coefficients(32, 28, "lanczos")
    # the checks of the unresized call still come first, and with everything in order only the device is missing
    with pytest.raises(ValueError, match="outside the 3 tiles"):
        pixels.encoder_input(_batch(3, 64), order, 2, 2, table, resize=32)
    with pytest.raises(_lib.PathsHipError, match="GPU only"):
        pixels.encoder_input(_batch(3, 64), order, 0, 3, table, resize=56, crop=48)
    enc = pixels.TileEncoder(read, model, 128, 100, patch_size=64, resize=56, crop=48, interpolation="bilinear")
    assert (enc.resize, enc.crop, enc.interpolation) == (56, 48, "bilinear")
    assert pixels.TileEncoder(read, model, 128, 100, patch_size=64, resize=48).crop == 48
    plain = pixels.TileEncoder(read, model, 128, 100, patch_size=64)
    assert (plain.resize, plain.crop) == (None, None)
    assert launched == []


def _recorded(monkeypatch, **kw):
    """The launches of one TileEncoder call on CPU tensors, every tile tissue: ``_lib.call`` records instead of launching (the
    compaction's stand-in writes order, m, slots and status through the addresses it is given), the device checks are switched off."""
    from paths_amd import _lib, pixels
    launched, shapes = [], []

    def call(name, *a):
        launched.append((name, len(a), a))
        if name == "paths_tile_compact":
            n = a[2]
            ids = (ctypes.c_int32 * n)(*range(n))
            ctypes.memmove(a[3], ids, 4 * n)
            ctypes.memmove(a[5], ids, 4 * n)
            ctypes.memmove(a[4], (ctypes.c_int32 * 1)(n), 4)
            ctypes.memmove(a[6], (ctypes.c_int32 * 1)(0), 4)

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "require_cuda", lambda *t: None)
    monkeypatch.setattr(_lib, "stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())

    def model(x):
        shapes.append(tuple(x.shape))
        return torch.zeros((x.shape[0], 128))

    enc = pixels.TileEncoder(lambda level, cells: _batch(int(cells.shape[0]), 32), model, 128, 100, patch_size=32, batch=4, **kw)
    rows = enc(0, torch.zeros((6, 2), dtype=torch.int64))
    assert tuple(rows.shape) == (6, 128) and enc.stats == {"requested": {0: 6}, "tissue": {0: 6}, "model_calls": {0: 2}}
    return launched, shapes


def test_without_resize_the_encoder_launches_what_it_launched_before(monkeypatch):
    launched, shapes = _recorded(monkeypatch)
    assert [(name, nargs) for name, nargs, _ in launched] == [("paths_tile_tissue", 9), ("paths_tile_compact", 8), ("paths_tiles_to_input", 10),
                                                             ("paths_tiles_to_input", 10), ("paths_scatter_rows", 9)]
    a, b = launched[2][2], launched[3][2]
    assert a[1:2] + a[3:6] + a[7:8] == (6, 0, 4, 32, 2) and b[1:2] + b[3:6] + b[7:8] == (6, 4, 2, 32, 2)      # n, first, count, P, elem_bytes
    assert shapes == [(4, 3, 32, 32), (2, 3, 32, 32)]
    launched, shapes = _recorded(monkeypatch, resize=None, crop=None, interpolation="bilinear")
    assert [name for name, _, _ in launched].count("paths_tiles_to_input") == 2 and shapes == [(4, 3, 32, 32), (2, 3, 32, 32)]


def test_with_resize_the_encoder_makes_the_new_launch(monkeypatch):
    launched, shapes = _recorded(monkeypatch, resize=28, crop=16)
    assert [(name, nargs) for name, nargs, _ in launched] == [("paths_tile_tissue", 9), ("paths_tile_compact", 8), ("paths_tiles_resize_to_input", 15),
                                                             ("paths_tiles_resize_to_input", 15), ("paths_scatter_rows", 9)]
    a, b = launched[2][2], launched[3][2]
    assert a[1:2] + a[3:8] + a[10:11] + a[12:13] == (6, 0, 4, 32, 28, 16, 7, 2)           # n, first, count, P, S, C, taps, elem_bytes
    assert b[3:5] == (4, 2) and (a[8], a[9]) == (b[8], b[9]), "one pair of device tables serves every chunk"
    assert shapes == [(4, 3, 16, 16), (2, 3, 16, 16)]
    assert launched[0][2][2:4] == (32, 4), "the tissue decision looks at the tile's own pixels"


# ------------------------------------------------------------------------------------------------
# the C surface
# ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    from paths_amd import _lib
    assert _lib.ABI_VERSION == 3 and _lib.load().paths_abi_version() == 3
    name = "paths_tiles_resize_to_input"
    assert name in _lib.DECLARATIONS, f"{name} is not declared in include/paths_hip.h"
    res, args = _lib.DECLARATIONS[name]
    assert res is ctypes.c_int and len(args) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    table = text[text.index(" * pixels to encoder input"):text.index("#ifndef PATHS_HIP_H")]
    assert name + " " in table, f"{name} has no line in the header's undefined-memory table"
    import __graft_entry__ as g
    assert "tile_resize.hip" in g.SOURCES and "tiles.hip" in g.SOURCES


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)

    def entry(tiles=A, n=8, order=A, first=2, count=3, P=32, S=28, C=16, bounds=A, coef=A, taps=7, table=A, eb=2, out=A):
        return lib.paths_tiles_resize_to_input(tiles, n, order, first, count, P, S, C, bounds, coef, taps, table, eb, out, None)

    cases = ((dict(n=0), b"n = 0"), (dict(n=65537), b"n = 65537"), (dict(first=-1), b"first"), (dict(count=0), b"first"), (dict(first=6), b"first"),
             (dict(P=24), b"P = 24"), (dict(P=8), b"P = 8"), (dict(P=1040), b"P = 1040"),
             (dict(S=15, C=16, taps=13), b"S = 15, C = 16"), (dict(S=28, C=32), b"S = 28, C = 32"), (dict(C=0), b"C = 0"),
             (dict(S=1040, C=16, taps=5), b"S = 1040"), (dict(C=24), b"C = 24 must be a multiple of 16"),
             (dict(P=128, S=28, taps=17), b"P = 128 is more than 4 S"), (dict(P=80, S=16, taps=17), b"more than 4 S"),
             (dict(taps=9), b"taps = 9"), (dict(taps=3), b"taps = 3"), (dict(taps=19), b"taps = 19"), (dict(taps=0), b"taps = 0"),
             (dict(taps=6), b"taps = 6"), (dict(P=48, S=16, taps=11), b"takes 7 (bilinear) or 13 (bicubic)"),
             (dict(eb=1), b"elem_bytes = 1"), (dict(eb=8), b"elem_bytes = 8"),
             (dict(tiles=None), b"null"), (dict(order=None), b"null"), (dict(bounds=None), b"null"), (dict(coef=None), b"null"),
             (dict(table=None), b"null"), (dict(out=None), b"null"),
             (dict(out=A + 8), b"alignment"), (dict(tiles=A + 4), b"alignment"), (dict(order=A + 2), b"alignment"), (dict(bounds=A + 2), b"alignment"),
             (dict(coef=A + 1), b"alignment"), (dict(table=A + 1), b"alignment"))
    for kw, word in cases:
        assert entry(**kw) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())
