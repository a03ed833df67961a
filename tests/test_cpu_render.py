"""CPU-only tests of the overlays (paths_amd.heatmap.render / save_png, paths_amd.colormaps, csrc/raster.hip's two render entries):
every refusal that happens before a launch, the colour tables, the PNG writer, the C surface, and the NumPy restatement
(tests/render_ref.py) against the reference's recipe on heatmap.importance_map.  No kernel runs here."""
import ctypes
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests.test_cpu_raster import PATCH, _cpu_trace, random_hierarchy


def test_render_rejects_before_any_launch(monkeypatch):
    from paths_amd import _lib, heatmap as hm
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    grids = [(3, 5), (2, 2)]                                         # _cpu_trace: L = 3, B = 2: f = 4
    thumbs = lambda c=4: [torch.zeros((g[0] * 4 * c, g[1] * 4 * c, 3), dtype=torch.uint8) for g in grids]
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="cell_px"):
            hm.render(_cpu_trace(), grids, cell_px=bad)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            hm.render(_cpu_trace(), grids, alpha=bad)
    for bad in (3, -1):
        with pytest.raises(ValueError, match="level .* out of range"):
            hm.render(_cpu_trace(), grids, level=bad)
    with pytest.raises(ValueError, match="fold is the weight of the folded map"):
        hm.render(_cpu_trace(), grids, level=1, fold=0.5)
    with pytest.raises(ValueError, match="fold is a weight or None"):
        hm.render(_cpu_trace(), grids, fold=False)
    for bad in (np.zeros((256, 4), np.uint8), np.zeros((255, 3), np.uint8), np.zeros((256, 3), np.float32), torch.zeros((256, 3)), "jet"):
        with pytest.raises(ValueError, match="cmap"):
            hm.render(_cpu_trace(), grids, cmap=bad)
    wrong = thumbs()
    wrong[1] = wrong[1][:-1]
    with pytest.raises(ValueError, match="thumbnail 1 must be a uint8 tensor"):
        hm.render(_cpu_trace(), grids, thumbnails=wrong)
    with pytest.raises(ValueError, match="thumbnail 0"):
        hm.render(_cpu_trace(), grids, thumbnails=thumbs(3))                                  # (the shape of another cell_px)
    with pytest.raises(ValueError, match="thumbnail 0"):
        hm.render(_cpu_trace(), grids, thumbnails=[t.to(torch.int16) for t in thumbs()])
    with pytest.raises(ValueError, match="thumbnail 0"):                                      # pixel stride 4
        hm.render(_cpu_trace(), grids, thumbnails=[torch.zeros(t.shape[:2] + (4,), dtype=torch.uint8)[..., :3] for t in thumbs()])
    with pytest.raises(ValueError, match="1 thumbnails for the 2 slides"):
        hm.render(_cpu_trace(), grids, thumbnails=thumbs()[:1])
    for bad in ([3], [0, -1], (1, 7)):
        with pytest.raises(ValueError, match="outline names level"):
            hm.render(_cpu_trace(), grids, outline=bad)
    for bad in (dict(vmin=[1.0, 2.0, 3.0]), dict(vmax=float("inf")), dict(center=float("nan")), dict(outline_rgb=(0, 0, 256)),
                dict(background=(1, 2))):
        with pytest.raises(ValueError, match="render"):
            hm.render(_cpu_trace(), grids, **bad)
    # the checks rasterize makes, through the same code
    with pytest.raises(ValueError, match="kind must be one of"):
        hm.render(_cpu_trace(), grids, kind="removed")
    with pytest.raises(ValueError, match="dtype"):
        hm.render(_cpu_trace(), grids, dtype=torch.float16)
    with pytest.raises(ValueError, match="3 grids for the 2 slides"):
        hm.render(_cpu_trace(), grids + [(1, 1)])
    with pytest.raises(KeyError, match="level 0 carries no grad_norm"):
        hm.render(_cpu_trace(), grids, kind="grad_norm")
    # and last, with everything else in order, the device
    with pytest.raises(_lib.PathsHipError, match="GPU only"):
        hm.render(_cpu_trace(), grids, thumbnails=thumbs(), outline=[0, 2], cmap="bwr", level=2, vmin=[0.0, 1.0], center=0.0)
    assert launched == []
    assert "out of scope" in hm.__doc__ and "drawing is out of scope" not in hm.__doc__
    for word in ("nearest-neighbour", "integer blending", "one-pixel outlines", "colour bar"):
        assert word in hm.render.__doc__, word


def test_viridis_is_matplotlibs_bytes():
    from paths_amd import colormaps
    table = colormaps.viridis()
    assert table.dtype == np.uint8 and table.shape == (256, 3)
    assert tuple(table[0]) == (68, 1, 84) and tuple(table[255]) == (253, 231, 36)
    cm = pytest.importorskip("matplotlib.cm")
    assert np.array_equal(table, cm.viridis(np.arange(256), bytes=True)[:, :3])


def test_bwr_is_its_docstring_and_tables_are_checked():
    from paths_amd import colormaps
    table = colormaps.bwr()
    assert table.dtype == np.uint8 and np.array_equal(table, RR.bwr())
    assert table[[0, 127, 128, 255]].tolist() == [[0, 0, 255], [255, 255, 255], [255, 255, 255], [255, 0, 0]]
    assert "k * 255 // 127" in colormaps.__doc__ and "(255 - k) * 255 // 127" in colormaps.__doc__
    own = np.arange(768, dtype=np.uint8).reshape(256, 3)
    assert np.array_equal(colormaps.colour_table(own), own) and np.array_equal(colormaps.colour_table(torch.from_numpy(own)), own)
    assert np.array_equal(colormaps.colour_table("viridis"), colormaps.viridis())


def decode_png(data):
    """8-bit RGB, filter 0 only, every CRC checked -> uint8 [H, W, 3] and the chunk names."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        tag, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        at += 12 + n
    assert at == len(data)
    names = [t for t, _ in chunks]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()                                       # filter type 0 on every row
    return raw[:, 1:].reshape(h, w, 3), names


def test_save_png_round_trips(tmp_path):
    from paths_amd import heatmap as hm
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 3), (7, 5, 3), (12, 40, 3)):
        image = rng.integers(0, 256, shape, dtype=np.uint8)
        for given in (image, torch.from_numpy(image), torch.from_numpy(np.pad(image, ((0, 0), (0, 3), (0, 0))))[:, :shape[1]]):
            path = tmp_path / "image.png"
            hm.save_png(path, given)
            back, names = decode_png(path.read_bytes())
            assert names == [b"IHDR", b"IDAT", b"IEND"] and np.array_equal(back, image)
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), image)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="save_png"):
            hm.save_png(tmp_path / "bad.png", bad)


def test_header_declares_and_library_exports_the_render_entry_points():
    from paths_amd import _lib
    assert _lib.ABI_VERSION == 3
    for name, nargs in (("paths_render_range", 16), ("paths_render_rgb", 22)):
        assert name in _lib.DECLARATIONS, f"{name} is not declared in include/paths_hip.h"
        res, args = _lib.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == nargs
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "paths_render_range") and hasattr(raw, "paths_render_rgb")
    assert lib.paths_abi_version() == 3
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    table = text[text.index(" * heat-map rasters"):text.index(" * row cache of on-demand slides")]
    assert "paths_render_range " in table and "paths_render_rgb " in table


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)
    rr = lambda table, gx, gy, L, B, GX, GY, level, raster, f64, ldo, center, partial, rng, status: lib.paths_render_range(
        table, gx, gy, L, B, GX, GY, level, raster, f64, ldo, center, partial, rng, status, None)
    ok = dict(table=A, gx=A, gy=A, L=3, B=3, GX=4, GY=5, level=-1, raster=A, f64=1, ldo=20, center=None, partial=A, rng=A, status=A)
    for change, word in ((dict(table=None), b"null"), (dict(raster=None), b"null"), (dict(partial=None), b"null"), (dict(rng=None), b"null"),
                         (dict(status=None), b"null"), (dict(B=0), b"B = 0"), (dict(L=0), b"L = 0"), (dict(L=9), b"L = 9"),
                         (dict(level=3), b"level = 3"), (dict(level=-2), b"level = -2"), (dict(GX=0), b"extent"), (dict(ldo=19), b"stride"),
                         (dict(raster=A + 4), b"alignment"), (dict(center=A + 4), b"alignment"), (dict(rng=A + 4), b"alignment"),
                         (dict(status=A + 2), b"alignment")):
        assert rr(**{**ok, **change}) == -1 and word in lib.paths_last_error(), (change, lib.paths_last_error())
    rg = lambda table, gx, gy, L, B, GX, GY, level, raster, f64, ldo, rng, colours, thumbs, c, a, lines, out, ldp: lib.paths_render_rgb(
        table, gx, gy, L, B, GX, GY, level, raster, f64, ldo, rng, colours, thumbs, c, a, lines, 0, 0xFFFFFF, out, ldp, None)
    ok = dict(table=A, gx=A, gy=A, L=3, B=3, GX=4, GY=5, level=1, raster=A, f64=0, ldo=20, rng=A, colours=A, thumbs=None, c=4, a=128, lines=7,
              out=A, ldp=240)
    for change, word in ((dict(table=None), b"null"), (dict(rng=None), b"null"), (dict(colours=None), b"null"), (dict(out=None), b"null"),
                         (dict(B=70000), b"B = 70000"), (dict(L=9), b"L = 9"), (dict(level=3), b"level = 3"), (dict(GY=0), b"extent"),
                         (dict(ldo=16), b"stride ldo"), (dict(c=0), b"cell_px = 0"), (dict(c=65), b"cell_px = 65"), (dict(a=-1), b"alpha255"),
                         (dict(a=256), b"alpha255"), (dict(lines=8), b"outline_levels = 8"), (dict(lines=-1), b"outline_levels"),
                         (dict(ldp=224), b"stride ldp"), (dict(ldp=250), b"multiple of 16"), (dict(GX=1 << 20, L=8, c=64, ldo=640, ldp=122880), b"too large"),
                         (dict(out=A + 8), b"alignment"), (dict(thumbs=A + 4), b"alignment"), (dict(colours=A + 2), b"alignment"),
                         (dict(rng=A + 4), b"alignment")):
        assert rg(**{**ok, **change}) == -1 and word in lib.paths_last_error(), (change, lib.paths_last_error())


def test_render_ref_is_the_reference_recipe_on_importance_map():
    """Fill the zeros of importance_map with its smallest positive value, autoscale, viridis, alpha where the map is positive
    (reference heatmap_visualise.py:170-181): the same picture, cell by cell, as render_ref on the folded importance map."""
    from paths_amd import colormaps, heatmap as hm
    rng = np.random.default_rng(8)
    table = colormaps.viridis()
    n_cases = holes = outlined = 0
    for L, grid, kw in ((3, (3, 5), {}), (1, (4, 1), {}), (2, (2, 2), {}), (3, (2, 2), dict(empty_below=2))):
        levels = random_hierarchy(rng, L, grid, **kw)
        m = hm.importance_map([{"locs": lv["locs"], "importance": lv["values"]} for lv in levels], grid)
        assert (m > 0).any() and m.min() >= 0
        holes += bool((m == 0).any())
        filled = np.where(m == 0, m[m > 0].min(), m)
        t = (filled - filled.min()) / (filled.max() - filled.min())
        colour = table[np.clip((t * 256.0).astype(np.int64), 0, 255)].astype(np.int64)
        want = np.where((m > 0)[..., None], (128 * colour + 127 * 255 + 127) // 255, 255).astype(np.uint8)
        got, (lo, hi), bad = RR.render(levels, grid, offset=1e-4, dtype=np.float64, cell_px=1, table=table, outline=())
        assert not bad and lo == m[m > 0].min() and hi == m.max()
        assert got.shape == m.shape + (3,) and np.array_equal(got, want), (L, grid)
        # a larger cell repeats it, and an outline touches the cell borders only
        big, _, _ = RR.render(levels, grid, offset=1e-4, dtype=np.float64, cell_px=4, table=table)
        inner = big.reshape(m.shape[0], 4, m.shape[1], 4, 3)[:, 1:3, :, 1:3]
        assert np.array_equal(inner, np.broadcast_to(want[:, None, :, None], inner.shape))
        corner = big.reshape(m.shape[0], 4, m.shape[1], 4, 3)[:, 0, :, 0]
        finest = RR.visited_masks(levels, grid)[L - 1]
        assert not corner[finest].any() and np.array_equal(corner[m == 0], want[m == 0])
        outlined += bool(finest.any())
        n_cases += 1
    assert n_cases == 4 and holes >= 3 and outlined >= 3


def test_render_ref_range_index_and_fallback_cell():
    assert RR.colour_index(np.array([0.0, 0.5, 1.0, 2.0, -1.0, 255.0 / 256, np.nextafter(1.0, 0)]), 0.0, 1.0).tolist() == [0, 128, 255, 255, 0, 255, 255]
    assert RR.colour_index(np.array([3.0, 4.0]), 3.0, 3.0).tolist() == [0, 0]
    v = np.array([[-0.0, 2.0], [np.nan, -3.0]])
    assert RR.value_range(v, np.ones((2, 2), bool)) == (-3.0, 2.0)
    lo, hi = RR.value_range(v, np.array([[True, False], [False, False]]))
    assert (lo, hi) == (0.0, 0.0) and np.signbit(lo) == np.signbit(hi) == False       # noqa: E712
    assert RR.value_range(v, np.ones((2, 2), bool), center=0.5) == (-3.0, 4.0)
    assert RR.value_range(v, np.zeros((2, 2), bool)) == (0.0, 0.0)
    # a level-1 patch outside any level-0 patch (the zero-children fallback's shape) is part of the folded picture
    levels = [{"locs": np.array([[0, 0]]) * PATCH, "values": np.array([1.0])},
              {"locs": np.array([[0, 0], [3, 2]]) * PATCH, "values": np.array([2.0, 5.0])}]
    image, (lo, hi), bad = RR.render(levels, (2, 2), dtype=np.float64, cell_px=1, table=RR.bwr(), alpha=1.0, outline=())
    assert (lo, hi) == (1.0, 2.5) and image[3, 2].tolist() == [255, 0, 0] and image[3, 3].tolist() == [255, 255, 255]
    plane0, _, _ = RR.render(levels, (2, 2), level=0, dtype=np.float64, cell_px=1, table=RR.bwr(), alpha=1.0, outline=())
    assert plane0[3, 2].tolist() == [255, 255, 255] and plane0[0, 0].tolist() == [0, 0, 255]
