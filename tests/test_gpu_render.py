"""GPU tests of the overlays (csrc/raster.hip: paths_render_range / paths_render_rgb; paths_amd.heatmap.render) against their NumPy
restatement (tests/render_ref.py), bit for bit.  The shapes are tests/test_gpu_raster.py's: grids (3, 5), (2, 2), (4, 1), at most 40
patches per level, one slide empty from level 2 on; rows of padding hold the hostile patterns, and every torch.empty of a call is
0xFF- / NaN-filled (tests/poison.py), so a byte the kernels do not write would show."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import poison as P
from tests import render_ref as RR
from tests.test_cpu_raster import PATCH
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)
from tests.test_gpu_raster import GRIDS, N_PAD, NP_OF, as_trace, hierarchies, level_tensors

pytestmark = pytest.mark.gpu

KIND = "grad_x_input"                                     # a signed kind: offset 0, no fold by default
TABLES = {"viridis": None, "bwr": RR.bwr()}


def viridis():
    if TABLES["viridis"] is None:
        from paths_amd import colormaps
        TABLES["viridis"] = colormaps.viridis()           # (its bytes are checked in tests/test_cpu_render.py)
    return TABLES["viridis"]


def thumbnails(dev, L, c, pad=0, seed=11):
    """One random uint8 image per grid of GRIDS; ``pad``: extra bytes behind every row (a row stride larger than the row)."""
    rng = np.random.default_rng(seed)
    f = 1 << (L - 1)
    host = [rng.integers(0, 256, (g[0] * f * c, g[1] * f * c, 3), dtype=np.uint8) for g in GRIDS]
    out = []
    for h in host:
        wide = torch.full((h.shape[0], h.shape[1] * 3 + pad), 0xA5, dtype=torch.uint8, device=dev)
        wide[:, :h.shape[1] * 3] = torch.from_numpy(h.reshape(h.shape[0], -1)).to(dev)
        out.append(wide[:, :h.shape[1] * 3].unflatten(-1, (h.shape[1], 3)))
        assert out[-1].stride() == (h.shape[1] * 3 + pad, 3, 1)
    return host, out


def base_of(images):
    base = images[0]
    while base._base is not None:
        base = base._base
    return base


def render_and_check(dev, hiers, vdtype=torch.float32, hostile=True, thumbs=None, label=None, ref_kw=None, **kw):
    """heatmap.render on the trace of ``hiers`` under poisoned allocations == render_ref per slide; bytes outside the slides' extents
    are 0.  ``thumbs``: (host images, device tensors).  Returns the images' bytes (the padded allocation, on the host)."""
    from paths_amd import heatmap as hm
    L = len(hiers[0])
    c = kw.get("cell_px", 4)
    f = 1 << (L - 1)
    trace = as_trace(level_tensors(dev, hiers, vdtype, hostile=hostile), KIND)
    with P.poisoned_empty("H"):
        images = hm.render(trace, GRIDS, KIND, thumbnails=None if thumbs is None else thumbs[1], **kw)
    torch.cuda.synchronize()
    base = base_of(images)
    assert base.dtype == torch.uint8 and base.dim() == 3 and base.shape[0] == len(GRIDS) and base.shape[2] % 16 == 0 and base.data_ptr() % 16 == 0
    whole = base.cpu().numpy().copy()
    ref = dict(cell_px=c, table=viridis(), dtype=NP_OF[kw.get("dtype", torch.float32)], level=kw.get("level"), fold=kw.get("fold") or 0.5)
    if isinstance(kw.get("cmap"), str):
        ref["table"] = TABLES[kw["cmap"]] if kw["cmap"] == "bwr" else viridis()
    elif "cmap" in kw:
        ref["table"] = np.asarray(kw["cmap"])
    for name in ("alpha", "center", "outline_rgb", "background", "offset"):
        if name in kw:
            ref[name] = kw[name]
    if "outline" in kw:
        ref["outline"] = None if kw["outline"] is True else (() if kw["outline"] is False else kw["outline"])
    ref.update(ref_kw or {})
    for b, g in enumerate(GRIDS):
        levels = [{"locs": lv["locs"], "values": lv["values"].astype(NP_OF[vdtype])} for lv in hiers[b]]
        per = dict(ref)
        for name in ("vmin", "vmax"):
            if kw.get(name) is not None:
                per[name] = np.broadcast_to(np.asarray(kw[name], np.float64), (len(GRIDS),))[b]
        want, _, _ = RR.render(levels, g, thumbnail=None if thumbs is None else thumbs[0][b], **per)
        got = images[b].cpu().numpy()
        assert got.shape == want.shape == (g[0] * f * c, g[1] * f * c, 3) and got.dtype == np.uint8
        if not np.array_equal(got, want):
            at = np.argwhere((got != want).any(axis=-1))
            raise AssertionError("%r, slide %d: %d pixels differ, the first at %s: got %s, want %s" % (
                label, b, len(at), at[:6].tolist(), got[tuple(at[:6].T)].tolist(), want[tuple(at[:6].T)].tolist()))
        whole[b, :g[0] * f * c, :g[1] * f * c * 3] = 0
    assert not whole.any(), (label, "bytes outside the slides' extents are not 0")
    return base.cpu().numpy()


@pytest.mark.parametrize("cell_px", [1, 3, 4, 5])
@pytest.mark.parametrize("L", [1, 3])
def test_render_vs_render_ref(dev, L, cell_px):
    """Folded and every single level, fp32 and fp64 values and rasters, automatic range, all outlines.  Odd cell_px: rows that are no
    multiple of 16 bytes and a ragged last run; s_l = cell_px << (L-1-l) is below 4 for some levels (no outline) and not for others."""
    hiers = hierarchies(L)
    spans = [cell_px << (L - 1 - l) for l in range(L)]
    assert L == 1 or cell_px > 3 or (min(spans) < 4 <= max(spans))
    for vdtype, dtype in ((torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float32, torch.float64)):
        for level in [None] + list(range(L)):
            render_and_check(dev, hiers, vdtype, cell_px=cell_px, level=level, dtype=dtype, label=(L, cell_px, vdtype, dtype, level))
    render_and_check(dev, hiers, cell_px=cell_px, fold=0.3, offset=0.25, label=(L, cell_px, "fold 0.3"))


@pytest.mark.parametrize("cell_px", [3, 4])
def test_thumbnails_and_alpha(dev, cell_px):
    hiers = hierarchies(3)
    for pad in (0, 7, 16):                                 # contiguous rows; rows that start unaligned; aligned rows with a gap
        thumbs = thumbnails(dev, 3, cell_px, pad)
        for alpha in (0.0, 0.5, 1.0):
            render_and_check(dev, hiers, thumbs=thumbs, cell_px=cell_px, alpha=alpha, label=(cell_px, pad, alpha))
    render_and_check(dev, hiers, thumbs=thumbnails(dev, 3, cell_px, 3), cell_px=cell_px, level=1, outline=False, label=(cell_px, "level 1"))
    for alpha in (0.0, 1.0, 0.25):
        render_and_check(dev, hiers, cell_px=cell_px, alpha=alpha, background=(10, 200, 30), outline_rgb=(255, 0, 7), label=(cell_px, alpha))
    # alpha 0 without outlines is the thumbnail itself; alpha 1 hides it wherever a cell is visited
    from paths_amd import heatmap as hm
    host, device = thumbnails(dev, 3, cell_px)
    trace = as_trace(level_tensors(dev, hiers, torch.float32), KIND)
    for b, im in enumerate(hm.render(trace, GRIDS, KIND, thumbnails=device, cell_px=cell_px, alpha=0.0, outline=False)):
        assert np.array_equal(im.cpu().numpy(), host[b])


def test_ranges_given_per_slide_and_constant(dev):
    from paths_amd import heatmap as hm
    hiers = hierarchies(3)
    render_and_check(dev, hiers, vmin=-0.5, vmax=0.75, label="scalar range")
    render_and_check(dev, hiers, vmin=[-1.0, 0.0, 0.25], vmax=[1.0, 2.0, 0.25], label="per-slide range")       # (slide 2: vmax == vmin)
    render_and_check(dev, hiers, vmin=0.0, label="vmin alone")
    render_and_check(dev, hiers, vmax=torch.tensor([0.1, 0.2, 0.3]), level=2, label="vmax alone")
    render_and_check(dev, hiers, vmin=-0.5, vmax=0.75, check=False, dtype=torch.float64, label="no range kernel")
    trace = as_trace(level_tensors(dev, hiers, torch.float32), KIND)
    for kw, want in ((dict(vmin=0.0, vmax=1.0, check=False), ["paths_render_rgb"]), (dict(vmin=0.0, vmax=1.0), ["paths_render_range", "paths_render_rgb"]),
                     (dict(vmin=0.0, check=False), ["paths_render_range", "paths_render_rgb"]), (dict(), ["paths_render_range", "paths_render_rgb"])):
        with H.spy_calls() as calls:
            hm.render(trace, GRIDS, KIND, **kw)
        assert calls == ["paths_raster_index"] * 3 + ["paths_raster_maps"] + want, (kw, calls)
    with H.spy_calls() as calls:                           # rasterize launches what it launched before
        hm.rasterize(trace, GRIDS, KIND)
    assert calls == ["paths_raster_index"] * 3 + ["paths_raster_maps"]
    # a constant map: vmax == vmin, every visited pixel takes colour 0
    flat = hierarchies(3)
    for h in flat:
        for lv in h:
            lv["values"] = np.full(len(lv["values"]), 0.375)
    render_and_check(dev, flat, level=0, label="constant plane")
    images = hm.render(as_trace(level_tensors(dev, flat, torch.float32), KIND), GRIDS, KIND, level=0, alpha=1.0, outline=False)
    seen = np.unique(images[0].cpu().numpy().reshape(-1, 3), axis=0).tolist()
    assert sorted(seen) == sorted([[255, 255, 255], viridis()[0].tolist()])


def test_signed_kind_centered_under_bwr(dev):
    hiers = hierarchies(3)
    assert any((lv["values"] < 0).any() and (lv["values"] > 0).any() for lv in hiers[0])
    for level in (None, 0, 2):
        for dtype in (torch.float32, torch.float64):
            render_and_check(dev, hiers, cmap="bwr", center=0.0, level=level, dtype=dtype, alpha=1.0, label=("bwr", level, dtype))
    render_and_check(dev, hiers, cmap="bwr", center=0.125, cell_px=5, label="center 0.125")
    own = np.random.default_rng(2).integers(0, 256, (256, 3), dtype=np.uint8)
    render_and_check(dev, hiers, cmap=own, label="a table of the caller's")
    render_and_check(dev, hiers, cmap=torch.from_numpy(own), ref_kw=dict(table=own), label="as a tensor")


@pytest.mark.parametrize("cell_px", [1, 4])
def test_outline_subsets(dev, cell_px):
    hiers = hierarchies(3)
    for outline in (True, False, [1], [0, 2], (2,)):
        for level in (None, 1):
            render_and_check(dev, hiers, cell_px=cell_px, outline=outline, level=level, label=(cell_px, outline, level))
    if cell_px == 4:                                       # the three levels' rectangles are there, and they differ
        sums = [int(render_and_check(dev, hiers, outline=o, alpha=0.0).astype(np.int64).sum()) for o in (False, [0], [1], [2], True)]
        assert len(set(sums)) == 5 and sums[0] == max(sums)


def test_a_deeper_cell_without_a_level0_parent_is_drawn_in_the_folded_map(dev):
    """The zero-children fallback's shape: slide 0 gets a level-1 patch (and its level-2 child) under a level-0 cell nobody visited."""
    from paths_amd import heatmap as hm
    hiers = hierarchies(3)
    cells0 = {tuple(c) for c in (hiers[0][0]["locs"] // PATCH).tolist()}
    hole = next((x, y) for x in range(GRIDS[0][0]) for y in range(GRIDS[0][1]) if (x, y) not in cells0)
    for l in (1, 2):
        cell = np.array([[(hole[0] << l) + (1 << l) - 1, (hole[1] << l) + (1 << l) - 1]], np.int64)      # (the level-2 one under the level-1 one)
        assert not (hiers[0][l]["locs"] // PATCH == cell).all(axis=1).any()
        keep = slice(1, None) if len(hiers[0][l]["locs"]) == N_PAD else slice(None)                     # (at most N_PAD rows per level)
        hiers[0][l] = {"locs": np.concatenate([hiers[0][l]["locs"][keep], cell * PATCH]),
                       "values": np.concatenate([hiers[0][l]["values"][keep], [0.5 * l]])}
    for level in (None, 0, 1):
        render_and_check(dev, hiers, level=level, label=("fallback", level))
    trace = as_trace(level_tensors(dev, hiers, torch.float32), KIND)
    x, y = (((hole[0] << 2) + 3) * 4 + 1, ((hole[1] << 2) + 3) * 4 + 1)      # inside the level-2 child, off its outline
    folded = hm.render(trace, GRIDS, KIND)[0][x, y].tolist()
    plane0 = hm.render(trace, GRIDS, KIND, level=0)[0][x, y].tolist()
    assert plane0 == [255, 255, 255] and folded != [255, 255, 255]


@pytest.mark.parametrize("vdtype", [torch.float32, torch.float64])
def test_nothing_depends_on_the_padding_and_a_repeat_is_bit_identical(dev, vdtype):
    hiers = hierarchies(3)
    for kw in (dict(), dict(level=2, cell_px=3), dict(center=0.0, cmap="bwr", dtype=torch.float64)):
        clean = render_and_check(dev, hiers, vdtype, hostile=False, **kw)
        dirty = render_and_check(dev, hiers, vdtype, hostile=True, **kw)
        again = render_and_check(dev, hiers, vdtype, hostile=True, **kw)
        assert clean.tobytes() == dirty.tobytes() == again.tobytes(), kw


def test_a_non_finite_value_raises_or_is_drawn_as_not_visited(dev):
    from paths_amd import _lib, heatmap as hm
    hiers = hierarchies(3)
    hiers[0][1]["values"][2] = np.nan
    hiers[2][0]["values"][0] = np.inf
    trace = as_trace(level_tensors(dev, hiers, torch.float32, hostile=True), KIND)
    with pytest.raises(_lib.PathsHipError, match=r"slide\(s\) 0, 2 hold a non-finite grad_x_input"):
        hm.render(trace, GRIDS, KIND)
    with pytest.raises(_lib.PathsHipError, match=r"slide\(s\) 0 hold a non-finite"):
        hm.render(trace, GRIDS, KIND, level=1, vmin=0.0, vmax=1.0)
    hm.render(trace, GRIDS, KIND, level=2)                          # plane 2 holds neither
    for level in (None, 0, 1):
        render_and_check(dev, hiers, level=level, check=False, label=("non-finite", level))
    ok = hierarchies(3)
    for b, g in enumerate(GRIDS):                                    # the reference agrees that those cells are bad, and only those
        levels = [{"locs": lv["locs"], "values": lv["values"].astype(np.float32)} for lv in hiers[b]]
        assert RR.render(levels, g, cell_px=1, table=viridis())[2] == (b != 1)
        assert not RR.render([{"locs": lv["locs"], "values": lv["values"].astype(np.float32)} for lv in ok[b]], g, cell_px=1, table=viridis())[2]
    # a location outside the grid is still rasterize's report
    far = hierarchies(3)
    far[1][1]["locs"] = np.concatenate([far[1][1]["locs"], np.array([[1000 * PATCH, 0]], np.int64)])
    far[1][1]["values"] = np.concatenate([far[1][1]["values"], [1.0]])
    with pytest.raises(_lib.PathsHipError, match=r"level\(s\) 1 hold a location outside"):
        hm.render(as_trace(level_tensors(dev, far, torch.float32), KIND), GRIDS, KIND)


def test_default_render_of_a_recursion_is_the_reference_picture_of_importance_map(dev, tmp_path):
    """recurse(..., trace=[]) of a small model, rendered with default arguments == render_ref.compose on heatmap.importance_map of the
    host records; saved by save_png it reads back."""
    from paths_amd import heatmap as hm, utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    from tests.test_cpu_render import decode_png
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[20] * 4)
    slides = [DeviceSlide.synthetic(14, sid, base, p_bg=0.1, device=dev) for sid, base in enumerate([(6, 7), (5, 4)])]
    grids = [s.shape(0) for s in slides]
    trace = []
    with torch.no_grad():
        putils.recurse(model, slides, cfg.top_k_patches, 5, trace=trace)
    with P.poisoned_empty("H"):
        images = hm.render(trace, slides)
    for b, g in enumerate(grids):
        host = hm.hierarchy_from_trace(trace, b)
        value = hm.importance_map(host, g).astype(np.float32)
        visited = RR.visited_masks([{"locs": lv["locs"]} for lv in host], g)
        assert np.array_equal(visited.any(axis=0), value != 0) and visited[4].any()
        want, _, bad = RR.compose(value, visited, range(5), 4, viridis(), outline=range(5))
        got = images[b].cpu().numpy()
        assert not bad and got.shape == (g[0] * 64, g[1] * 64, 3) and np.array_equal(got, want), b
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 8
    hm.save_png(tmp_path / "slide0.png", images[0])
    back, _ = decode_png((tmp_path / "slide0.png").read_bytes())
    assert np.array_equal(back, images[0].cpu().numpy())
