"""GPU tests of the annotation kernels (csrc/polygons.hip: paths_polygon_cover / paths_polygon_outline; paths_amd/annotations.py) against
their NumPy contract (tests/polygon_ref.py): coverage bit for bit, outlines byte for byte including every byte they must not touch,
and one pass from a recursion's trace to per-patch coverage and localisation scores.  Grids are a few cells, so that every extent is
ragged against the kernel's 16 x 16 tile; the long polygon overruns its 256-edge LDS tile a dozen times."""
import numpy as np
import pytest
import torch

from tests import polygon_ref as PR
from tests.test_cpu_annotations import localisation_loop, patch_cover_loop
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

L = 3
CELL = 256 >> (L - 1)                                      # level-0 pixels per finest cell
GRIDS = [(3, 5), (2, 2), (1, 1)]                           # finest rasters 12 x 20, 8 x 8, 4 x 4


def star(cr, cc, radius, points=5):
    a = 2 * np.pi * np.arange(points) * 2 / points + 0.3
    return np.stack([cr + radius * np.cos(a), cc + radius * np.sin(a)], axis=1)


def ragged_polygons():
    """Per slide, in level-0 pixels (one finest cell = 64): slide 0 carries every kind, slide 1 none, slide 2 two."""
    slide0 = [
        np.array([[20.5, 700.25], [300.0, 1250.75], [180.0, 800.0]]),                                         # a triangle
        np.array([[400.0, 700.0], [400.0, 1200.0], [700.0, 1200.0], [700.0, 700.0], [550.0, 950.0]]),         # concave
        star(380.0, 330.0, 290.0),                                                                            # self-intersecting: a parity hole
        np.array([[10.0, 10.0], [10.0, 200.0], [200.0, 200.0], [200.0, 10.0]]),                               # two that overlap ...
        np.array([[100.0, 100.0], [100.0, 300.0], [300.0, 300.0], [300.0, 100.0]]),                           # ... a union
        # vertices and horizontal edges exactly on sample coordinates: rows 64 + 8 (s = 4), 128 + 6 (s = 16), 192 + 32 (s = 1), columns
        # 64 + 32 (s = 1), 576 + 24 (s = 4), 384 + 6 (s = 16)
        np.array([[72.0, 96.0], [72.0, 600.0], [134.0, 600.0], [134.0, 390.0], [224.0, 390.0], [224.0, 96.0]]),
        np.array([[600.0, 1000.0], [900.0, 1400.0], [500.0, 1350.0]]),                                        # partly outside the grid
        np.array([[-40.0, 420.0], [90.0, 500.0], [-10.0, 640.0]]),
        np.array([[2000.0, 3000.0], [2000.0, 3400.0], [2500.0, 3100.0]]),                                     # entirely outside: beyond,
        np.array([[100.0, -900.0], [600.0, -100.0], [300.0, -50.0]]),                                         # on the near side,
        np.array([[100.0, 1400.0], [700.0, 1500.0], [300.0, 2500.0]]),                                        # on the far side
    ]
    slide2 = [np.array([[20.0, 30.0], [240.0, 100.0], [100.0, 250.0]]), np.array([[-50.0, 128.0], [128.0, 300.0], [300.0, 128.0], [128.0, -50.0]])]
    return [slide0, [], slide2]


def long_polygons():
    """About 3,000 jittered vertices around a circle on a 16 x 16-cell grid, and the same polygon over a 20 x 12 one next to it."""
    rng = np.random.default_rng(7)
    n = 3001
    a = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = 380.0 + rng.uniform(-25, 25, n)
    ring = np.stack([512.0 + r * np.cos(a), 512.0 + r * np.sin(a)], axis=1)
    return [[ring], [ring * 0.9 + 40.0, np.array([[600.0, 100.0], [1200.0, 300.0], [900.0, 700.0]])]], [(4, 4), (5, 3)]


_cache = {}


def case(name):
    """(Polygons, reference polygons per slide): built once per case."""
    from paths_amd import annotations as A
    if name not in _cache:
        per_slide, grids = (ragged_polygons(), GRIDS) if name == "ragged" else long_polygons()
        p = A.Polygons(per_slide, grids, L)
        fixed = [[PR.fixed(poly, 1 << (L - 1), 256) for poly in polys] for polys in per_slide]
        for b in range(p.B):                                                   # the host conversion is the contract's
            assert [q.tolist() for q in p.slide_polygons(b)] == [q.tolist() for q in fixed[b]]
        _cache[name] = (p, fixed, {})
    return _cache[name]


def reference_cover(name, s):
    p, fixed, refs = case(name)
    if s not in refs:
        refs[s] = [PR.coverage(fixed[b], *p.finest(b), s) for b in range(p.B)]
    return refs[s]


def base_of(views):
    base = views[0]
    while base._base is not None:
        base = base._base
    return base


@pytest.mark.parametrize("s", [1, 4, 16])
@pytest.mark.parametrize("name", ["ragged", "long"])
def test_coverage_equals_the_contract_bit_for_bit(dev, name, s):
    from paths_amd import annotations as A
    p, _, _ = case(name)
    want = reference_cover(name, s)
    with torch.cuda.device(dev):
        got = A.coverage(p, s)
        base = base_of(got)
        X, Y = max(g[0] for g in p.grids) << (L - 1), max(g[1] for g in p.grids) << (L - 1)
        assert base.dtype == torch.int32 and tuple(base.shape) == (p.B, X, (Y + 3) // 4 * 4)
        whole = base.cpu().numpy().copy()
        for b in range(p.B):
            g = got[b].cpu().numpy()
            assert g.shape == want[b].shape == p.finest(b) and g.dtype == np.int32
            if not np.array_equal(g, want[b]):
                at = np.argwhere(g != want[b])
                raise AssertionError("%s, s = %d, slide %d: %d cells differ, the first at %s: got %s, want %s" % (
                    name, s, b, len(at), at[:6].tolist(), g[tuple(at[:6].T)].tolist(), want[b][tuple(at[:6].T)].tolist()))
            whole[b, :g.shape[0], :g.shape[1]] = 0
        assert not whole.any(), "cells outside the slides' extents are not 0"
        # a second launch, into an allocation that held something else, gives identical bytes
        out = torch.full_like(base, -7)
        again = A.coverage(p, s, out=out)
        assert base_of(again) is out and out.cpu().numpy().tobytes() == base.cpu().numpy().tobytes()
    if name == "ragged":                                                       # the cases are what they claim to be
        assert not want[1].any() and want[2].any() and 0 < want[0].sum() < want[0].size * s * s
        if s == 4:
            assert want[0].max() == 16 and want[0][5:7, 4:6].sum() == 0          # (the star's centre: outside by parity)
            assert (want[0][0:3, 0:3] == 16).sum() >= 4                          # the union holds whole cells, counted once


def random_images(dev, p, c, pad, seed):
    """One allocation [B, rows, ld] of pseudo-random bytes and per slide the view render would return; rows ``pad`` bytes longer than
    the widest image."""
    f = 1 << (L - 1)
    H, W = max(g[0] for g in p.grids) * f * c, max(g[1] for g in p.grids) * f * c
    ld = (W * 3 + pad + 15) // 16 * 16
    host = np.random.default_rng(seed).integers(0, 256, (p.B, H, ld), dtype=np.uint8)
    base = torch.from_numpy(host).to(dev)
    views = [base[b, :g[0] * f * c, :g[1] * f * c * 3].unflatten(-1, (g[1] * f * c, 3)) for b, g in enumerate(p.grids)]
    return host, base, views


OUTLINE_GRIDS = [(3, 5), (2, 2)]


def outline_polygons():
    slide0 = ragged_polygons()[0][:3] + [
        np.array([[-300.0, -200.0], [500.0, 1500.0], [900.0, 600.0]]),                                        # edges that leave the image
        np.array([[64.0, 64.0], [64.0, 640.0], [640.0, 640.0], [640.0, 64.0]]),                               # horizontal and vertical
        np.array([[0.0, 0.0], [767.9, 1279.9], [767.9, 0.0]]),                                                # corner to corner, along the border
        np.array([[333.0, 333.0], [333.0, 333.0], [333.2, 333.1]]),                                           # zero-length edges
    ]
    slide1 = [np.array([[20.0, 30.0], [500.0, 100.0], [100.0, 505.0]]), np.array([[-50.0, 256.0], [256.0, 600.0], [600.0, 256.0], [256.0, -50.0]])]
    return [slide0, slide1]


@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("cell_px", [1, 4])
def test_outlines_equal_the_contract_byte_for_byte(dev, cell_px, width):
    from paths_amd import annotations as A
    p = A.Polygons(outline_polygons(), OUTLINE_GRIDS, L)
    rgb = (0, 0, 255) if width == 1 else (250, 3, 77)
    host, base, views = random_images(dev, p, cell_px, 7, 100 * cell_px + width)
    assert views[0].stride(0) > 3 * views[0].shape[1] and views[1].shape[0] < base.shape[1]
    want = host.copy()
    for b, g in enumerate(p.grids):
        h, w = p.finest(b)[0] * cell_px, p.finest(b)[1] * cell_px
        image = np.ascontiguousarray(want[b, :h, :3 * w].reshape(h, w, 3))
        PR.draw(image, p.slide_polygons(b), cell_px, rgb, width)
        want[b, :h, :3 * w] = image.reshape(h, 3 * w)
    back = A.draw(views, p, cell_px, rgb=rgb, width=width)
    assert all(x is y for x, y in zip(back, views))
    got = base.cpu().numpy()
    assert (want != host).any() and got.tobytes() == want.tobytes(), "%d bytes differ" % int((got != want).sum())
    A.draw(views, p, cell_px, rgb=rgb, width=width)                            # drawing again changes nothing
    assert base.cpu().numpy().tobytes() == want.tobytes()


def test_outlines_on_rendered_overlays_and_a_batch_without_polygons(dev):
    from paths_amd import annotations as A
    empty = A.Polygons([[], []], OUTLINE_GRIDS, L)
    host, base, views = random_images(dev, empty, 2, 0, 5)
    A.draw(views, empty, 2)
    assert base.cpu().numpy().tobytes() == host.tobytes()
    with torch.cuda.device(dev):
        assert all(not c.any() for c in A.coverage(empty, 4))
    with pytest.raises(ValueError, match="image 1 must be"):
        A.draw([views[0], views[1][:, :-1]], empty, 2)


def test_recursion_to_patch_cover_and_localisation(dev):
    """recurse(..., trace=[]) on two synthetic slides; a rectangle around a known block of level-0 cells and a triangle; patch_cover and
    localisation on the device records == the NumPy loop on their host copies."""
    from paths_amd import annotations as A, heatmap as hm, utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[20] * 4)
    slides = [DeviceSlide.synthetic(14, sid, base, p_bg=0.1, device=dev) for sid, base in enumerate([(6, 7), (5, 4)])]
    trace = []
    with torch.no_grad():
        putils.recurse(model, slides, cfg.top_k_patches, 5, trace=trace)
    # cells x in [1, 3), y in [2, 5) of level 0, the rectangle a little inside them on one side and outside on the other
    block = np.array([[256.0 - 37.5, 512.0 + 20.25], [256.0 - 37.5, 1280.0 + 11.0], [768.0 - 3.0, 1280.0 + 11.0], [768.0 - 3.0, 512.0 + 20.25]])
    p = A.Polygons([[block, np.array([[900.0, 100.0], [1500.0, 300.0], [1000.0, 900.0]])], [block * 0.8]], slides, 5)
    assert p.grids == [(6, 7), (5, 4)] and p.f == 16
    s = 4
    cover = A.coverage(p, s)
    host_cover = [c.cpu().numpy() for c in cover]
    for b in range(2):
        assert np.array_equal(host_cover[b], PR.coverage(p.slide_polygons(b), *p.finest(b), s))
    assert (host_cover[0][16:47, 48:80] == s * s).all() and not host_cover[0][:13].any()
    host_trace = [{k: v.detach().cpu() for k, v in lv.items() if k in ("locs", "num_ims", "importance", "keep_idx", "keep_count")} for lv in trace]
    masks = [[m.cpu().numpy() for m in sl.masks] for sl in slides]
    got = A.patch_cover(trace, cover, s)
    want = patch_cover_loop(host_trace, host_cover, 5)
    for l in range(5):
        assert got[l].is_cuda and got[l].dtype == torch.int32 and np.array_equal(got[l].cpu().numpy(), want[l]), l
    assert 0 < want[0].max() <= (s * 16) ** 2
    res = A.localisation(trace, slides, cover, s)
    ref = localisation_loop(host_trace, host_cover, masks, 5, s, 0.5)
    for l in range(5):
        for b in range(2):
            for key, v in ref[l][b].items():
                g = res[l][b][key]
                assert g == v or (isinstance(v, float) and np.isnan(v) and np.isnan(g)), (l, b, key, g, v)
    assert res[0][0]["visited_pos"] > 0 and res[0][0]["tissue_pos"] > 0 and res[4][0]["kept_pos"] is None
    # the outlines go on the overlay render returns for the same trace
    images = hm.render(trace, slides, cell_px=1)
    before = [im.cpu().numpy().copy() for im in images]
    A.draw(images, p, 1, rgb=(0, 0, 255), width=3)
    for b in range(2):
        want_image = PR.draw(before[b].copy(), p.slide_polygons(b), 1, (0, 0, 255), 3)
        assert np.array_equal(images[b].cpu().numpy(), want_image) and (want_image != before[b]).any()
