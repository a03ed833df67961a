"""Every route to a stored slide (paths_amd/data_utils/slide.py: _Slide._build) gives the same slide: synthetic, from_host and
from_patches, dense and packed, pack / to_dense / to_device, on DeviceSlide and HostSlide, fp32 and fp16.  Tiny grids (base 2 x 3, three
levels, D = 8, half of the deeper cells background); the reference is the host generator's grid (synthetic.SyntheticSlide.grid)."""
import pytest
import torch

from tests.test_gpu_packed_slides import F16, F32, bits, free_pinned
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, LEVELS, BASE = 8, 3, (2, 3)


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def stored_bits(s, l):
    """The bits of level ``l``'s dense grid as the slide stores it (a packed level through unpack_grid), on the host."""
    from paths_amd.data_utils.slide import unpack_grid
    g = unpack_grid(s.rows[l].cpu(), s.index[l].cpu()) if s.packed else s.grids[l].cpu()
    return bits(g)


def assert_same_slide(s, want_grids, want_masks, absmax, what):
    assert s.num_levels == len(want_grids) and s.dim == D, what
    for l, (g, m) in enumerate(zip(want_grids, want_masks)):
        assert s.shape(l) == tuple(g.shape[:2]), (what, l)
        assert torch.equal(s.masks[l].cpu(), m), (what, l)
        assert torch.equal(stored_bits(s, l), bits(g)), (what, l)
    assert s.feature_absmax() == absmax, what
    if s.host_resident:
        assert s.host_bytes() == nbytes(s.rows if s.packed else s.grids), what
        assert s.resident_bytes() == nbytes(s.masks) + (nbytes(s.index) if s.packed else 0), what
        assert all(t.is_pinned() for t in (s.rows if s.packed else s.grids) if t.numel()), what
    else:
        assert s.resident_bytes() == nbytes(s.masks) + (nbytes(s.rows) + nbytes(s.index) if s.packed else nbytes(s.grids)), what
    assert (s.grids is None and s.rows is not None and s.index is not None) if s.packed else (s.rows is None and s.index is None), what


def patch_lists(grids):
    """Exactly the tissue cells of ``grids`` in row-major order, as from_patches takes them."""
    coords, feats = [], []
    for g in grids:
        c = torch.nonzero((g != 0).any(dim=-1)).to(torch.int64).reshape(-1, 2)
        coords.append(c)
        feats.append(g[c[:, 0], c[:, 1]].reshape(-1, D))
    return coords, feats, [tuple(g.shape[:2]) for g in grids]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", ["device", "host"])
def test_every_route_gives_the_same_slide(dev, kind, dtype):
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide
    cls = DeviceSlide if kind == "device" else HostSlide
    kw = dict(dim=D, num_levels=LEVELS, p_bg=0.5, device=dev, dtype=dtype)
    # HostSlide: a bounce buffer of ONE row - the smallest the chunk plan accepts, every row is its own chunk
    one_row = dict(bounce_bytes=D * (2 if dtype == F16 else 4)) if kind == "host" else {}
    base = cls.synthetic(31, 2, BASE, **kw)
    spec = base.synthetic_spec
    host = [torch.from_numpy(spec.grid(l)) for l in range(LEVELS)]               # (fp32 arrays; fp16: of fp16-representable values)
    want = [g.to(dtype) for g in host]
    masks = [(g != 0).any(dim=-1).to(torch.uint8) for g in host]                # synthetic tissue rows never sum to zero
    absmax = max(float(g.abs().max()) for g in host)
    assert [tuple(g.shape) for g in host] == [(2, 3, D), (4, 6, D), (8, 12, D)] and all(0 < int(m.sum()) for m in masks)
    assert int(masks[2].sum()) < 96, "the largest level has background"
    packed = base.pack()
    routes = {"synthetic": base, "synthetic packed": cls.synthetic(31, 2, BASE, packed=True, **kw, **one_row),
              "from_host": cls.from_host(host, dev, dtype=dtype, **one_row), "from_host packed": cls.from_host(host, dev, dtype=dtype, packed=True),
              "from_patches": cls.from_patches(*patch_lists(host), dev, dtype=dtype), "pack": packed, "pack to_dense": packed.to_dense()}
    if kind == "host":
        routes.update({"to_device": base.to_device(), "pack to_device": packed.to_device()})
    for what, s in routes.items():
        assert_same_slide(s, want, masks, absmax, what)
        assert s.dtype == dtype and s.packed == ("pack" in what and "dense" not in what or what == "from_patches"), what
        assert s.host_resident == (kind == "host" and "to_device" not in what) and not s.masked_view, what
        assert s.synthetic_spec == (None if what.startswith("from_") else spec), what
    assert packed.pack() is packed and base.to_dense() is base
    # a level without tissue (n = 0) from patch lists, against the dense slide of the same grids
    holed = [host[0], torch.zeros_like(host[1]), host[2]]
    coords, feats, shapes = patch_lists(holed)
    assert coords[1].shape == (0, 2) and feats[1].shape == (0, D)
    s = cls.from_patches(coords, feats, shapes, dev, dtype=dtype, **one_row)
    hmasks = [masks[0], torch.zeros_like(masks[1]), masks[2]]
    habs = max(float(holed[0].abs().max()), float(holed[2].abs().max()))
    assert s.rows[1].shape == (0, D) and int((s.index[1] >= 0).sum()) == 0
    for what, t in (("from_patches n=0", s), ("from_patches n=0 to_dense", s.to_dense()), ("from_host holed", cls.from_host(holed, dev, dtype=dtype))):
        assert_same_slide(t, [g.to(dtype) for g in holed], hmasks, habs, what)
    del routes, base, packed, s, t
    free_pinned()
