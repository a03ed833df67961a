"""GPU tests of the device rasters (csrc/raster.hip: paths_raster_index / paths_raster_maps; paths_amd.heatmap.rasterize) against
their NumPy restatement (tests/raster_ref.py) and the NumPy painting functions of paths_amd.heatmap, bit for bit."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import poison as P
from tests import raster_ref as R
from tests.test_cpu_raster import PATCH, random_hierarchy, same_bits
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GRIDS = [(3, 5), (2, 2), (4, 1)]
N_PAD = 40
NP_OF = {torch.float32: np.float32, torch.float64: np.float64}
# what padded rows hold in the poisoned runs: huge, negative and NaN (int64 rows: huge and negative, and the NaN words read as integers)
HOSTILE_I64 = (1 << 62, -(1 << 62), -1, 0x7FC000007FC00000, -(1 << 40) - 7)
HOSTILE_F64 = (float("nan"), float("inf"), -float("inf"), 3.0e300, -3.0e300)


def hierarchies(L, seed=5, signed=True, empty=(1, 2)):
    """One hierarchy per grid of GRIDS with at most N_PAD patches per level; slide ``empty[0]`` has no patch from level ``empty[1]`` on."""
    rng = np.random.default_rng(seed)
    return [random_hierarchy(rng, L, g, signed=signed, cap=N_PAD, empty_below=empty[1] if b == empty[0] and L > empty[1] else None)
            for b, g in enumerate(GRIDS)]


def level_tensors(dev, hiers, vdtype, hostile=False, N=N_PAD):
    """Per level: locs [B, N, 2] int64, num_ims [B] int64, values [B, N]; rows of padding hold zeros, or the hostile patterns."""
    B, L = len(hiers), len(hiers[0])
    out = []
    for l in range(L):
        locs = np.zeros((B, N, 2), np.int64)
        vals = np.zeros((B, N), NP_OF[vdtype])
        if hostile:
            locs[:] = np.resize(np.array(HOSTILE_I64, np.int64), locs.shape)
            if vdtype == torch.float32:
                vals[:] = np.resize(np.array(P.HOSTILE_F32, np.uint32).view(np.float32), vals.shape)
            else:
                vals[:] = np.resize(np.array(HOSTILE_F64, np.float64), vals.shape)
        num_ims = np.zeros((B,), np.int64)
        for b in range(B):
            n = len(hiers[b][l]["locs"])
            assert n <= N
            locs[b, :n], vals[b, :n], num_ims[b] = hiers[b][l]["locs"], hiers[b][l]["values"].astype(NP_OF[vdtype]), n
        out.append((torch.from_numpy(locs).to(dev), torch.from_numpy(num_ims).to(dev), torch.from_numpy(vals).to(dev)))
    return out


def run_kernels(dev, levels, grids, odtype, fold, offset=0.0, w=0.5, extra_ld=4):
    """The two entry points alone, with strides of the caller's choosing: index rows exactly GY << l wide (odd widths included), output
    rows padded to four and then by ``extra_ld``.  Returns (out, status): out [B, X, ldo] (fold) or [B, L, X, ldo], NaN-filled before."""
    from paths_amd import _lib
    B, L = len(grids), len(levels)
    f = 1 << (L - 1)
    GX, GY = max(g[0] for g in grids), max(g[1] for g in grids)
    gx = torch.tensor([g[0] for g in grids], dtype=torch.int32, device=dev)
    gy = torch.tensor([g[1] for g in grids], dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    index = [torch.full((B, GX << l, GY << l), -1, dtype=torch.int32, device=dev) for l in range(L)]
    ldo = (GY * f + 3) // 4 * 4 + extra_ld
    out = torch.full((B, GX * f, ldo) if fold else (B, L, GX * f, ldo), float("nan"), dtype=odtype, device=dev)
    table = torch.tensor([[index[l].data_ptr(), GY << l, levels[l][2].data_ptr(), levels[l][2].stride(0)] for l in range(L)],
                         dtype=torch.int64, device=dev)
    offw = torch.tensor([offset, w], dtype=torch.float64, device=dev)
    s = _lib.stream()
    for l, (locs, num_ims, vals) in enumerate(levels):
        _lib.call("paths_raster_index", locs.data_ptr(), num_ims.data_ptr(), gx.data_ptr(), gy.data_ptr(), l, PATCH, locs.shape[1], B, GX, GY,
                  index[l].data_ptr(), GY << l, status.data_ptr(), s)
    _lib.call("paths_raster_maps", table.data_ptr(), gx.data_ptr(), gy.data_ptr(), L, B, GX, GY, int(levels[0][2].dtype == torch.float64),
              int(odtype == torch.float64), int(fold), offw.data_ptr(), out.data_ptr(), ldo, s)
    torch.cuda.synchronize()
    return out, int(status.item())


def check_against_ref(out, hiers, grids, vdtype, odtype, fold, offset, w, label):
    """Each slide's own extent equals raster_ref bit for bit; everything else of the padded allocation is +0."""
    L = len(hiers[0])
    f = 1 << (L - 1)
    got = out.cpu().numpy()
    for b, g in enumerate(grids):
        levels = [{"locs": lv["locs"], "values": lv["values"].astype(NP_OF[vdtype])} for lv in hiers[b]]
        want = R.raster(levels, g, offset=offset, fold=w if fold else None, dtype=NP_OF[odtype])
        mine = got[b][..., :g[0] * f, :g[1] * f]
        assert same_bits(mine, want), (label, b, int((mine != want).sum()))
        rest = got[b].copy()
        rest[..., :g[0] * f, :g[1] * f] = 0
        assert not rest.view(np.uint32 if odtype == torch.float32 else np.uint64).any(), (label, b, "cells outside the slide's extent are not +0")


@pytest.mark.parametrize("L", [3, 1, 2])
def test_kernels_vs_raster_ref(dev, L):
    """B = 3, base grids (3, 5), (2, 2), (4, 1), N padded to 40; fp32 / fp64 values and outputs, both forms; L = 1 is the odd Y = 5."""
    hiers = hierarchies(L)
    assert len({len(h[L - 1]["locs"]) for h in hiers}) > 1 and (L < 3 or len(hiers[1][2]["locs"]) == 0)
    for vdtype in (torch.float32, torch.float64):
        levels = level_tensors(dev, hiers, vdtype)
        for odtype in (torch.float32, torch.float64):
            for fold, offset, w in ((False, 0.0, 0.5), (True, 1e-4, 0.5), (False, 1e-4, 0.5), (True, 0.0, 0.3)):
                out, status = run_kernels(dev, levels, GRIDS, odtype, fold, offset, w)
                assert status == 0
                check_against_ref(out, hiers, GRIDS, vdtype, odtype, fold, offset, w, (L, vdtype, odtype, fold, offset, w))


@pytest.mark.parametrize("vdtype", [torch.float32, torch.float64])
def test_padded_rows_are_never_read(dev, vdtype):
    """Rows i >= num_ims[b] of locs and of the values hold huge, negative and NaN patterns: same bits as with zeros there, status 0."""
    hiers = hierarchies(3)
    for fold in (False, True):
        clean, st0 = run_kernels(dev, level_tensors(dev, hiers, vdtype), GRIDS, torch.float64, fold, 1e-4)
        dirty, st1 = run_kernels(dev, level_tensors(dev, hiers, vdtype, hostile=True), GRIDS, torch.float64, fold, 1e-4)
        assert st0 == 0 and st1 == 0
        assert P.same_bits(clean, dirty) and bool(torch.isfinite(dirty).all())


def as_trace(levels, key="importance"):
    return [{"locs": locs, "num_ims": num_ims, key: vals} for locs, num_ims, vals in levels]


def test_out_of_grid_rows_are_reported_and_duplicates_resolve_to_the_later_row(dev):
    from paths_amd import _lib, heatmap as hm
    hiers = hierarchies(3, signed=False, empty=(9, 9))
    # slide 1 (grid (2, 2)), level 1 (grid (4, 4)): a cell inside the batch's padded grid but outside the slide's, one far outside, a
    # negative location; slide 0, level 0: the first cell again as a LATER row with another value
    lv = hiers[1][1]
    bad = np.array([[5 * PATCH, 0], [1000 * PATCH, 3 * PATCH], [-PATCH, 0]], np.int64)
    lv["locs"] = np.concatenate([lv["locs"][:1], bad, lv["locs"][1:]])
    lv["values"] = np.concatenate([lv["values"][:1], np.array([7.0, 8.0, 9.0]), lv["values"][1:]])
    l0 = hiers[0][0]
    l0["locs"] = np.concatenate([l0["locs"], l0["locs"][:1]])
    l0["values"] = np.concatenate([l0["values"], np.array([42.0])])
    levels = level_tensors(dev, hiers, torch.float32)
    out, status = run_kernels(dev, levels, GRIDS, torch.float64, True, 1e-4)
    assert status == 1 << 1                                          # level 1, and only it
    check_against_ref(out, hiers, GRIDS, torch.float32, torch.float64, True, 1e-4, 0.5, "kernels")
    index, skipped = R.index_grid(l0["locs"], GRIDS[0])
    assert skipped == 0 and index[tuple(l0["locs"][0] // PATCH)] == len(l0["locs"]) - 1
    with pytest.raises(_lib.PathsHipError, match=r"level\(s\) 1 hold a location outside"):
        hm.rasterize(as_trace(levels), GRIDS, dtype=torch.float64)
    maps = hm.rasterize(as_trace(levels), GRIDS, dtype=torch.float64, check=False)
    for b, g in enumerate(GRIDS):
        want = R.raster([{"locs": v["locs"], "values": v["values"].astype(np.float32)} for v in hiers[b]], g, offset=1e-4, fold=0.5)
        assert maps[b].shape == want.shape and same_bits(maps[b].cpu().numpy(), want), b
    cx, cy = (int(c) for c in l0["locs"][0] // PATCH)
    assert float(maps[0][4 * cx, 4 * cy]) >= 42.0                   # the later row's value, not the first row's 0.0


@pytest.fixture(scope="module")
def real_records(dev):
    """Two synthetic slides with different level-0 grids through recurse(trace, attention, rollout) and saliency.input_gradients at the
    shipped K = 20 x 5 levels (f = 16); computed once, read-only."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    from paths_amd.saliency import input_gradients
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[20] * 4)
    slides = [DeviceSlide.synthetic(14, sid, base, p_bg=0.1, device=dev) for sid, base in enumerate([(6, 7), (5, 4)])]
    trace = []
    with torch.no_grad():
        putils.recurse(model, slides, cfg.top_k_patches, 5, trace=trace, attention=True, rollout=True)
    _, strace = input_gradients(model, slides, cfg.top_k_patches, 5)
    strace = [{k: (v.detach() if torch.is_tensor(v) else v) for k, v in rec.items()} for rec in strace]
    return cfg, model, slides, trace, strace


def numpy_maps(hm, levels, grid, kind, **kw):
    if kind == "importance":
        return hm.importance_map(levels, grid)
    if kind == "attention":
        return np.stack(hm.attention_map(levels, grid, **kw))
    if kind == "rollout":
        return np.stack(hm.rollout_map(levels, grid))
    return np.stack(hm.saliency_map(levels, grid, kind=kind))


def test_rasterize_equals_the_numpy_maps_on_real_records(dev, real_records):
    from paths_amd import heatmap as hm
    cfg, model, slides, trace, strace = real_records
    grids = [s.shape(0) for s in slides]
    assert len(trace) == 5 and grids[0] != grids[1]
    jobs = [(trace, "importance", {}), (trace, "attention", dict(layer=-1, head=1)), (trace, "attention", dict(layer=0, head=None)),
            (trace, "rollout", {})] + [(strace, k, {}) for k in hm.SALIENCY_KINDS if k in strace[0]]
    assert len(jobs) >= 6
    for tr, kind, kw in jobs:
        hosts = [hm.hierarchy_from_trace(tr, b) for b in range(2)]
        got64 = hm.rasterize(tr, slides, kind, dtype=torch.float64, **kw)
        got32 = hm.rasterize(tr, grids, kind, **kw)
        for b in range(2):
            want = numpy_maps(hm, hosts[b], grids[b], kind, **kw)
            assert want.shape == ((grids[b][0] * 16, grids[b][1] * 16) if kind == "importance" else (5, grids[b][0] * 16, grids[b][1] * 16))
            assert np.count_nonzero(want) > 256
            a64, a32 = got64[b].cpu().numpy(), got32[b].cpu().numpy()
            assert a32.dtype == np.float32 and a64.shape == want.shape == a32.shape
            if kind == "attention" and kw["head"] is None:              # (torch's and NumPy's means may sum in another order)
                assert np.abs(a64 - want).max() <= 1e-12 and np.abs(a32 - want.astype(np.float32)).max() <= 1e-7
            else:
                assert same_bits(a64, want), (kind, b)
                assert same_bits(a32, want.astype(np.float32)), (kind, b)
    # the one new quantity: the cross-level fold of another map, and per-level planes of the importance
    folded = hm.rasterize(trace, slides, "rollout", fold=0.5, dtype=torch.float64)
    planes = hm.rasterize(trace, slides, "importance", fold=False, dtype=torch.float64)
    for b in range(2):
        host = hm.hierarchy_from_trace(trace, b)
        want = R.raster([{"locs": lv["locs"], "values": lv["rollout"]} for lv in host], grids[b], fold=0.5)
        assert same_bits(folded[b].cpu().numpy(), want)
        want = R.raster([{"locs": lv["locs"], "values": lv["importance"]} for lv in host], grids[b], offset=1e-4)
        assert same_bits(planes[b].cpu().numpy(), want)


def test_a_repeat_is_bit_identical(dev, real_records):
    from paths_amd import heatmap as hm
    cfg, model, slides, trace, strace = real_records
    for kind, kw in (("importance", {}), ("attention", dict(head=None)), ("rollout", dict(fold=0.5, dtype=torch.float64))):
        first = [m.clone() for m in hm.rasterize(trace, slides, kind, **kw)]
        again = hm.rasterize(trace, slides, kind, **kw)
        assert all(P.same_bits(a, b) for a, b in zip(first, again)), kind
    hiers = hierarchies(3)
    levels = level_tensors(dev, hiers, torch.float32)
    a, _ = run_kernels(dev, levels, GRIDS, torch.float32, True, 1e-4)
    b, _ = run_kernels(dev, levels, GRIDS, torch.float32, True, 1e-4)
    assert P.same_bits(a, b)


def test_launch_lists(dev, real_records):
    """rasterize: one paths_raster_index per level and one paths_raster_maps, nothing else; recurse() launches what it launched before."""
    from paths_amd import heatmap as hm, utils as putils
    cfg, model, slides, trace, strace = real_records

    def recurse_calls():
        with H.spy_calls() as calls:
            with torch.no_grad():
                putils.recurse(model, slides, cfg.top_k_patches, 5, trace=[], attention=True, rollout=True)
        return list(calls)

    before = recurse_calls()
    for kind, kw in (("importance", {}), ("attention", dict(head=None)), ("rollout", dict(fold=0.5))):
        with H.spy_calls() as calls:
            hm.rasterize(trace, slides, kind, **kw)
        assert calls == ["paths_raster_index"] * 5 + ["paths_raster_maps"], (kind, calls)
    after = recurse_calls()
    assert before == after and len(before) > 20 and not [c for c in before if c.startswith("paths_raster")]
