"""CPU-only tests of the device rasters (paths_amd.heatmap.rasterize, csrc/raster.hip): the NumPy restatement of the two kernels
(tests/raster_ref.py, a gather) against the painting functions of paths_amd.heatmap, the C surface, and every rejection that happens
before a launch.  No kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

from tests import raster_ref as R

GRIDS = ((3, 5), (2, 2), (4, 1), (1, 1))
LEVELS = (1, 2, 3, 5)
PATCH = 256
LAYERS, HEADS = 2, 4


def random_hierarchy(rng, L, grid, dtype=np.float64, empty_below=None, signed=False, cap=None):
    """One slide's levels [{"locs", "values"}]: unique cells per level, children only below visited parents, the last row and column
    visited at every level that has patches, some values exactly 0.0 and -0.0.  ``empty_below``: the first level without any patch;
    ``cap``: at most that many patches per level (the last row and column are then no longer guaranteed)."""
    levels, parents = [], None
    for l in range(L):
        if l == 0:
            cells = np.array([(x, y) for x in range(grid[0]) for y in range(grid[1])], dtype=np.int64)
            keep = rng.random(len(cells)) < 0.7
            keep[-1] = True                                                    # (the cell in the last row and column)
            cells = cells[keep]
        elif empty_below is not None and l >= empty_below or len(parents) == 0:
            cells = np.zeros((0, 2), dtype=np.int64)
        else:
            chosen = parents[rng.random(len(parents)) < 0.6]
            last = parents[np.argmax(parents[:, 0] * 100000 + parents[:, 1])]
            kids = [(2 * px + dx, 2 * py + dy) for px, py in chosen.tolist() for dx in (0, 1) for dy in (0, 1) if rng.random() < 0.8]
            kids.append((2 * int(last[0]) + 1, 2 * int(last[1]) + 1))          # the child in the last row and column of its level
            cells = np.unique(np.array(kids, dtype=np.int64), axis=0)
        cells = cells[rng.permutation(len(cells))][:cap]
        v = rng.standard_normal(len(cells)) if signed else rng.random(len(cells))
        if len(v) > 1:
            v[0], v[1] = 0.0, -0.0
        levels.append({"locs": cells * PATCH, "values": v.astype(dtype)})
        parents = cells
    return levels


def cases():
    rng = np.random.default_rng(20)
    for L in LEVELS:
        for grid in GRIDS:
            yield L, grid, random_hierarchy(rng, L, grid), rng
    yield 3, (3, 5), random_hierarchy(rng, 3, (3, 5), empty_below=1), rng       # nothing below a visited level 0
    yield 5, (2, 2), random_hierarchy(rng, 5, (2, 2), empty_below=3), rng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_raster_ref_is_the_numpy_maps_for_every_kind_rasterize_offers():
    from paths_amd import heatmap as hm
    assert set(hm.RASTER_KINDS) == {"importance", "attention", "rollout", "attention_relevance"} | set(hm.SALIENCY_KINDS)
    n_cases = 0
    for L, grid, levels, rng in cases():
        n_cases += 1
        for kind in hm.RASTER_KINDS:
            signed = kind in hm.SALIENCY_KINDS
            for dtype in (np.float64, np.float32):
                vals = [(lv["values"] * (rng.choice((-1.0, 1.0), len(lv["values"])) if signed else 1.0)).astype(dtype) for lv in levels]
                ref_levels = [{"locs": lv["locs"], "values": v} for lv, v in zip(levels, vals)]
                if kind == "importance":
                    host = [{"locs": lv["locs"], "importance": v} for lv, v in zip(levels, vals)]
                    want = hm.importance_map(host, grid)
                    got = R.raster(ref_levels, grid, offset=1e-4, fold=0.5)
                    assert same_bits(got, want), (L, grid, kind, dtype)
                    assert want[-1, -1] != 0                                   # the last row and column are painted
                    continue
                if kind == "attention":
                    att = [rng.random((LAYERS, HEADS, len(v))).astype(dtype) for v in vals]
                    for a, v in zip(att, vals):
                        a[1, 2] = v
                    host = [{"locs": lv["locs"], "attention": a} for lv, a in zip(levels, att)]
                    want = hm.attention_map(host, grid, layer=1, head=2)
                    mean = hm.attention_map(host, grid, layer=-1, head=None)
                    mref = R.raster([{"locs": lv["locs"], "values": torch.from_numpy(a[-1]).to(torch.float64).mean(dim=0).numpy()}
                                     for lv, a in zip(levels, att)], grid)
                    assert np.abs(mref - np.stack(mean)).max() <= 1e-12, (L, grid)
                    assert same_bits(mref != 0, np.stack(mean) != 0)
                elif kind == "rollout":
                    want = hm.rollout_map([{"locs": lv["locs"], "rollout": v} for lv, v in zip(levels, vals)], grid)
                elif kind == "attention_relevance":
                    want = hm.relevance_map([{"locs": lv["locs"], "attention_relevance": v} for lv, v in zip(levels, vals)], grid)
                else:
                    want = hm.saliency_map([{"locs": lv["locs"], kind: v} for lv, v in zip(levels, vals)], grid, kind=kind)
                got = R.raster(ref_levels, grid)
                assert same_bits(got, np.stack(want)), (L, grid, kind, dtype)
    assert n_cases == len(LEVELS) * len(GRIDS) + 2


def test_raster_ref_index_grid_later_row_wins_and_skips_outside():
    locs = np.array([[0, 0], [256, 512], [0, 0], [768, 0], [0, 1280], [-1, 0]])
    index, skipped = R.index_grid(locs, (3, 5))
    want = np.full((3, 5), -1, np.int32)
    want[0, 0], want[1, 2] = 2, 1
    assert (index == want).all() and skipped == 3
    planes = R.level_planes([{"locs": locs, "values": np.arange(6, dtype=np.float32)}], (3, 5), offset=0.5)
    assert planes[0, 0, 0] == 2.5 and planes[0, 1, 2] == 1.5 and np.count_nonzero(planes) == 2
    # the fold tests the VALUE against zero, not "visited": a deeper 0.0 + 0 offset does not reach the level above
    two = [{"locs": np.array([[0, 0]]), "values": np.array([3.0])}, {"locs": np.array([[0, 0], [256, 256]]), "values": np.array([0.0, 2.0])}]
    assert R.raster(two, (1, 1), fold=0.5).tolist() == [[3.0, 3.0], [3.0, 4.0]]
    assert R.raster(two, (1, 1), fold=0.5, dtype=np.float32).dtype == np.float32


def test_header_declares_and_library_exports_the_raster_entry_points():
    from paths_amd import _lib
    assert _lib.ABI_VERSION == 3
    for name, nargs in (("paths_raster_index", 14), ("paths_raster_maps", 14)):
        assert name in _lib.DECLARATIONS, f"{name} is not declared in include/paths_hip.h"
        res, args = _lib.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == len(_lib.SIGNATURES[name]) == nargs
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "paths_raster_index") and hasattr(raw, "paths_raster_maps")
    assert lib.paths_abi_version() == 3


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)
    ri = lambda locs, ni, gx, gy, level, ps, N, B, GX, GY, index, ldi, status: lib.paths_raster_index(
        locs, ni, gx, gy, level, ps, N, B, GX, GY, index, ldi, status, None)
    ok = dict(locs=A, ni=A, gx=A, gy=A, level=2, ps=256, N=40, B=3, GX=4, GY=5, index=A, ldi=20, status=A)
    for change, word in ((dict(locs=None), b"null"), (dict(ni=None), b"null"), (dict(gx=None), b"null"), (dict(gy=None), b"null"),
                         (dict(index=None), b"null"), (dict(status=None), b"null"), (dict(B=0), b"B = 0"), (dict(B=70000), b"B = 70000"),
                         (dict(N=0), b"N = 0"), (dict(ps=0), b"patch_size"), (dict(level=-1), b"level"), (dict(level=8), b"level"),
                         (dict(GX=0), b"extent"), (dict(GY=0), b"extent"), (dict(ldi=19), b"stride"), (dict(locs=A + 4), b"alignment"),
                         (dict(ni=A + 4), b"alignment"), (dict(index=A + 2), b"alignment"), (dict(status=A + 1), b"alignment"),
                         (dict(gx=A + 2), b"alignment")):
        assert ri(**{**ok, **change}) == -1 and word in lib.paths_last_error(), (change, lib.paths_last_error())
    rm = lambda table, gx, gy, L, B, GX, GY, vf, of, fold, offw, out, ldo: lib.paths_raster_maps(
        table, gx, gy, L, B, GX, GY, vf, of, fold, offw, out, ldo, None)
    ok = dict(table=A, gx=A, gy=A, L=3, B=3, GX=4, GY=5, vf=0, of=0, fold=1, offw=A, out=A, ldo=20)
    for change, word in ((dict(table=None), b"null"), (dict(gx=None), b"null"), (dict(gy=None), b"null"), (dict(offw=None), b"null"),
                         (dict(out=None), b"null"), (dict(B=0), b"B = 0"), (dict(L=0), b"L = 0"), (dict(L=9), b"L = 9"),
                         (dict(GX=0), b"extent"), (dict(GY=-1), b"extent"), (dict(ldo=16), b"stride"), (dict(ldo=22), b"multiple of 4"),
                         (dict(GX=1 << 20, L=8, ldo=1 << 20), b"too large"), (dict(out=A + 8), b"alignment"), (dict(table=A + 4), b"alignment"),
                         (dict(offw=A + 4), b"alignment"), (dict(gy=A + 2), b"alignment")):
        assert rm(**{**ok, **change}) == -1 and word in lib.paths_last_error(), (change, lib.paths_last_error())
    with pytest.raises(_lib.PathsHipError, match=r"paths_raster_maps failed \(-1\)"):
        _lib.call("paths_raster_maps", None, None, None, 3, 2, 4, 5, 0, 0, 1, None, None, 20, None)
    with pytest.raises(_lib.PathsHipError, match=r"paths_raster_index failed \(-1\)"):
        _lib.call("paths_raster_index", None, None, None, None, 0, 256, 40, 2, 4, 5, None, 5, None, None)


def _cpu_trace(L=3, B=2, N=6, with_attention=False):
    trace = []
    for l in range(L):
        rec = {"locs": torch.zeros((B, N, 2), dtype=torch.int64), "num_ims": torch.zeros((B,), dtype=torch.int64),
               "importance": torch.zeros((B, N)), "rollout": torch.zeros((B, N))}
        if with_attention:
            rec["attention"] = torch.zeros((B, LAYERS, HEADS, N))
        trace.append(rec)
    return trace


def test_rasterize_rejects_before_any_launch(monkeypatch):
    from paths_amd import _lib, heatmap as hm
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    grids = [(3, 5), (2, 2)]
    with pytest.raises(_lib.PathsHipError, match="GPU only"):
        hm.rasterize(_cpu_trace(), grids)
    with pytest.raises(ValueError, match="kind must be one of"):
        hm.rasterize(_cpu_trace(), grids, kind="removed")
    with pytest.raises(ValueError, match="magnification_factor"):
        hm.rasterize(_cpu_trace(), grids, magnification_factor=4)
    with pytest.raises(KeyError, match=r"level 0 carries no attention: run recurse\(\.\.\., attention=True\)"):
        hm.rasterize(_cpu_trace(), grids, kind="attention")
    with pytest.raises(KeyError, match="level 0 carries no attention relevance: run saliency.attention_relevance"):
        hm.rasterize(_cpu_trace(), grids, kind="attention_relevance")
    with pytest.raises(KeyError, match="level 0 carries no grad_norm: take the trace from saliency.input_gradients"):
        hm.rasterize(_cpu_trace(), grids, kind="grad_norm")
    partial = _cpu_trace()
    del partial[2]["rollout"], partial[1]["importance"]
    with pytest.raises(KeyError, match=r"level 2 carries no rollout: run recurse\(\.\.\., rollout=True\)"):
        hm.rasterize(partial, grids, kind="rollout")
    with pytest.raises(KeyError, match="importance"):
        hm.rasterize(partial, grids)
    with pytest.raises(ValueError, match="3 grids for the 2 slides"):
        hm.rasterize(_cpu_trace(), grids + [(1, 1)])
    with pytest.raises(ValueError, match="positive"):
        hm.rasterize(_cpu_trace(), [(3, 5), (0, 2)])
    for bad in (dict(layer=LAYERS), dict(layer=-LAYERS - 1), dict(head=HEADS), dict(head=-1)):
        with pytest.raises(IndexError, match="out of range"):
            hm.rasterize(_cpu_trace(with_attention=True), grids, kind="attention", **bad)
    for bad in (torch.float16, torch.int32, np.float64):
        with pytest.raises(ValueError, match="dtype"):
            hm.rasterize(_cpu_trace(), grids, dtype=bad)
    with pytest.raises(ValueError, match="1 to 8 levels"):
        hm.rasterize(_cpu_trace(L=9), grids)
    short = _cpu_trace()
    short[1]["rollout"] = short[1]["rollout"][:, :4]
    with pytest.raises(ValueError, match="level 1: .* do not describe the same"):
        hm.rasterize(short, grids, kind="rollout")
    with pytest.raises(ValueError, match="fold"):
        hm.rasterize(_cpu_trace(), grids, fold=True)
    assert launched == []
    assert "NumPy only" in hm.removed_map.__doc__
