"""CPU tests of the annotation module (paths_amd/annotations.py) and of its NumPy contract (tests/polygon_ref.py): the contract against an
independent exact evaluation in fractions, exact areas, the parser, the fixed-point conversion and every refusal, the per-patch sums and
localisation scores against a direct loop, the outline rule, and the C surface.  The kernels themselves: tests/test_gpu_annotations.py."""
import ctypes
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import polygon_ref as PR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camelyon17_annotation.xml")


# ------------------------------------------------------------------------------------------------
# the contract against exact rational arithmetic
# ------------------------------------------------------------------------------------------------
def contains_fraction(poly, pr: int, pc: int) -> bool:
    """Even-odd rule with the crossing's column as a fraction: an edge counts when exactly one endpoint lies strictly below the
    point's row and the edge meets that row strictly beyond the point's column."""
    inside = False
    n = len(poly)
    for e in range(n):
        (ar, ac), (br, bc) = (int(v) for v in poly[e]), (int(v) for v in poly[(e + 1) % n])
        if (ar > pr) == (br > pr):
            continue
        crossing = Fraction(ac) + Fraction(pr - ar, br - ar) * (bc - ac)
        if crossing > pc:
            inside = not inside
    return inside


def coverage_fraction(polys, X, Y, s):
    off = [((2 * i + 1) << 15) >> (s.bit_length() - 1) for i in range(s)]
    out = np.zeros((X, Y), dtype=np.int32)
    for x in range(X):
        for y in range(Y):
            out[x, y] = sum(any(contains_fraction(p, (x << 16) + oi, (y << 16) + oj) for p in polys) for oi in off for oj in off)
    return out


def small_polygons(seed):
    """Polygons on a 3 x 4 grid: random ones (some vertices outside the grid), a self-intersecting one, one with vertices and a
    horizontal edge exactly on sample coordinates of s = 4, and two that overlap."""
    rng = np.random.default_rng(seed)
    polys = [rng.integers(-(1 << 15), 5 << 16, (int(n), 2)) for n in rng.integers(3, 9, 3)]
    polys.append(np.array([[8192, 8192], [3 << 16, 8192 + (1 << 16)], [8192, 3 << 16], [3 << 16, 3 << 16]]))          # a bow tie
    on = PR.sample_offsets(4)
    polys.append(np.array([[on[1], on[0]], [on[1], (2 << 16) + on[2]], [(1 << 16) + on[3], (2 << 16) + on[2]], [(2 << 16) + on[0], on[0]]]))
    polys += [np.array([[0, 0], [0, 2 << 16], [2 << 16, 2 << 16], [2 << 16, 0]]), np.array([[1 << 16, 1 << 16], [1 << 16, 3 << 16], [3 << 16, 3 << 16], [3 << 16, 1 << 16]])]
    return [p.astype(np.int64) for p in polys]


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_contract_equals_exact_fractions_on_every_sample(s):
    polys = small_polygons(s)
    for subset in ([p] for p in polys):
        assert np.array_equal(PR.coverage(subset, 3, 4, s), coverage_fraction(subset, 3, 4, s))
    assert np.array_equal(PR.coverage(polys, 3, 4, s), coverage_fraction(polys, 3, 4, s))
    assert np.array_equal(PR.coverage([], 3, 4, s), np.zeros((3, 4), np.int32))


def test_contract_at_sixteen_samples_and_parity_hole_and_union():
    polys = small_polygons(16)
    assert np.array_equal(PR.coverage(polys[:5], 2, 3, 16), coverage_fraction(polys[:5], 2, 3, 16))
    # a pentagram: its centre is outside by parity; two overlapping squares: the overlap counts once
    star = np.array([[(2 << 16) + int(np.round(1.9 * 65536 * np.cos(a))), (2 << 16) + int(np.round(1.9 * 65536 * np.sin(a)))]
                     for a in 2 * np.pi * np.arange(5) * 2 / 5], dtype=np.int64)
    centre, arm = PR.contains(star, [2 << 16], [2 << 16]), PR.contains(star, [(2 << 16) + 3 * 32768], [2 << 16])
    assert not centre.any() and arm.all() and 0 < PR.coverage([star], 4, 4, 4).sum() < 16 * 16
    two = small_polygons(0)[-2:]
    assert PR.coverage(two, 3, 3, 4).sum() == (4 + 4 - 1) * 16 and PR.coverage(two[:1], 3, 3, 4).sum() == 4 * 16


def shoelace(poly):
    r, c = poly[:, 0].astype(object), poly[:, 1].astype(object)
    return abs(sum(r[i] * c[(i + 1) % len(poly)] - r[(i + 1) % len(poly)] * c[i] for i in range(len(poly)))) / Fraction(2)


@pytest.mark.parametrize("s", [1, 2, 4, 8, 16])
def test_rectangles_on_cell_boundaries_have_their_exact_area(s):
    for r0, c0, r1, c1 in ((0, 0, 5, 7), (1, 2, 4, 3), (2, 0, 3, 7), (0, 6, 5, 7)):
        for order in (1, -1):
            poly = np.array([[r0, c0], [r0, c1], [r1, c1], [r1, c0]], dtype=np.int64)[::order] << 16
            cover = PR.coverage([poly], 5, 7, s)
            assert Fraction(int(cover.sum()), s * s) * (1 << 32) == shoelace(poly) and cover.max() == s * s
            assert cover[r0:r1, c0:c1].min() == s * s and cover.sum() == (r1 - r0) * (c1 - c0) * s * s
    # tiling polygons count every sample once: the half-open rule
    left = np.array([[0, 0], [0, 3], [5, 3], [5, 0]], dtype=np.int64) << 16
    right = np.array([[0, 3], [0, 7], [5, 7], [5, 3]], dtype=np.int64) << 16
    assert np.array_equal(PR.coverage([left], 5, 7, s) + PR.coverage([right], 5, 7, s), np.full((5, 7), s * s, np.int32))


# ------------------------------------------------------------------------------------------------
# parser, fixed point, refusals
# ------------------------------------------------------------------------------------------------
def test_parser_reads_the_fixture(tmp_path):
    from paths_amd import annotations as A
    polys = A.parse_camelyon17(FIXTURE, 20)
    assert len(polys) == 2 and all(p.dtype == np.float64 for p in polys)
    # (X, Y) at 40x -> (row, col) = (Y, X) * 20 / 40
    assert polys[0].tolist() == [[256.0, 512.0], [256.0, 1536.25], [1024.125, 1536.25], [1024.125, 512.0]]
    assert polys[1].tolist() == [[2500.0, 2000.0], [2500.0, 2100.0], [3000.0, 2050.0]]              # taken in their Order
    assert A.parse_camelyon17(FIXTURE, 40)[0][1].tolist() == [512.0, 3072.5]
    assert A.parse_camelyon17(FIXTURE, 10)[0][2].tolist() == [2048.25 * 0.25, 3072.5 * 0.25]
    with open(FIXTURE) as fh:
        text = fh.read()
    other = tmp_path / "group.xml"
    other.write_text(text.replace('<Group Name="Tumor"', '<Group Name="Exclusion"'))
    with pytest.raises(ValueError, match="group name 'Exclusion'"):
        A.parse_camelyon17(other, 20)
    other = tmp_path / "type.xml"
    other.write_text(text.replace('Name="Annotation 1" Type="Polygon"', 'Name="Annotation 1" Type="Spline"'))
    with pytest.raises(ValueError, match="annotation type 'Spline'"):
        A.parse_camelyon17(other, 20)
    with pytest.raises(ValueError, match="base_power"):
        A.parse_camelyon17(FIXTURE, 0)
    # the parsed polygons go straight into Polygons
    p = A.Polygons([polys], [(16, 16)], 3)
    assert p.V == 7 and p.P == 2 and p.verts[1].tolist() == [256 * 4 * 256, int(np.rint(1536.25 * 4 / 256 * 65536))]


def test_fixed_point_rounds_halves_to_even():
    from paths_amd import annotations as A
    # f = 1, patch_size 256: x = (k + 1/2) / 256 pixels lies exactly between the fixed-point values k and k + 1
    halves = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 1001.5, 1002.5]) / 256.0
    want = [0, 2, 2, 4, 0, -2, -2, 1002, 1002]
    assert A.to_fixed(halves, 1, 256).tolist() == want and PR.fixed(halves, 1, 256).tolist() == want
    p = A.Polygons([[np.stack([halves[:4], halves[:4][::-1]], axis=1)]], [(1, 1)], 1)
    assert p.verts.dtype == np.int32 and p.verts.tolist() == [[0, 4], [2, 2], [2, 2], [4, 0]]
    # f and patch_size enter as x * f / patch_size * 65536: one finest cell is patch_size / f pixels
    assert A.to_fixed([64.0, 96.0], 4, 256).tolist() == [65536, 98304] and A.to_fixed([100.0], 1, 100).tolist() == [65536]
    x = np.random.default_rng(0).uniform(-3000, 90000, 1000)
    assert np.array_equal(A.to_fixed(x, 8, 224), PR.fixed(x, 8, 224))
    assert A.to_fixed(x[:50], 8, 224).tolist() == [float(round(Fraction(v) * 8 / 224 * 65536)) for v in x[:50]]


def test_polygons_layout_and_every_refusal():
    from paths_amd import annotations as A
    tri = np.array([[0.0, 0.0], [0.0, 256.0], [256.0, 0.0]])
    quad = np.array([[10.0, 10.0], [10.0, 500.0], [300.0, 500.0], [300.0, 10.0]])
    p = A.Polygons([[tri, quad], [], [quad]], [(3, 5), (2, 2), (1, 1)], 3)
    assert (p.B, p.L, p.f, p.V, p.P) == (3, 3, 4, 11, 3)
    assert p.poly_off.tolist() == [0, 3, 7, 11] and p.slide_poly.tolist() == [0, 2, 2, 3]
    assert p.next_vertex.tolist() == [1, 2, 0, 4, 5, 6, 3, 8, 9, 10, 7]
    assert [len(p.slide_polygons(b)) for b in range(3)] == [2, 0, 1] and p.finest(0) == (12, 20)
    assert all(v % 4 == 0 for v in p.at.values()) and p.packed.dtype == np.int32 and not p.packed[p.pad_words].any()
    assert p.packed[p.at["verts"]:p.at["verts"] + 22].reshape(11, 2).tolist() == p.verts.tolist()
    assert p.packed[p.at["gx"]:p.at["gx"] + 3].tolist() == [12, 8, 4] and p.packed[p.at["gy"]:p.at["gy"] + 3].tolist() == [20, 8, 4]
    assert p.pad_words.sum() == 2 + 0 + 0 + 1 + 1
    empty = A.Polygons([[], []], [(1, 1), (2, 1)], 2)
    assert empty.V == 0 and empty.P == 0 and empty.slide_poly.tolist() == [0, 0, 0]

    with pytest.raises(ValueError, match=r"finest raster of slide\(s\) \[1\] exceeds 8192"):
        A.Polygons([[tri], [tri]], [(2048, 1), (3, 2049)], 3)
    A.Polygons([[tri]], [(2048, 2048)], 3)                                      # exactly 8,192 cells: accepted
    with pytest.raises(ValueError, match="leaves the fixed-point range"):
        A.Polygons([[np.array([[0.0, 0.0], [0.0, 256.0], [8192 * 256.0 + 1.0, 0.0]])]], [(1, 1)], 1)
    with pytest.raises(ValueError, match="leaves the fixed-point range"):
        A.Polygons([[np.array([[0.0, 0.0], [0.0, 256.0], [256.0, -8192 * 64.0 - 0.25]])]], [(1, 1)], 3)
    edge = A.Polygons([[np.array([[0.0, 0.0], [-8192 * 256.0, 256.0], [8192 * 256.0, 0.0]])]], [(1, 1)], 1)      # +-2**29 itself: accepted
    assert edge.verts[1:, 0].tolist() == [-(1 << 29), 1 << 29]
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            A.Polygons([[np.array([[0.0, 0.0], [0.0, bad], [256.0, 0.0]])]], [(1, 1)], 1)
    with pytest.raises(ValueError, match="n >= 3 vertices"):
        A.Polygons([[tri[:2]]], [(1, 1)], 1)
    with pytest.raises(ValueError, match="n >= 3 vertices"):
        A.Polygons([[np.zeros((4, 3))]], [(1, 1)], 1)
    big = np.zeros((1 << 19, 2))
    A.Polygons([[big, big]], [(1, 1)], 1)                                       # 2**20 vertices: accepted
    with pytest.raises(ValueError, match="more than 1048576 vertices"):
        A.Polygons([[big, big], [tri]], [(1, 1), (1, 1)], 1)
    with pytest.raises(ValueError, match="num_levels"):
        A.Polygons([[tri]], [(1, 1)], 9)
    with pytest.raises(ValueError, match="base_grids"):
        A.Polygons([[tri]], [(1, 1), (2, 2)], 1)
    # the refusals of the entry functions that need no device
    for s in (0, 3, 32, True):
        with pytest.raises(ValueError, match="samples must be one of"):
            A.coverage(p, s)
    images = [torch.zeros((12 * 2, 20 * 2, 3), dtype=torch.uint8), torch.zeros((16, 16, 3), dtype=torch.uint8), torch.zeros((8, 8, 3), dtype=torch.uint8)]
    for kw, word in ((dict(cell_px=0), "cell_px"), (dict(cell_px=65), "cell_px"), (dict(cell_px=2, width=0), "width"), (dict(cell_px=2, width=8), "width"),
                     (dict(cell_px=2, rgb=(0, 0, 256)), "rgb"), (dict(cell_px=4), "image 0 must be")):
        with pytest.raises(ValueError, match=word):
            A.draw(images, p, **kw)
    with pytest.raises(ValueError, match="2 images for the 3 slides"):
        A.draw(images[:2], p, 2)
    far = A.Polygons([[np.array([[-8192 * 256.0, 0.0], [8192 * 256.0, 0.0], [0.0, 8192 * 256.0]])] * 1100], [(1, 1)], 1)
    with pytest.raises(ValueError, match="one call draws fewer than"):
        A.draw([torch.zeros((64, 64, 3), dtype=torch.uint8)], far, 64)
    assert A.positive_count(16, 0.5) == 8 and A.positive_count(16, 0.0) == 0 and A.positive_count(16, 1.0) == 16 and A.positive_count(16, 1.01) == 17
    for total in (1, 3, 16, 49, 4096):
        for thr in (0.1, 0.3, 1 / 3, 0.5, 0.7, 0.9999):
            c = A.positive_count(total, thr)
            assert c / total >= thr and (c == 0 or not (c - 1) / total >= thr)


# ------------------------------------------------------------------------------------------------
# per-patch sums and localisation scores against a direct loop
# ------------------------------------------------------------------------------------------------
def hand_built(seed=3, L=3, grids=((2, 3), (1, 2)), s=4, N=(8, 12, 20)):
    """A trace as recurse(..., trace=[]) leaves it (CPU tensors), finest counts and slides that hold nothing but masks."""
    rng = np.random.default_rng(seed)
    f = 1 << (L - 1)
    cover = [rng.integers(0, s * s + 1, (g[0] * f, g[1] * f)).astype(np.int32) for g in grids]
    cover[0][:f] = 0                                                          # a region without tumour
    cover[1][:] = np.where(cover[1] > 8, s * s, 0)
    masks = [[(rng.random((g[0] << l, g[1] << l)) > 0.25).astype(np.uint8) for l in range(L)] for g in grids]
    trace = []
    for l in range(L):
        locs = rng.integers(-10 ** 6, 10 ** 6, (len(grids), N[l], 2))        # rows of padding hold anything
        num = np.zeros(len(grids), dtype=np.int64)
        for b, g in enumerate(grids):
            cells = [(x, y) for x in range(g[0] << l) for y in range(g[1] << l)]
            n = min(len(cells), N[l] - 1 - b)
            pick = rng.permutation(len(cells))[:n]
            locs[b, :n] = np.array([cells[i] for i in pick]) * 256 + rng.integers(0, 256, (n, 2))
            num[b] = n
        rec = {"locs": torch.from_numpy(locs), "num_ims": torch.from_numpy(num), "importance": torch.from_numpy(rng.random((len(grids), N[l])).astype(np.float32))}
        if l < L - 1:
            count = np.array([max(1, int(n) // 2) for n in num], dtype=np.int64)
            keep = np.stack([np.concatenate([rng.permutation(int(num[b]))[:count[b]], np.zeros(N[l] - count[b], np.int64)]) for b in range(len(grids))])
            rec["keep_idx"], rec["keep_count"] = torch.from_numpy(keep), torch.from_numpy(count)
        trace.append(rec)
    slides = [SimpleNamespace(masks=[torch.from_numpy(m) for m in ms]) for ms in masks]
    return trace, cover, masks, slides


def patch_cover_loop(trace, cover, L):
    out = []
    for l, lv in enumerate(trace):
        size = 1 << (L - 1 - l)
        got = np.zeros(lv["locs"].shape[:2], dtype=np.int32)
        for b in range(len(cover)):
            for i in range(int(lv["num_ims"][b])):
                cx, cy = (lv["locs"][b, i].numpy() // 256).tolist()
                got[b, i] = cover[b][cx * size:(cx + 1) * size, cy * size:(cy + 1) * size].sum()
        out.append(got)
    return out


def localisation_loop(trace, cover, masks, L, s, threshold, scores="importance"):
    from paths_amd import eval as E
    counts = patch_cover_loop(trace, cover, L)
    out = []
    for l, lv in enumerate(trace):
        size = 1 << (L - 1 - l)
        total = (s * size) ** 2
        row = []
        for b in range(len(cover)):
            n = int(lv["num_ims"][b])
            pos = np.array([counts[l][b, i] / total >= threshold for i in range(n)], dtype=bool)
            X, Y = masks[b][l].shape
            tissue = sum(1 for x in range(X) for y in range(Y)
                         if masks[b][l][x, y] and cover[b][x * size:(x + 1) * size, y * size:(y + 1) * size].sum() > 0)
            kept = None
            if "keep_idx" in lv:
                kept = int(sum(pos[int(i)] for i in lv["keep_idx"][b, :int(lv["keep_count"][b])]))
            row.append({"visited": n, "visited_pos": int(pos.sum()), "kept_pos": kept, "tissue_pos": tissue,
                        "recall": pos.sum() / tissue if tissue else float("nan"), "auroc": E.binary_auroc(lv[scores][b, :n].numpy(), pos)})
        out.append(row)
    return out


def test_patch_cover_and_localisation_equal_a_direct_loop():
    from paths_amd import _lib, annotations as A
    trace, cover, masks, slides = hand_built()
    tcover = [torch.from_numpy(c) for c in cover]
    got = A.patch_cover(trace, tcover, 4)
    want = patch_cover_loop(trace, cover, 3)
    for l in range(3):
        assert got[l].dtype == torch.int32 and np.array_equal(got[l].numpy(), want[l]), l
        assert want[l].max() <= (4 << (2 - l)) ** 2 and want[l].any()
    for threshold in (0.5, 0.25, 1.0, 0.0):
        res = A.localisation(trace, slides, tcover, 4, threshold)
        ref = localisation_loop(trace, cover, masks, 3, 4, threshold)
        for l in range(3):
            for b in range(2):
                assert set(res[l][b]) == {"visited", "visited_pos", "kept_pos", "tissue_pos", "recall", "auroc"}
                for key, v in ref[l][b].items():
                    g = res[l][b][key]
                    assert g == v or (isinstance(v, float) and np.isnan(v) and np.isnan(g)), (threshold, l, b, key, g, v)
        assert res[2][0]["kept_pos"] is None and res[0][0]["kept_pos"] is not None
    assert any(r["visited_pos"] not in (0, r["visited"]) for row in A.localisation(trace, slides, tcover, 4) for r in row)
    # another record as the score; a slide without tumour tissue has recall nan
    for lv in trace:
        lv["rollout"] = 1.0 - lv["importance"]
    res = A.localisation(trace, slides, tcover, 4, scores="rollout")
    ref = localisation_loop(trace, cover, masks, 3, 4, 0.5, "rollout")
    assert [[r["auroc"] for r in row] for row in res] == [[r["auroc"] for r in row] for row in ref]
    none = [torch.zeros_like(t) for t in tcover]
    assert all(np.isnan(r["recall"]) and r["tissue_pos"] == 0 and r["auroc"] == 0.5 for row in A.localisation(trace, slides, none, 4) for r in row)
    with pytest.raises(KeyError, match="carries no attention_relevance"):
        A.localisation(trace, slides, tcover, 4, scores="attention_relevance")
    # refusals: a location outside the grid, slides whose level grids are not (X0 << l, Y0 << l)
    far = [dict(lv) for lv in trace]
    far[1]["locs"] = trace[1]["locs"].clone()
    far[1]["locs"][1, 0, 1] = 4 * 256 * 2
    with pytest.raises(_lib.PathsHipError, match=r"level\(s\) 1 hold a location outside"):
        A.patch_cover(far, tcover, 4)
    far[1]["locs"][1, 0, 1] = -1
    with pytest.raises(_lib.PathsHipError, match=r"level\(s\) 1 hold a location outside"):
        A.localisation(far, slides, tcover, 4)
    odd = [slides[0], SimpleNamespace(masks=[slides[1].masks[0], slides[1].masks[1][:, :3], slides[1].masks[2]])]
    with pytest.raises(ValueError, match=r"slide\(s\) 1 do not hold tissue masks"):
        A.localisation(trace, odd, tcover, 4)
    with pytest.raises(ValueError, match="samples must be one of"):
        A.patch_cover(trace, tcover, 5)
    with pytest.raises(ValueError, match=r"cover\[0\] must be an int32 tensor"):
        A.patch_cover(trace, [tcover[0][:7], tcover[1]], 4)


# ------------------------------------------------------------------------------------------------
# the outline rule
# ------------------------------------------------------------------------------------------------
def px(u, v, c=1):
    """A fixed-point vertex inside pixel (u, v) at ``c`` pixels per cell."""
    return np.array([(u << 16) // c + 5, (v << 16) // c + 9], dtype=np.int64)


@pytest.mark.parametrize("a, b", [((2, 3), (2, 11)), ((2, 11), (2, 3)), ((3, 4), (12, 4)), ((12, 4), (3, 4)), ((1, 1), (9, 9)), ((9, 9), (1, 1)),
                                  ((9, 1), (1, 9)), ((0, 0), (13, 4)), ((13, 4), (0, 0)), ((2, 12), (5, 0)), ((5, 0), (2, 12)), ((0, 3), (10, 2)),
                                  ((4, 4), (4, 4)), ((-3, 2), (4, -6)), ((7, 7), (8, 7))])
def test_outline_rule_on_every_kind_of_edge(a, b):
    u, v = PR.edge_pixels(px(*a), px(*b), 1)
    du, dv = b[0] - a[0], b[1] - a[1]
    n = max(abs(du), abs(dv))
    assert len(u) == len(v) == n + 1 and (u[0], v[0]) == a and (u[-1], v[-1]) == b
    for k in range(n + 1):                                                   # floor(k d / n + 1 / 2), exactly
        want = a if n == 0 else tuple(a[i] + (Fraction(k * d, n) + Fraction(1, 2)).__floor__() for i, d in ((0, du), (1, dv)))
        assert (u[k], v[k]) == want, k
    steps = np.stack([np.diff(u), np.diff(v)])
    if n:
        major = 0 if abs(du) >= abs(dv) else 1
        assert (np.abs(steps[major]) == 1).all() and (np.abs(steps[1 - major]) <= 1).all()       # one pixel per step, connected
        assert (steps[major] == np.sign((du, dv)[major])).all()


def test_outline_endpoints_floor_and_squares_are_clipped():
    # the endpoint's pixel is floor(fixed * c / 65536), also for negative coordinates
    for fx, c, want in ((65535, 1, 0), (65536, 1, 1), (-1, 1, -1), (-65536, 4, -4), (-65537, 4, -5), (16383, 4, 0), (16384, 4, 1), (3 << 16, 64, 192)):
        u, _ = PR.edge_pixels((fx, 0), (fx, 0), c)
        assert u.tolist() == [want], (fx, c)
    image = np.zeros((6, 8, 3), dtype=np.uint8)
    PR.draw(image, [np.stack([px(0, 0), px(0, 7), px(5, 7)])], 1, rgb=(1, 2, 3), width=1)
    assert image[0, :, 0].all() and image[:, 7, 1].all() and (image[image.any(axis=2)] == (1, 2, 3)).all()
    closing = {(5 + (Fraction(-5 * k, 7) + Fraction(1, 2)).__floor__(), 7 - k) for k in range(8)}
    want = {(0, v) for v in range(8)} | {(u, 7) for u in range(6)} | closing
    assert {tuple(p) for p in np.argwhere(image.any(axis=2)).tolist()} == want and (3, 4) in closing and (0, 0) in closing
    for width, lo, hi in ((1, 3, 4), (2, 2, 4), (3, 2, 5), (4, 1, 5), (7, 0, 6)):          # from u - width // 2, width pixels, clipped at 6
        image = np.zeros((6, 8, 3), dtype=np.uint8)
        PR.draw(image, [np.stack([px(3, 4), px(3, 4), px(3, 4)])], 1, width=width)
        rows, cols = np.nonzero(image[:, :, 2])
        assert (rows.min(), rows.max() + 1) == (lo, min(hi, 6)) and (cols.min(), cols.max() + 1) == (4 - width // 2, min(4 - width // 2 + width, 8)), width
    image = np.full((4, 4, 3), 7, dtype=np.uint8)
    PR.draw(image, [np.stack([px(-9, -9), px(-9, 20), px(-5, 3)])], 1, width=3)             # wholly outside: nothing is painted
    assert (image == 7).all()


def test_step_table_is_the_rule_s_pixel_count():
    from paths_amd import annotations as A
    rng = np.random.default_rng(5)
    polys = [rng.uniform(-300, 2500, (n, 2)) for n in (3, 7, 4)]
    p = A.Polygons([polys[:2], polys[2:]], [(2, 2), (2, 1)], 3)
    for c in (1, 4, 64):
        cum = A.step_table(p, c)
        assert cum.dtype == np.int64 and cum[0] == 0 and np.array_equal(np.diff(cum), PR.step_counts(p.verts, p.poly_off, c))


# ------------------------------------------------------------------------------------------------
# the C surface
# ------------------------------------------------------------------------------------------------
def test_header_declares_the_polygon_entry_points():
    from paths_amd import _lib
    i, i64, u32, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p
    assert _lib.ABI_VERSION == 3
    assert _lib.DECLARATIONS["paths_polygon_cover"] == (i, [vp, i, vp, i, vp, vp, vp, i, i, i, i, vp, i64, vp])
    assert _lib.DECLARATIONS["paths_polygon_outline"] == (i, [vp, i, vp, i, vp, vp, vp, i, vp, i64, vp, i, i, u32, vp])
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    table = text[text.index(" * annotation polygons"):text.index("#ifndef PATHS_HIP_H")]
    for name in ("paths_polygon_cover", "paths_polygon_outline"):
        assert name + " " in table, f"{name} has no line in the header's undefined-memory table"
    assert "2^61" in text and "every element of the padded allocation is written" in table
    import __graft_entry__ as g
    assert "polygons.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "polygons.hip"))


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "paths_polygon_cover") and hasattr(raw, "paths_polygon_outline") and lib.paths_abi_version() == 3
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)
    cover = dict(verts=A, V=6, poly_off=A, P=2, slide_poly=A, gx=A, gy=A, B=1, X=16, Y=16, samples=4, out=A, ld=16)
    for kw, word in ((dict(samples=3), b"samples = 3"), (dict(samples=32), b"samples = 32"), (dict(verts=None), b"null"), (dict(out=None), b"out is null"),
                     (dict(X=8193), b"extent"), (dict(Y=0), b"extent"), (dict(ld=15), b"stride ld"), (dict(V=(1 << 20) + 1), b"V ="), (dict(P=3), b"P = 3"),
                     (dict(B=0), b"B = 0"), (dict(B=65536), b"B = 65536"), (dict(verts=A + 4), b"alignment"), (dict(gx=A + 2), b"alignment")):
        args = dict(cover, **kw)
        assert lib.paths_polygon_cover(*args.values(), None) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())
    outline = dict(verts=A, V=6, poly_off=A, P=2, slide_poly=A, gx=A, gy=A, B=1, cum=A, steps=10, images=A, cell_px=4, width=1, rgb=255)
    for kw, word in ((dict(cell_px=0), b"cell_px = 0"), (dict(cell_px=65), b"cell_px = 65"), (dict(width=0), b"width = 0"), (dict(width=8), b"width = 8"),
                     (dict(steps=0), b"steps = 0"), (dict(steps=(1 << 31) - 256), b"steps ="), (dict(cum=None), b"null"), (dict(images=A + 4), b"misaligned"),
                     (dict(V=0, P=0), b"no polygon"), (dict(slide_poly=None), b"null")):
        args = dict(outline, **kw)
        assert lib.paths_polygon_outline(*args.values(), None) == -1 and word in lib.paths_last_error(), (kw, lib.paths_last_error())
