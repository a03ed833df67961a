"""The pixel side on the GPU (paths_amd.pixels, csrc/tiles.hip): the grey histogram, the tissue decision with its compaction, the
encoder input and the row scatter against tests/tiles_ref.py bit for bit, under poisoned allocations, on windows into images whose
rows carry 0xA5 padding and on plain batches; then OnDemandSlide / CachedOnDemandSlide over a TileEncoder against a resident twin
built on the host over ALL cells."""
import numpy as np
import pytest
import torch

from tests import poison as PZ
from tests import tiles_ref as TR
from tests.helpers import build_model
from tests.test_gpu_half_grids import assert_same_recursion
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PAD_BYTE = 0xA5
T = 100                         # the grey threshold of the kernel tests
KINDS = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def padded(dev, image, pad, fill=PAD_BYTE):
    """``image`` (uint8 [rows, cols, 3]) on the device inside rows that carry at least ``pad`` more bytes of ``fill`` (the stride is
    the next multiple of 16): a [rows, cols, 3] view with last strides (3, 1)."""
    rows, cols = image.shape[:2]
    stride = (3 * cols + pad + 15) // 16 * 16
    whole = torch.full((rows, stride), fill, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 16 == 0
    view = whole[:, :3 * cols].unflatten(1, (cols, 3))
    view.copy_(torch.from_numpy(np.ascontiguousarray(image)).to(dev))
    return view


def mosaic(tiles, per_row=10):
    """n tiles [n, P, P, 3] laid out as the cells of one level image (white where the last grid row has no tile) and their cells."""
    n, P = tiles.shape[:2]
    X = (n + per_row - 1) // per_row
    image = np.full((X * P, per_row * P, 3), 255, np.uint8)
    cells = np.stack([np.arange(n) // per_row, np.arange(n) % per_row], axis=1)
    for k, (x, y) in enumerate(cells):
        image[x * P:(x + 1) * P, y * P:(y + 1) * P] = tiles[k]
    return image, cells


def windows(dev, tiles, pad):
    """The tiles as windows into a padded mosaic image: the (addresses, stride) pair of pixels.LevelImages, and what keeps it alive."""
    from paths_amd import pixels
    image, cells = mosaic(tiles)
    im = padded(dev, image, pad)
    reader = pixels.LevelImages([im], patch_size=tiles.shape[1])
    return reader(0, torch.from_numpy(cells).to(dev)), im


# ------------------------------------------------------------------------------------------------
# 1. histogram
# ------------------------------------------------------------------------------------------------
HIST_CASES = {"one-16x16": [(16, 16)], "three": [(48, 80), (16, 16), (32, 1040)], "ragged": [(5, 1043), (7, 9), (70, 33)]}


@pytest.mark.parametrize("case", sorted(HIST_CASES))
def test_histogram_equals_the_numpy_contract_and_repeats(dev, case):
    """"ragged": columns that are no multiple of a thread's 16 pixels (the byte-load end of a row), fewer columns than one piece, and
    more rows than workgroups per image."""
    from paths_amd import pixels
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (r, c, 3), dtype=np.uint8) for r, c in HIST_CASES[case]]
    images[0][: images[0].shape[0] // 2] = 255                                   # a constant half: runs of equal grey values
    on_dev = [padded(dev, im, pad) for im, pad in zip(images, (16, 48, 16))]
    want = TR.histogram(images)
    with PZ.poisoned_empty("H"):
        a = pixels.grey_histogram(on_dev)
        b = pixels.grey_histogram(on_dev)
    assert a.dtype == torch.int64 and tuple(a.shape) == (256,)
    assert np.array_equal(a.cpu().numpy(), want) and torch.equal(a, b)
    assert int(a.sum()) == sum(r * c for r, c in HIST_CASES[case])
    assert pixels.otsu_threshold(on_dev) == TR.otsu(want)


def test_histogram_reports_a_refused_image_entry(dev):
    """The C entry point alone (pixels.grey_histogram refuses such images on the host): an entry with a misaligned address, one
    with a stride shorter than its row and one without pixels count nothing and set the status word; the good image still counts."""
    from paths_amd import _lib
    rng = np.random.default_rng(9)
    image = rng.integers(0, 256, (20, 33, 3), dtype=np.uint8)
    im = padded(dev, image, 16)
    good = [im.data_ptr(), im.stride(0), 20, 33]
    for bad, want_status in (([im.data_ptr() + 8, im.stride(0), 20, 33], 1), ([im.data_ptr(), 96, 20, 33], 1), ([im.data_ptr(), im.stride(0), 0, 33], 1), (None, 0)):
        rows = [good] + ([bad] if bad else []) + [good]
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        ws = int(_lib.load().paths_grey_histogram_workspace(len(rows)))
        partials = PZ.fill_(torch.empty((ws,), dtype=torch.uint8, device=dev), "H")
        counts = torch.full((256,), -7, dtype=torch.int64, device=dev)
        status = torch.full((1,), -7, dtype=torch.int32, device=dev)
        _lib.call("paths_grey_histogram", table.data_ptr(), len(rows), partials.data_ptr(), counts.data_ptr(), status.data_ptr(), _lib.stream())
        assert int(status.item()) == want_status
        assert np.array_equal(counts.cpu().numpy(), 2 * TR.histogram([image]))


# ------------------------------------------------------------------------------------------------
# 2. tissue and compaction
# ------------------------------------------------------------------------------------------------
def tissue_tiles(n, P, stride, thr, seed):
    """n tiles: random ones around the threshold, and - where n leaves room - tiles built to hold exactly the passing count of dark
    lattice pixels and one fewer, tiles whose every pixel has g == T (background) and g == T - 1 (tissue), a white and a black one."""
    rng = np.random.default_rng(seed)
    tiles = rng.integers(0, 256, (n, P, P, 3), dtype=np.uint8)
    tiles[rng.random(n) < 0.4] //= 4                                              # dark tiles
    tiles[rng.random(n) < 0.3] = 255
    at = TR.lattice(P, stride)
    need = TR.passing_count(len(at) ** 2, thr)
    special = []
    on = np.zeros((P, P), bool)
    on[np.ix_(at, at)] = True
    lat = np.argwhere(on)
    for count in (need, need - 1):
        t = np.full((P, P, 3), 255, np.uint8)
        t[~on & (np.add.outer(np.arange(P), np.arange(P)) % 3 == 0)] = 0            # dark pixels beside the lattice count nothing
        for i, j in lat[rng.permutation(len(lat))[:max(count, 0)]]:
            t[i, j] = (10, 20, 30)
        special.append(t)
    special += [np.full((P, P, 3), T, np.uint8), np.full((P, P, 3), T - 1, np.uint8), np.full((P, P, 3), 255, np.uint8), np.zeros((P, P, 3), np.uint8)]
    for k, t in zip(rng.permutation(n)[:len(special)] if n >= len(special) else [], special):
        tiles[k] = t
    return tiles, need


def check_tissue(got, want, n):
    counts, flags, order, m, slots = want
    assert got.m == m and got.counts.cpu().numpy().tolist() == counts.tolist()
    assert got.flags.cpu().numpy().tolist() == flags.tolist()
    assert got.order.dtype == torch.int32 and got.order[:m].cpu().numpy().tolist() == order.tolist(), "the stable compaction"
    assert got.slots.cpu().numpy().tolist() == slots.tolist()
    assert tuple(got.counts.shape) == tuple(got.flags.shape) == tuple(got.order.shape) == tuple(got.slots.shape) == (n,)


@pytest.mark.parametrize("P, stride", [(16, 1), (16, 4), (16, 16), (48, 1), (48, 4), (48, 16), (64, 1), (64, 4), (64, 16), (48, 3), (64, 32)])
def test_tissue_equals_the_numpy_contract(dev, P, stride):
    """(48, 3) and (64, 32): strides that do not divide a thread's 16 pixels take the kernel's byte-load form."""
    from paths_amd import pixels
    for n, pad, thr in ((1, 16, 0.1), (65, 48, 0.1), (300, 16, 0.1), (65, 16, 0.5), (65, 16, 0.0)):
        tiles, need = tissue_tiles(n, P, stride, thr, seed=n + P + stride)
        want = TR.tissue(tiles, T, thr, stride)
        if n >= 65:
            assert need in want[0] and (need - 1 in want[0] or need == 0), "a tile at the passing count and one below it"
            size = (P // stride) ** 2
            assert {0, size} <= set(want[0].tolist()), "g == T is background everywhere, g == T - 1 tissue everywhere"
            assert 0 < want[3] < n
        source, keep = windows(dev, tiles, pad)
        with PZ.poisoned_empty("H"):
            got = pixels.tile_tissue(source, T, thr, stride, patch_size=P)
        check_tissue(got, want, n)
        if n == 65:                                                                # the same tiles as a plain batch
            batch = torch.from_numpy(tiles).to(dev)
            with PZ.poisoned_empty("F"):
                check_tissue(pixels.tile_tissue(batch, T, thr, stride), want, n)
        del keep


def test_all_background_gives_m_zero_and_a_misaligned_address_is_refused(dev):
    from paths_amd import pixels
    tiles = np.full((70, 16, 16, 3), 255, np.uint8)
    tiles[3] = T                                                                   # g == T: background
    source, keep = windows(dev, tiles, 16)
    got = pixels.tile_tissue(source, T, patch_size=16)
    assert got.m == 0 and not got.flags.any() and (got.slots == -1).all() and not got.counts.any()
    rows = pixels.scatter_rows(None, got.slots, 70, 128, torch.float16)
    assert rows.dtype == torch.float16 and not rows.view(torch.int16).any()
    # an address that is no multiple of 16 is never followed: count -1, and the call raises
    addresses, stride = source
    bad = addresses.clone()
    bad[5] += 8
    with pytest.raises(ValueError, match="not a multiple of 16"):
        pixels.tile_tissue((bad, stride), T, patch_size=16)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 3. encoder input
# ------------------------------------------------------------------------------------------------
def same_values(got, want):
    """A device tensor holds exactly the float32-representable values of ``want`` (signs of zeros included)."""
    g = got.float().cpu().numpy()
    return g.shape == want.shape and np.array_equal(g, want) and np.array_equal(np.signbit(g), np.signbit(want))


@pytest.mark.parametrize("P", [16, 48, 64])
@pytest.mark.parametrize("dtype", list(KINDS), ids=list(KINDS.values()))
def test_encoder_input_equals_the_table_lookup(dev, dtype, P):
    """P = 16: one thread per row; 48: rows of three pieces; 64: a tile of 256 pieces, one full round of the workgroup."""
    from paths_amd import pixels
    rng = np.random.default_rng(P)
    n = 9
    tiles = rng.integers(0, 256, (n, P, P, 3), dtype=np.uint8)
    tiles[0, :, :, 0], tiles[0, :, :, 1], tiles[0, :, :, 2] = 0, 128, 255           # a tile that tells the channels apart
    order = np.array([5, 2, 8, 0, 7, 123456, -3, 9, 1 << 30], np.int32)             # m = 5; what follows is never read
    d_order = torch.from_numpy(order).to(dev)
    source, keep = windows(dev, tiles, 48 if P == 48 else 16)
    batch = torch.from_numpy(tiles).to(dev)
    for kind in ("to_tensor", "normalize"):
        table = pixels.to_tensor_table(dtype) if kind == "to_tensor" else pixels.normalize_table(MEAN, STD, dtype)
        ref = TR.to_tensor_table(KINDS[dtype]) if kind == "to_tensor" else TR.normalize_table(MEAN, STD, KINDS[dtype])
        d_table = table.to(dev)
        for first, count in ((0, 5), (1, 2), (3, 1), (4, 1)):
            want = TR.encoder_input(tiles, order, first, count, ref)
            for pattern, src in (("H", source), ("F", batch)):
                with PZ.poisoned_empty(pattern):
                    got = pixels.encoder_input(src, d_order, first, count, d_table, patch_size=P)
                assert got.dtype == dtype and tuple(got.shape) == (count, 3, P, P) and got.is_contiguous()
                assert same_values(got, want), (kind, first, count, pattern)       # (H fills the output with NaN: every element was written)
        # what torch computes from the same bytes where the reference computes it: to_tensor on the host (a true division; the device's
        # division by a scalar multiplies by the reciprocal and differs in the last bit), then Normalize
        x = torch.from_numpy(tiles[order[:5]]).permute(0, 3, 1, 2).float().div(255)
        if kind == "normalize":
            x = x.sub(torch.tensor(MEAN).view(1, 3, 1, 1)).div(torch.tensor(STD).view(1, 3, 1, 1))
        assert torch.equal(pixels.encoder_input(batch, d_order, 0, 5, d_table).float().cpu(), x.to(dtype).float())
    del keep


# ------------------------------------------------------------------------------------------------
# 4. rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 132])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16], ids=["to-f32", "to-f16"])
@pytest.mark.parametrize("enc_dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_scatter_rows_equals_the_numpy_contract(dev, enc_dtype, out_dtype, dim):
    """n = 37 at dim 132 in fp16 is an odd number of 8-byte units: the last store is the short one."""
    from paths_amd import pixels
    rng = np.random.default_rng(dim)
    np_enc, np_out = (np.float32 if enc_dtype == torch.float32 else np.float16), (np.float32 if out_dtype == torch.float32 else np.float16)
    for n, share in ((37, 0.5), (1, 1.0), (300, 0.9), (37, 0.0)):
        flags = rng.random(n) < share
        slots = np.full(n, -1, np.int32)
        slots[flags] = np.arange(int(flags.sum()), dtype=np.int32)
        m = int(flags.sum())
        enc = (rng.standard_normal((m, dim)) * 3).astype(np.float32)
        if m:
            enc[0, :8] = (0.0, -0.0, 70000.0, -70000.0, 1e-8, 6.1e-5, 2049.0, 2051.0)      # zeros, overflow, underflow, subnormal, ties
        with np.errstate(over="ignore"):
            enc = enc.astype(np_enc)
        want = TR.scatter_rows(enc, slots, dim, np_out)
        with PZ.poisoned_empty("H"):
            got = pixels.scatter_rows(torch.from_numpy(enc).to(dev) if m else None, torch.from_numpy(slots).to(dev), n, dim, out_dtype)
        assert got.dtype == out_dtype and tuple(got.shape) == (n, dim)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (n, share)


def test_indices_outside_their_range_are_not_followed(dev):
    """What the header promises for an index that names nothing: an ``order`` entry outside [0, n) that IS read gives a tile of zero
    bytes, i.e. table[c][0] in every element of channel c; a slot outside [0, m) gives a zero row."""
    from paths_amd import pixels
    rng = np.random.default_rng(21)
    P, n = 16, 6
    tiles = rng.integers(1, 256, (n, P, P, 3), dtype=np.uint8)
    table = pixels.normalize_table(MEAN, STD, torch.float16)
    order = torch.tensor([4, -3, 1, n, 1 << 30, 0], dtype=torch.int32, device=dev)
    with PZ.poisoned_empty("H"):
        got = pixels.encoder_input(torch.from_numpy(tiles).to(dev), order, 0, n, table.to(dev)).cpu()
    ref = TR.normalize_table(MEAN, STD, "float16")
    for i, k in enumerate(order.cpu().tolist()):
        source = tiles[k] if 0 <= k < n else np.zeros((P, P, 3), np.uint8)
        want = TR.encoder_input(source[None], [0], 0, 1, ref)[0]
        assert np.array_equal(got[i].float().numpy(), want), (i, k)
        if not 0 <= k < n:
            assert all(bool((got[i, c] == table[c, 0]).all()) for c in range(3)) and bool((got[i] != 0).all())
    enc = rng.standard_normal((2, 132)).astype(np.float32)
    slots = np.array([1, 2, -1, 0, 1 << 30, -(1 << 31), 5], np.int32)              # m = 2: slots 2, 5 and 2^30 name no row
    with PZ.poisoned_empty("H"):
        rows = pixels.scatter_rows(torch.from_numpy(enc).to(dev), torch.from_numpy(slots).to(dev), 7, 132, torch.float16).cpu().numpy()
    want = np.zeros((7, 132), np.float16)
    want[0], want[3] = enc[1].astype(np.float16), enc[0].astype(np.float16)
    assert rows.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------
# 5. end to end: OnDemandSlide over a TileEncoder against a resident twin built on the host over all cells
# ------------------------------------------------------------------------------------------------
P0, DIM, KEEP, LEVELS = 16, 128, [12, 12], 3
PICK = np.sort(np.random.default_rng(77).choice(3 * P0 * P0, DIM, replace=False))


def level_images(grid, seed, blank_children_of=None, no_tissue_below=False):
    """Random dark pixels, about a third of the cells of every level painted white; ``blank_children_of``: a level-0 cell that keeps
    its tissue and loses all four children; ``no_tissue_below``: levels 1.. are white."""
    rng = np.random.default_rng(seed)
    images = []
    for l in range(LEVELS):
        X, Y = grid[0] << l, grid[1] << l
        im = rng.integers(0, 150, (X * P0, Y * P0, 3), dtype=np.uint8)
        blank = rng.random((X, Y)) < 1 / 3
        if l == 0:
            blank[0, 0] = False
        if blank_children_of is not None:
            x, y = blank_children_of
            if l == 0:
                blank[x, y] = False
            if l == 1:
                blank[2 * x:2 * x + 2, 2 * y:2 * y + 2] = True
        if no_tissue_below and l >= 1:
            blank[:] = True
        im[np.repeat(np.repeat(blank, P0, axis=0), P0, axis=1)] = 255
        images.append(im)
    return images


def pick_model(x):
    """128 fixed elements of the input: exact, and independent of the batch it is called with."""
    return x.flatten(1)[:, torch.from_numpy(PICK).to(x.device)]


def build_side(dev, grids, seeds, cached=False, **kw):
    """Per slide: the level images on the device (padded rows), a TileEncoder fitted on the level-0 image, the on-demand slide over
    it - and the host twin: tests/tiles_ref.py over ALL cells of every level."""
    from paths_amd import pixels
    from paths_amd.data_utils.slide import CachedOnDemandSlide, DeviceSlide, OnDemandSlide
    od, twins, encoders, calls = [], [], [], []
    ref_table = TR.to_tensor_table("float16")
    for j, (grid, seed) in enumerate(zip(grids, seeds)):
        images = level_images(grid, seed, **(kw if j == len(grids) - 1 else {}))
        on_dev = [padded(dev, im, 16 if l % 2 == 0 else 48) for l, im in enumerate(images)]
        t = TR.otsu(TR.histogram(images[:1]))
        assert 100 < t < 255

        def model(x, j=j):
            calls.append((j, int(x.shape[0])))
            return pick_model(x)

        enc = pixels.TileEncoder.fit(on_dev[:1], pixels.LevelImages(on_dev, patch_size=P0), model, DIM, patch_size=P0, batch=40)
        assert enc.threshold == t
        shapes = [(grid[0] << l, grid[1] << l) for l in range(LEVELS)]
        od.append((CachedOnDemandSlide if cached else OnDemandSlide)(shapes, enc, DIM, dev, slide_id=f"pixels-{j}"))
        grids_host = [TR.encode_level(im, P0, t, ref_table, lambda x: x.reshape(len(x), -1)[:, PICK], DIM, np.float32) for im in images]
        twins.append(DeviceSlide.from_host([torch.from_numpy(g) for g in grids_host], dev))
        encoders.append(enc)
    return od, twins, encoders, calls


def run(model, slides):
    from paths_amd import utils as putils
    trace = []
    with torch.no_grad():
        out = putils.recurse(model, slides, KEEP, LEVELS, trace=trace)
    torch.cuda.synchronize()
    return trace, out


@pytest.fixture(scope="module")
def paths_model(dev):
    return build_model(dev, 0, {"model_config": {"patch_embed_dim": DIM}, "num_levels": LEVELS}, top_k_patches=KEEP)[1]


def check_requests(od, tb):
    """requested[0] is every cell; requested[l] is exactly the in-bounds children of the patches the twin kept."""
    for j, s in enumerate(od):
        X, Y = s.shape(0)
        assert torch.equal(s.requested[0].cpu(), torch.cartesian_prod(torch.arange(X), torch.arange(Y)))
        for l in range(1, LEVELS):
            c = int(tb[l - 1]["keep_count"][j])
            kept = (tb[l - 1]["locs"][j][tb[l - 1]["keep_idx"][j, :c].long()].cpu().numpy() // 256).tolist()
            X, Y = s.shape(l)
            allowed = {(2 * x + dx, 2 * y + dy) for x, y in kept for dx in (0, 1) for dy in (0, 1) if 2 * x + dx < X and 2 * y + dy < Y}
            asked = [tuple(q) for q in s.requested[l].cpu().tolist()]
            assert len(set(asked)) == len(asked) and set(asked) == allowed, f"slide {j} level {l}"


def test_on_demand_over_pixels_is_bitwise_the_host_twin(dev, paths_model):
    od, twins, encoders, calls = build_side(dev, [(3, 5), (2, 2)], [1, 2], blank_children_of=(0, 0))
    tb, ob = run(paths_model, twins)
    assert int(ob["status"].item()) == 0
    with PZ.poisoned_empty("H"):
        ta, oa = run(paths_model, od)
    assert int(oa["status"].item()) == 0
    assert_same_recursion(ta, tb, oa, ob)
    check_requests(od, tb)
    kept0 = (tb[0]["locs"][1][tb[0]["keep_idx"][1, :int(tb[0]["keep_count"][1])].long()].cpu().numpy() // 256).tolist()
    assert [0, 0] in kept0, "the (2, 2) slide keeps the parent whose four children are background"
    for j, (s, e) in enumerate(zip(od, encoders)):
        req, tis = e.stats["requested"], e.stats["tissue"]
        assert [req[l] for l in range(LEVELS)] == [int(s.requested[l].shape[0]) for l in range(LEVELS)]
        assert sum(tis.values()) < sum(req.values()), "fewer model rows than requested cells"
        assert sum(n for k, n in calls if k == j) == sum(tis.values()) and all(n <= 40 for _, n in calls)
        assert e.stats["model_calls"] == {l: -(-tis[l] // 40) for l in range(LEVELS)}
        total = sum(x * y for x, y in s.shapes)
        assert sum(req.values()) < total
    share = 1 - sum(sum(e.stats["tissue"].values()) for e in encoders) / sum(sum(e.stats["requested"].values()) for e in encoders)
    assert 0.15 < share < 0.6, f"about a third of the requested cells are background (got {share:.2f})"


def test_a_second_pass_through_the_cache_calls_no_model(dev, paths_model):
    od, twins, encoders, calls = build_side(dev, [(3, 5), (2, 2)], [1, 2], cached=True, blank_children_of=(0, 0))
    tb, ob = run(paths_model, twins)
    ta, oa = run(paths_model, od)
    assert_same_recursion(ta, tb, oa, ob)
    n_calls, stats = len(calls), [dict(e.stats["requested"]) for e in encoders]
    assert n_calls > 0
    t2, o2 = run(paths_model, od)
    assert_same_recursion(t2, tb, o2, ob)
    assert len(calls) == n_calls and [dict(e.stats["requested"]) for e in encoders] == stats, "the warm pass asks neither reader nor model"
    assert all(s.stats["hits"] == s.count for s in od)


def test_no_tissue_among_the_requested_cells_raises(dev, paths_model):
    from paths_amd import _lib
    od, _, encoders, _ = build_side(dev, [(2, 2)], [4], no_tissue_below=True)
    with torch.no_grad(), pytest.raises(_lib.PathsHipError, match=r"on-demand slide .*pixels-0"):
        run(paths_model, od)
    torch.cuda.synchronize()
    assert encoders[0].stats["tissue"][1] == 0 and encoders[0].stats["model_calls"][1] == 0
