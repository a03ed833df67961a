"""The row cache of on-demand slides on the GPU: paths_cache_probe and both fills against tests/cache_ref.py byte for byte over
sentinel-filled outputs; the recursion on CachedOnDemandSlide.from_slide(s) against the resident slides, bit for bit, cold, warm, under
another model, with a bounded cache; its launch list; and the hand-over of the visited part as a stored slide."""
import re

import numpy as np
import pytest
import torch

from tests import cache_ref as R
from tests.helpers import build_model, spy_calls
from tests.test_gpu_half_grids import assert_same_recursion
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16 = torch.float16
FILL = -7
KEEP = [12] * 4


def _chunk():
    from paths_amd import _lib
    return int(re.search(r"#define PATHS_CACHE_PROBE_CHUNK (\d+)", open(_lib.HEADER_PATH).read()).group(1))


def _sizes():
    """The wave, workgroup and chunk-carry edges; the kernel's own chunk size +- 1 if it is not 1,024."""
    ns, c = [1, 63, 64, 65, 1024, 1025, 4097], _chunk()
    return sorted(set(ns + [c - 1, c, c + 1]))


# ------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ------------------------------------------------------------------------------------------------
def _case(n, hit, cut, D, np_dtype, seed=0):
    """B = 3 slides: n cells, none, and about n / 2 cells of grids a little larger than the request.  ``hit``: 0, 1 or 0.5 (every
    other position of the request: hits and misses alternate inside a wave).  ``cut``: the store has room for none ("zero"), half
    ("middle") or all ("none") of the misses.  Returns the host-side state (lists per slide)."""
    rng = np.random.default_rng(seed + n)
    ns = [n, 0, max(1, n // 2)]
    cells, index, store, count, capacity, enc = [], [], [], [], [], []
    for b, nb in enumerate(ns):
        X, Y = 70, nb // 70 + 2 + b
        lin = rng.permutation(X * Y)[:nb]
        c = np.stack([lin // Y, lin % Y], axis=1).astype(np.int64)
        is_hit = np.ones(nb, bool) if hit == 1 else np.zeros(nb, bool) if hit == 0 else (np.arange(nb) % 2 == 0)
        h = int(is_hit.sum())
        cnt = h + 3                                                      # three stored rows nobody asks for
        ix = np.full((X, Y), -1, np.int32)
        rows = rng.permutation(cnt)
        ix[c[is_hit, 0], c[is_hit, 1]] = rows[:h]
        others = np.setdiff1d(np.arange(X * Y), lin)[:3]
        ix[others // Y, others % Y] = rows[h:]
        m = nb - h
        cap = cnt + {"zero": 0, "middle": m // 2, "none": m + 3}[cut]
        st = rng.standard_normal((cap, D)).astype(np_dtype)
        st[cnt:] = FILL
        cells.append(c); index.append(ix); store.append(st); count.append(cnt); capacity.append(cap)
        enc.append(rng.standard_normal((m, D)).astype(np_dtype) if m else None)
    return ns, cells, index, store, count, capacity, enc


def _run(dev, ns, cells, index, store, count, capacity, enc, D, dtype, n_max):
    """probe + fill on the device over sentinel-filled outputs -> everything they may write, as NumPy arrays."""
    from paths_amd import _lib
    B = len(ns)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_cells = [t(c) if len(c) else torch.empty((0, 2), dtype=torch.int64, device=dev) for c in cells]
    d_index, d_store = [t(ix) for ix in index], [t(s) for s in store]
    d_enc = [None if e is None else t(e) for e in enc]
    table = lambda vals: torch.tensor(vals, dtype=torch.int64, device=dev)
    ptrs = lambda ts: table([0 if x is None else x.data_ptr() for x in ts])
    tc, tn, ti, te, ts = ptrs(d_cells), table(ns), ptrs(d_index), ptrs(d_enc), ptrs(d_store)
    tcount, tcap = table(count), table(capacity)
    gx = torch.tensor([ix.shape[0] for ix in index], dtype=torch.int32, device=dev)
    gy = torch.tensor([ix.shape[1] for ix in index], dtype=torch.int32, device=dev)
    src = torch.full((B, n_max), FILL, dtype=torch.int32, device=dev)
    mc = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    mcells = torch.full((B, n_max, 2), FILL, dtype=torch.int64, device=dev)
    status = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    out = torch.full((B, n_max, D), FILL, dtype=dtype, device=dev)
    p = lambda x: x.data_ptr()
    _lib.call("paths_cache_probe", p(tc), p(tn), p(ti), p(gx), p(gy), B, n_max, D, p(src), p(mc), p(mcells), p(status), _lib.stream())
    _lib.call("paths_cache_fill" + ("_h16" if dtype == F16 else ""), p(tc), p(tn), p(src), p(mc), p(te), p(ts), p(tcount), p(tcap), p(ti),
              p(gx), p(gy), B, n_max, D, p(out), _lib.stream())
    torch.cuda.synchronize()
    host = lambda x: x.cpu().numpy()
    return dict(src=host(src), miss_count=host(mc), miss_cells=host(mcells), status=host(status), out=host(out),
                index=[host(x) for x in d_index], store=[host(x) for x in d_store])


def _ref(ns, cells, index, store, count, capacity, enc, D, np_dtype, n_max):
    B = len(ns)
    index, store = [ix.copy() for ix in index], [s.copy() for s in store]
    src, mc = np.full((B, n_max), FILL, np.int32), np.full((B,), FILL, np.int32)
    mcells, status = np.full((B, n_max, 2), FILL, np.int64), np.full((B,), FILL, np.int32)
    out = np.full((B, n_max, D), FILL, np_dtype)
    R.probe(cells, ns, index, src, mc, mcells, status)
    new = R.fill(cells, ns, src, mc, enc, store, count, capacity, index, out)
    return dict(src=src, miss_count=mc, miss_cells=mcells, status=status, out=out, index=index, store=store), new


def _same_bytes(got, want, what):
    for k in want:
        pairs = zip(got[k], want[k]) if isinstance(want[k], list) else [(got[k], want[k])]
        for b, (g, w) in enumerate(pairs):
            assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k}"
            assert g.tobytes() == w.tobytes(), f"{what}: {k}[{b}] differs in {int((g != w).sum())} elements"


FORMS = [(torch.float32, np.float32, 4), (torch.float32, np.float32, 1024), (F16, np.float16, 4), (F16, np.float16, 12), (F16, np.float16, 1024)]


@pytest.mark.parametrize("dtype, np_dtype, D", FORMS, ids=["f32-4", "f32-1024", "f16-4", "f16-12", "f16-1024"])
@pytest.mark.parametrize("cut", ["zero", "middle", "none"])
def test_probe_and_fill_equal_the_numpy_contract(dev, dtype, np_dtype, D, cut):
    """Every n at hit fraction 1/2 (n_max a little above n: rows behind n are zeroed); hit fractions 0 and 1 at n = 65 and at the
    first size with a chunk carry.  D = 12 in fp16 is a 24-byte row: the 8-byte pieces."""
    c = _chunk()
    cases = [(n, 0.5) for n in _sizes()] + [(n, h) for n in (65, c + 1) for h in (0, 1)]
    if D == 1024:                                   # (the same paths at fewer sizes: the NumPy side copies 4 KiB per row)
        cases = [(n, h) for n, h in cases if n in (1, 65, c + 1)]
    for n, hit in cases:
        state = _case(n, hit, cut, D, np_dtype)
        n_max = n + 2
        want, new = _ref(*state, D, np_dtype, n_max)
        got = _run(dev, *state, D, dtype, n_max)
        _same_bytes(got, want, f"n {n} hit {hit}")
        m = [nb - int((want["src"][b, :nb] >= 0).sum()) for b, nb in enumerate(state[0])]
        assert want["miss_count"].tolist() == m and want["status"].tolist() == [0, 0, 0]
        room = {"zero": [0, 0, 0], "middle": [x // 2 for x in m], "none": m}[cut]
        assert new == [cnt + r for cnt, r in zip(state[4], room)], "the capacity cuts the misses where the case says"
        if hit == 0.5 and n >= 64:
            assert (want["src"][0, :64] >= 0).tolist() == [i % 2 == 0 for i in range(64)], "hits and misses alternate inside a wave"


def test_a_rerun_is_identical_and_an_outside_cell_reads_as_zeros(dev):
    state = list(_case(1025, 0.5, "middle", 12, np.float16, seed=3))
    state[1][0][7] = (70, 0)                         # slide 0 asks for a cell outside its 70 x Y grid (at a miss position)
    state[1][2][0] = (0, -1)                         # ... and slide 2 at a hit position: both read as zero rows, neither is a miss
    want, _ = _ref(*state, 12, np.float16, 1030)
    a = _run(dev, *state, 12, F16, 1030)
    b = _run(dev, *state, 12, F16, 1030)
    _same_bytes(a, want, "outside cells")
    _same_bytes(b, a, "rerun")
    assert want["status"].tolist() == [1, 0, 1] and want["src"][0, 7] == R.SRC_NONE and (want["out"][0, 7] == 0).all()


def test_bad_arguments_return_minus_one_and_write_nothing(dev):
    from paths_amd import _lib
    lib = _lib.load()
    z = torch.full((256,), FILL, dtype=torch.int64, device=dev)
    a, st = z.data_ptr(), _lib.stream()
    probe = lambda **kw: [kw.get("cells", a), a, a, a, a, kw.get("B", 1), kw.get("n_max", 2), kw.get("D", 4), a, a, a, kw.get("status", a), st]
    fill = lambda **kw: [kw.get("cells", a), a, a, a, a, a, a, a, a, a, a, kw.get("B", 1), kw.get("n_max", 2), kw.get("D", 4), kw.get("out", a), st]
    bad = (dict(B=0), dict(B=-1), dict(n_max=0), dict(D=0), dict(D=6), dict(D=-4), dict(cells=None))
    for kw in bad:
        assert "cells" in kw or R.check_args(kw.get("B", 1), kw.get("n_max", 2), kw.get("D", 4)) == -1
        assert lib.paths_cache_probe(*probe(**kw)) == -1 and b"cache_probe" in lib.paths_last_error()
        for name in ("paths_cache_fill", "paths_cache_fill_h16"):
            assert getattr(lib, name)(*fill(**kw)) == -1 and b"cache_fill" in lib.paths_last_error()
    assert lib.paths_cache_probe(*probe(status=None)) == -1 and lib.paths_cache_fill(*fill(out=None)) == -1
    assert lib.paths_cache_fill(*fill(out=a + 8)) == -1, "out is 16-byte aligned"
    with pytest.raises(_lib.PathsHipError, match=r"paths_cache_probe failed \(-1\)"):
        _lib.call("paths_cache_probe", *probe(B=0))
    torch.cuda.synchronize()
    assert bool((z == FILL).all()), "nothing was launched"


# ------------------------------------------------------------------------------------------------
# 2. the recursion on a caching slide is the recursion on its resident twin, bit for bit
# ------------------------------------------------------------------------------------------------
def _slides(dev, dtype=torch.float32, max_rows=None):
    """tests/test_gpu_on_demand.py's two synthetic slides, base (7, 6), as resident slides and as their caching twins, whose
    encoders are counted."""
    from paths_amd.data_utils.slide import CachedOnDemandSlide, DeviceSlide
    res = [DeviceSlide.synthetic(41, sid, (7, 6), device=dev, dtype=dtype) for sid in range(2)]
    od = [CachedOnDemandSlide.from_slide(s, max_rows=max_rows) for s in res]
    calls = []
    for s in od:
        s.encode = (lambda enc, sid: lambda level, cells: (calls.append((sid, level, int(cells.shape[0]))), enc(level, cells))[1])(s.encode, s.slide_id)
    return od, res, calls


def _pass(model, slides, **kw):
    from paths_amd import utils as putils
    trace = []
    with torch.no_grad():
        out = putils.recurse(model, slides, KEEP, 5, trace=trace, **kw)
    torch.cuda.synchronize()
    assert int(out["status"].item()) == 0
    return trace, out


def _cellset(t):
    return set(map(tuple, t.cpu().tolist()))


@pytest.fixture(scope="module")
def models(dev):
    return build_model(dev, 0, None, top_k_patches=KEEP)[1], build_model(dev, 5, None, top_k_patches=KEEP)[1]


@pytest.mark.parametrize("dtype", [torch.float32, F16])
def test_three_passes_are_bitwise_the_resident_twin(dev, dtype, models):
    model, other = models
    od, res, calls = _slides(dev, dtype)
    tb, ob = _pass(model, res)
    # pass 1: cold - everything asked is encoded and stored
    ta, oa = _pass(model, od)
    assert_same_recursion(ta, tb, oa, ob)
    first = []
    for s in od:
        assert all(torch.equal(s.encoded[l], s.requested[l]) for l in range(5)), "a cold cache encodes what is requested"
        assert s.count == [int(r.shape[0]) for r in s.requested] == s.stats["misses"] == s.stats["stored"] and s.stats["hits"] == [0] * 5
        first.append([_cellset(r) for r in s.requested])
    assert len(calls) == 10
    # pass 2: warm, same model - bitwise pass 1, the encoder is not called once
    del calls[:]
    t2, o2 = _pass(model, od)
    assert_same_recursion(t2, ta, o2, oa)
    assert calls == [] and all(int(s.encoded[l].shape[0]) == 0 for s in od for l in range(5))
    assert all(s.stats["hits"] == s.count and s.stats["requests"] == [2 * c for c in s.count] for s in od)
    # pass 3: another model - its resident twin; only what was not stored is encoded; the store is the union
    t3r, o3r = _pass(other, res)
    t3, o3 = _pass(other, od)
    assert_same_recursion(t3, t3r, o3, o3r)
    grew = False
    for s, had in zip(od, first):
        for l in range(5):
            asked, enc = _cellset(s.requested[l]), _cellset(s.encoded[l])
            assert not enc & had[l] and enc == asked - had[l] and len(enc) == int(s.encoded[l].shape[0]), f"level {l}"
            assert s.count[l] == len(asked | had[l])
            grew |= bool(enc)
    assert grew, "the second model visits cells the first did not (pick another seed otherwise)"
    assert sum(n for _, _, n in calls) == sum(int(s.encoded[l].shape[0]) for s in od for l in range(5)) and all(n >= 1 for _, _, n in calls)


def test_exports_on_a_warm_cache_equal_the_twin(dev, models):
    model, _ = models
    od, res, calls = _slides(dev)
    _pass(model, od)
    del calls[:]
    ta, oa = _pass(model, od, attention=True, rollout=True)
    tb, ob = _pass(model, res, attention=True, rollout=True)
    assert_same_recursion(ta, tb, oa, ob)
    assert calls == []
    for l, (a, b) in enumerate(zip(ta, tb)):
        for key in ("attention", "attention_self", "rollout", "rollout_self"):
            assert torch.equal(a[key], b[key]), f"level {l}: {key}"


def test_a_bounded_cache_changes_no_result(dev, models):
    model, _ = models
    od, res, calls = _slides(dev, max_rows=5)
    tb, ob = _pass(model, res)
    ta, oa = _pass(model, od)
    assert_same_recursion(ta, tb, oa, ob)
    stored = []
    for s in od:
        assert all(c <= 5 for c in s.count) and s.count[0] == 5
        coords = s.export_patches()[0]
        assert all(torch.equal(coords[l], s.requested[l][:s.count[l]]) for l in range(5)), "the first misses in request order are kept"
        stored.append([_cellset(c) for c in coords])
    t2, o2 = _pass(model, od)
    assert_same_recursion(t2, tb, o2, ob)
    for s, had in zip(od, stored):
        for l in range(5):
            want = [c for c in s.requested[l].cpu().tolist() if tuple(c) not in had[l]]
            assert s.encoded[l].cpu().tolist() == want, f"level {l}: exactly the requested cells that are not stored, in request order"
            assert s.count[l] <= 5


def test_launch_lists(dev, models):
    """A caching pass launches the plain on-demand pass's list plus one probe and one fill per level; plain and resident passes
    contain neither."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import OnDemandSlide
    model, _ = models
    for dtype, sfx in ((torch.float32, ""), (F16, "_h16")):
        od, res, _ = _slides(dev, dtype)
        plain = [OnDemandSlide.from_slide(s) for s in res]
        with torch.no_grad():
            putils.recurse(model, res, KEEP, 5)            # (weight images are packed once per model and mode)
            lists = []
            for slides in (od, od, plain, res):            # a cold and a warm caching pass
                with spy_calls() as calls:
                    putils.recurse(model, slides, KEEP, 5)
                lists.append(list(calls))
        torch.cuda.synchronize()
        cold, warm, pl, rs = lists
        cache = ("paths_cache_probe", "paths_cache_fill" + sfx)
        for c in (cold, warm):
            assert c.count(cache[0]) == c.count(cache[1]) == 5
            assert [n for n in c if n not in cache] == pl
            i = [k for k, n in enumerate(c) if n in cache]
            assert [c[k] for k in i] == list(cache) * 5 and all(b == a + 1 for a, b in zip(i[::2], i[1::2])), "probe, then fill, per level"
        assert not [n for n in pl + rs if n.startswith("paths_cache_")]


# ------------------------------------------------------------------------------------------------
# 3. handing the visited part over
# ------------------------------------------------------------------------------------------------
def _kept_cells(trace, l, j, patch=256):
    c = int(trace[l]["keep_count"][j])
    return _cellset(trace[l]["locs"][j][trace[l]["keep_idx"][j, :c].long()] // patch)


@pytest.mark.parametrize("dtype", [torch.float32, F16])
def test_visited_is_a_stored_slide_with_the_same_results(dev, dtype, models):
    from paths_amd import saliency
    from paths_amd.data_utils.slide import DeviceSlide, uncached_children
    model, other = models
    od, res, calls = _slides(dev, dtype)
    ta, oa = _pass(model, od)
    vis = [s.visited() for s in od]
    assert all(isinstance(v, DeviceSlide) and v.packed and v.dtype == dtype and not v.on_demand for v in vis)
    assert [int(v.rows[l].shape[0]) for v in vis for l in range(5)] == [s.count[l] for s in od for l in range(5)]
    del calls[:]
    tv, ov = _pass(model, vis)
    tb, ob = _pass(model, res)
    assert_same_recursion(tv, tb, ov, ob)
    gv, sv = saliency.input_gradients(model, vis, KEEP, 5)
    gb, sb = saliency.input_gradients(model, res, KEEP, 5)
    assert torch.equal(gv["logits"], gb["logits"]) and torch.equal(gv["target"], gb["target"])
    for l, (a, b) in enumerate(zip(sv, sb)):
        for key in ("num_ims", "locs", "importance", "grad_x_input", "grad_norm"):
            assert torch.equal(a[key], b[key]), f"level {l}: {key}"
    if dtype == torch.float32:
        _, rv = saliency.attention_relevance(model, vis, KEEP, 5)
        _, rb = saliency.attention_relevance(model, res, KEEP, 5)
        for l, (a, b) in enumerate(zip(rv, rb)):
            for key in ("attention_relevance", "attention_relevance_self", "grad_x_input"):
                assert torch.equal(a[key], b[key]), f"level {l}: {key}"
    assert calls == [], "a stored slide asks no encoder"
    # the guard: the pass that filled the cache saw everything ...
    assert uncached_children(od, ta, KEEP).tolist() == [[0] * 5] * 2
    assert od[0].uncached_children([{k: v[:1] for k, v in t.items() if k in ("keep_idx", "keep_count", "locs")} for t in ta], KEEP).tolist() == [0] * 5
    # ... a pass on visited() under other weights did not: the other model keeps patches the first did not, below level 0 too
    t_other, _ = _pass(other, res)
    differ = [l for l in range(4) if any(_kept_cells(tb, l, j) != _kept_cells(t_other, l, j) for j in range(2))]
    assert any(l >= 1 for l in differ), "the two models keep the same patches: pick another seed"
    from paths_amd import utils as putils
    t_vis = []
    with torch.no_grad():
        putils.recurse(other, vis, KEEP, 5, trace=t_vis)
    torch.cuda.synchronize()
    miss = uncached_children(od, t_vis, KEEP)
    assert tuple(miss.shape) == (2, 5) and int(miss[:, 0].sum()) == 0 and int(miss[:, 1:].sum()) > 0, miss.tolist()
    assert calls == [] and [s.count for s in od] == [[int(v.rows[l].shape[0]) for l in range(5)] for v in vis], "the guard leaves the caches alone"
