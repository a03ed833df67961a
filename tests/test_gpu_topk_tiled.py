"""The tiled top-K (csrc/topk_tiled.hip: paths_topk_tiled / paths_topk_rows_tiled) on the GPU: against the NumPy contract of the
LDS-resident entries (tests/select_ref.py::topk) byte for byte, against those entries where both apply, twice for identical bytes,
refusals that write nothing, and the recursion - inference, training forward, launch tape - on a batch whose level 0 is the smallest
past the old limit of 8,192 patches per slide, against the oracle."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import select_ref as S
from tests.test_cpu_topk_tiled import A, TILED_MAX, refusals
from tests.test_gpu_parity import LOGIT_TOL, STATE_TOL, build_model, dev  # noqa: F401  (fixture)
from tests.test_gpu_select import FILL, _like, _same, _topk_scores

pytestmark = pytest.mark.gpu

TILE = 2048                                        # csrc/topk_tiled.hip TT_TILE; 64 elements per workgroup, a quarter of a tile per wave
# 1: a tile of 4 key pairs, one per wave (the one-pair loop only); 65: two workgroups, 9 pairs per wave (two four-pair steps and one
# pair); 2050: one whole tile and a ragged second of 2 keys; 8193: the first size the LDS-resident entries refuse, four whole tiles
# and one key; 20001: ten tiles, the last ragged, 313 workgroups per slide
TILED_N = (1, 65, 2050, 8193, 20001)
KEEPS = {"one": lambda n: 1, "64": lambda n: 64, "n_max": lambda n: n, "n_max+5": lambda n: n + 5, "all": lambda n: -1,
         "8200": lambda n: 8200,               # 8200 (at 20001 only): a kept-row table longer than the old cap
         "512": lambda n: 512}                 # (the comparison of the two families)
CASES = [(n, k) for n in TILED_N for k in ("one", "64", "n_max", "n_max+5", "all")] + [(20001, "8200")]


def _case(dev, n_max, keep_kind):
    """The inputs of tests/test_gpu_select.py::test_topk_equals_the_numpy_contract at another size: B = 5 slides of n_max, n_max - 1,
    n_max // 2, 1 and 0 patches in rows of stride n_max + 3, the four kinds of score rows, +NaN and 3e38 at and beyond num_ims[b]."""
    keep = KEEPS[keep_kind](n_max)
    rng = np.random.default_rng(1000 * n_max + list(KEEPS).index(keep_kind))
    B, ld = 5, n_max + 3
    num_ims = [n_max, n_max - 1, n_max // 2, min(1, n_max), 0]
    ldk = max(n_max if keep < 0 else min(keep, n_max), 70)
    sc = _topk_scores(rng, ld, num_ims, keep, list(KEEPS).index(keep_kind))
    slide_rows, row_ld = n_max + 2, 12
    c = dict(B=B, ld=ld, n_max=n_max, keep=keep, ldk=ldk, num_ims=num_ims, sc=sc, slide_rows=slide_rows, row_ld=row_ld)
    c["table"] = torch.zeros((B, slide_rows, row_ld), device=dev)
    c["zero_row"] = torch.zeros((row_ld,), device=dev)
    c["d_sc"], c["d_num"] = torch.from_numpy(sc).to(dev), torch.tensor(num_ims, dtype=torch.int64, device=dev)
    return c


def _fresh(dev, c, rows):
    out = dict(keep_idx=np.full((c["B"], c["ldk"]), FILL, np.int32), keep_count=np.full((c["B"],), FILL, np.int32))
    if rows:
        out["kept_rows"] = np.full((c["B"], c["ldk"]), FILL, np.int64)
    return _like(dev, out)


def _launch(name, c, got):
    """One launch of a top-K entry point (either family: the parameter lists are the same) into the buffers ``got``."""
    from paths_amd import _lib
    head = [c["d_sc"].data_ptr(), c["ld"], c["d_num"].data_ptr(), c["B"], c["n_max"], c["keep"], got["keep_idx"].data_ptr(), c["ldk"],
            got["keep_count"].data_ptr()]
    if "kept_rows" in got:
        head += [c["table"].data_ptr(), c["row_ld"], c["slide_rows"], got["kept_rows"].data_ptr(), c["zero_row"].data_ptr()]
    _lib.call(name, *head, _lib.stream())
    torch.cuda.synchronize()


def _want(c, rows):
    want = dict(keep_idx=np.full((c["B"], c["ldk"]), FILL, np.int32), keep_count=np.full((c["B"],), FILL, np.int32))
    if rows:
        want["kept_rows"] = np.full((c["B"], c["ldk"]), FILL, np.int64)
        S.topk(c["sc"], c["ld"], c["num_ims"], c["keep"], want["keep_idx"], want["keep_count"], want["kept_rows"], c["table"].data_ptr(),
               c["row_ld"], c["slide_rows"], c["zero_row"].data_ptr())
    else:
        S.topk(c["sc"], c["ld"], c["num_ims"], c["keep"], **want)
    return want


@pytest.mark.parametrize("n_max,keep_kind", CASES)
def test_tiled_topk_equals_the_numpy_contract(dev, n_max, keep_kind):
    """Every byte of keep_idx, keep_count and kept_rows, from sentinel-filled buffers, for both entries; ldk = max(needed, 70).
    keep = -1 at n_max = 8193 (through both entries) is the reference's ``top_k_patches = -1`` on a level past the old cap: every
    patch in original order, nothing ranked."""
    c = _case(dev, n_max, keep_kind)
    assert max(c["num_ims"]) <= n_max <= TILED_MAX and c["ldk"] <= TILED_MAX
    for rows, name in ((False, "paths_topk_tiled"), (True, "paths_topk_rows_tiled")):
        want = _want(c, rows)
        got = _fresh(dev, c, rows)
        _launch(name, c, got)
        _same(got, want)
        for b, n in enumerate(c["num_ims"]):
            cnt = n if c["keep"] < 0 else min(n, c["keep"])
            assert want["keep_count"][b] == cnt and (want["keep_idx"][b, cnt:] == FILL).all()
        if rows:
            assert (want["kept_rows"][4] == c["zero_row"].data_ptr()).all() and (want["kept_rows"] != FILL).all()
    if keep_kind == "8200":
        assert c["ldk"] == 8200 > S.TOPK_MAX


@pytest.mark.parametrize("keep_kind", ["512", "all"])
@pytest.mark.parametrize("n_max", [2050, 8192])
def test_tiled_topk_equals_the_lds_resident_entries(dev, n_max, keep_kind):
    """Where both families apply each _tiled output is the output of paths_topk / paths_topk_rows on the same buffers."""
    c = _case(dev, n_max, keep_kind)
    assert S.check_topk_args(c["B"], n_max, c["keep"], c["ldk"]) == 0
    for rows, name in ((False, "paths_topk"), (True, "paths_topk_rows")):
        old, new = _fresh(dev, c, rows), _fresh(dev, c, rows)
        _launch(name, c, old)
        _launch(name + "_tiled", c, new)
        for k in old:
            assert torch.equal(old[k], new[k]), (name, k)
        assert int(old["keep_count"][0]) == (n_max if c["keep"] < 0 else 512)


def test_tiled_topk_is_bit_identical_on_a_rerun(dev):
    c = _case(dev, 20001, "8200")
    for rows, name in ((False, "paths_topk_tiled"), (True, "paths_topk_rows_tiled")):
        first, second = _fresh(dev, c, rows), _fresh(dev, c, rows)
        _launch(name, c, first)
        _launch(name, c, second)
        for k in first:
            assert torch.equal(first[k], second[k]), (name, k)
        assert first["keep_count"].tolist() == [8200, 8200, 8200, 1, 0]


def test_refusals_launch_nothing(dev):
    """The refusals of tests/test_cpu_topk_tiled.py with device pointers (buffers as large as the cap, whatever the refused sizes
    are): rc = -1 and every output keeps its fill."""
    from paths_amd import _lib
    lib = _lib.load()
    n = TILED_MAX + 1
    sc = torch.zeros((1, n), device=dev)
    num = torch.full((1,), 100, dtype=torch.int64, device=dev)
    table, zero_row = torch.zeros((n, 12), device=dev), torch.zeros((12,), device=dev)
    out = dict(keep_idx=torch.full((1, n), FILL, dtype=torch.int32, device=dev), keep_count=torch.full((1,), FILL, dtype=torch.int32, device=dev),
               kept_rows=torch.full((1, n), FILL, dtype=torch.int64, device=dev))
    at = {0: sc, 2: num, 6: out["keep_idx"], 8: out["keep_count"], 9: table, 12: out["kept_rows"], 13: zero_row}
    count = 0
    for name, args, word in refusals():
        real = [at[i].data_ptr() if (v == A and i in at) else v for i, v in enumerate(args)]
        real[-1] = _lib.stream()
        assert getattr(lib, name)(*real) == -1 and word in lib.paths_last_error(), (name, args)
        count += 1
    torch.cuda.synchronize()
    assert count >= 25
    for k, t in out.items():
        assert bool((t == FILL).all()), k


# ------------------------------------------------------------------------------------------------
# the recursion at the smallest size past the old cap
# ------------------------------------------------------------------------------------------------
BASES = ((91, 91), (90, 92), (40, 50))             # 8,281, 8,280 and 2,000 level-0 patches: one slide under the old cap in a batch over it
KEEP = [24, 12]
# Chosen on the CPU from the oracle's scores alone: with these seeds the smallest gap between the last kept and the first dropped
# importance over the three slides and two selecting levels is 1.94e-4 (seeds (5, 21): 7.3e-5, (3, 14): 4.1e-5, (11, 31): 1.97e-4)
WSEED, DSEED = 77, 640
MIN_GAP = 5e-5                                     # ten times STATE_TOL: a screened near-tie cannot hide a wrong selection


@pytest.fixture(scope="module")
def past_cap(dev):
    """Model, slides and the oracle's pass (computed once, shared, left unchanged)."""
    from oracle import paths_oracle as orc
    from paths_amd.data_utils.slide import DeviceSlide
    over = {"num_levels": 3}
    cfg, model, params = build_model(dev, WSEED, over, top_k_patches=KEEP)
    ocfg = H.oracle_config(over, top_k_patches=KEEP)
    slides = [DeviceSlide.synthetic(DSEED, sid, base, num_levels=3, p_bg=0.0, device=dev) for sid, base in enumerate(BASES)]
    otrace = []
    with torch.no_grad():
        hz, _ = orc.inference_end2end(params, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], None, otrace)
    assert [int(n) for n in otrace[0]["num_ims"]] == [8281, 8280, 2000]
    return dict(model=model, slides=slides, otrace=otrace, hz=hz)


def _check_against_oracle(trace, logits, st):
    from oracle.compare import compare_recursion
    res = compare_recursion(trace, st["otrace"], torch.sigmoid(logits), st["hz"], imp_tol=STATE_TOL, hazard_tol=LOGIT_TOL,
                            raise_on_mismatch=False)
    print({k: res[k] for k in ("max_importance_diff", "max_hazard_diff", "min_boundary_gap", "kept_indices_compared", "near_tie_slides")})
    assert res["problems"] == [], res["problems"]
    assert res["near_tie_slides"] == []
    assert res["kept_indices_compared"] == 3 * (24 + 12)
    assert res["min_boundary_gap"] >= MIN_GAP
    return res


def test_recursion_past_the_old_cap_matches_the_oracle(dev, past_cap):
    """Three slides of 8,281 / 8,280 / 2,000 level-0 patches, three levels, top_k_patches [24, 12], the shipped model: the parent
    commit raises PathsHipError here (paths_topk[_rows] refuses n_max = 8281).  Level 0 selects through the tiled entry, level 1 (96
    patches) through the LDS-resident one."""
    from paths_amd import utils as putils
    st = past_cap
    trace = []
    with H.spy_calls() as calls, torch.no_grad():
        out = putils.recurse(st["model"], st["slides"], KEEP, 3, trace=trace)
    torch.cuda.synchronize()
    assert int(out["status"].item()) == 0
    topk = [c for c in calls if c.startswith("paths_topk")]
    assert topk in (["paths_topk_rows_tiled", "paths_topk_rows"], ["paths_topk_tiled", "paths_topk"]), topk
    _check_against_oracle(trace, out["logits"], st)
    st["eager"] = dict(logits=out["logits"].clone(), keep=[(r["keep_idx"].clone(), r["keep_count"].clone()) for r in trace[:-1]])


def test_training_forward_past_the_old_cap_matches_the_oracle(dev, past_cap):
    """The same batch through recurse_train (dropout 0): its top-K call site takes paths_topk_tiled at level 0.  No backward pass:
    the backward kernels take keep_idx as data and are untouched."""
    from paths_amd import utils as putils
    st = past_cap
    model = st["model"]
    trace = []
    model.train()
    try:
        with H.spy_calls() as calls, torch.no_grad():
            out = putils.recurse_train(model, st["slides"], KEEP, 3, trace=trace)
        torch.cuda.synchronize()
    finally:
        model.eval()
    assert int(out["status"].item()) == 0
    assert [c for c in calls if c.startswith("paths_topk")] == ["paths_topk_tiled", "paths_topk"]
    _check_against_oracle(trace, out["logits"], st)


def test_launch_tape_past_the_old_cap_replays_the_eager_pass(dev, past_cap, monkeypatch):
    """TapedRecursion on the same batch: the tape records what _lib.call launches, the tiled entry included, and a replay writes the
    eager pass's logits and per-level selections bit for bit.  (The selections are read from the recorded pass's own buffers, which
    the tape addresses: they are filled with a sentinel before the replay that is compared.)"""
    from paths_amd import utils as putils
    st = past_cap
    if "eager" not in st:
        trace = []
        with torch.no_grad():
            out = putils.recurse(st["model"], st["slides"], KEEP, 3, trace=trace)
        st["eager"] = dict(logits=out["logits"].clone(), keep=[(r["keep_idx"].clone(), r["keep_count"].clone()) for r in trace[:-1]])
    kept = []
    real = putils._expand_children

    def noting(batch, level, patch_size, keep_idx, keep_count, *a, **kw):
        kept.append((keep_idx, keep_count))
        return real(batch, level, patch_size, keep_idx, keep_count, *a, **kw)

    monkeypatch.setattr(putils, "_expand_children", noting)
    with torch.no_grad():
        tape = putils.TapedRecursion(st["model"], st["slides"], KEEP, 3)
        tape.replay()                                   # (records: a warm-up pass, then the recorded one)
        monkeypatch.setattr(putils, "_expand_children", real)
        names = [name for _, _, name in tape.tape if name.startswith("paths_topk")]
        assert names in (["paths_topk_rows_tiled", "paths_topk_rows"], ["paths_topk_tiled", "paths_topk"]), names
        recorded = kept[-2:]                            # the recorded pass's two selections
        for ki, kc in recorded:
            ki.fill_(FILL)
            kc.fill_(FILL)
        out = tape.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["logits"], st["eager"]["logits"])
        for l, ((ki, kc), (eki, ekc)) in enumerate(zip(recorded, st["eager"]["keep"])):
            assert torch.equal(kc, ekc) and kc.tolist() == [KEEP[l]] * 3, l
            assert torch.equal(ki[:, :KEEP[l]], eki[:, :KEEP[l]]), l
        tape.close()
