"""On-demand slides on the GPU: the two selection kernels against their NumPy contract (every output, padding included), the row
predicate over a candidate buffer, and the recursion on OnDemandSlide.from_slide(s) against the resident slides themselves, bit for
bit; what is asked of the encoder, what is refused, the range contract, and that nothing else moved."""
import numpy as np
import pytest
import torch

from tests import on_demand_ref as R
from tests.helpers import spy_calls
from tests.test_gpu_half_grids import assert_same_recursion
from tests.test_gpu_parity import LOGIT_TOL, build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16 = torch.float16
FILL = -7                     # what the kernels leave untouched keeps this value


# ------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 8, 600)       # kept patches per slide in ONE launch (four counts need four slides): none, one thread's worth, fewer
                              # than four candidates per thread (all cached in registers) and, at 600, 2,400 candidates on 512
                              # threads = five per thread, past the four that candidate_kernel caches


def _kernel_inputs(patch_size, seed=0):
    rng = np.random.default_rng(seed)
    B, ldk, n_cur = len(COUNTS), max(COUNTS), 700
    cells = np.stack([rng.integers(0, 3, (B, n_cur)), rng.integers(0, 4, (B, n_cur))], axis=2).astype(np.int64)     # a 3 x 4 parent level
    locs = cells * patch_size
    keep_idx = rng.integers(0, n_cur, (B, ldk)).astype(np.int32)
    keep_count = np.asarray(COUNTS, np.int32)
    next_x, next_y = np.full((B,), 5, np.int32), np.full((B,), 7, np.int32)      # 5 x 7: 2x+1 = 5 and 2y+1 = 7 fall outside
    return B, ldk, n_cur, locs, keep_idx, keep_count, next_x, next_y


def _candidates(dev, patch_size):
    from paths_amd import _lib
    B, ldk, n_cur, locs, keep_idx, keep_count, nx, ny = _kernel_inputs(patch_size)
    t = lambda a: torch.from_numpy(a).to(dev)
    d = dict(keep_idx=t(keep_idx), keep_count=t(keep_count), locs=t(locs), nx=t(nx), ny=t(ny))
    cc = torch.full((B,), FILL, dtype=torch.int32, device=dev)
    cells = torch.full((B, 4 * ldk, 2), FILL, dtype=torch.int64, device=dev)
    slot = torch.full((B, 4 * ldk), FILL, dtype=torch.int32, device=dev)
    _lib.call("paths_candidate_children", d["keep_idx"].data_ptr(), ldk, d["keep_count"].data_ptr(), d["locs"].data_ptr(), n_cur, patch_size,
              d["nx"].data_ptr(), d["ny"].data_ptr(), B, cc.data_ptr(), cells.data_ptr(), slot.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    ref = R.candidate_children(keep_idx, keep_count, locs, patch_size, nx, ny, np.full((B,), FILL, np.int32),
                               np.full((B, 4 * ldk, 2), FILL, np.int64), np.full((B, 4 * ldk), FILL, np.int32))
    return d, (cc, cells, slot), ref, (B, ldk, keep_idx, keep_count)


@pytest.mark.parametrize("patch_size", [256, 1 << 30])
def test_candidate_kernel_equals_the_numpy_contract(dev, patch_size):
    """patch_size 2^30 puts the pixel coordinates of every cell with x = 2 at 2^31: the 64-bit division path."""
    _, got, ref, (B, ldk, _, keep_count) = _candidates(dev, patch_size)
    if patch_size == 1 << 30:
        assert _kernel_inputs(patch_size)[3].max() >= 1 << 31
    for g, r, name in zip(got, ref, ("cand_count", "cand_cells", "cand_slot")):
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg=name)
    cc = ref[0]
    assert cc[0] == 0 and 0 < cc[3] < 4 * 600, "some children of the 600 kept patches fall outside the 5 x 7 grid"
    assert (ref[1][0] == -1).all() and (ref[2][3, cc[3]:] == -1).all()


@pytest.mark.parametrize("patch_size", [256, 1 << 30])
@pytest.mark.parametrize("mask_kind", ["ones", "zeros", "alternating"])
@pytest.mark.parametrize("n_next", [2400, 5])
def test_admit_kernel_equals_the_numpy_contract(dev, patch_size, mask_kind, n_next):
    """n_next = 5 is smaller than what the slides with 8 and 600 kept patches admit under the ones / alternating masks: status bit 1,
    and those slides write num_out only."""
    from paths_amd import _lib
    d, (cc, cells, slot), ref, (B, ldk, keep_idx, keep_count) = _candidates(dev, patch_size)
    mask = {"ones": np.ones, "zeros": np.zeros}.get(mask_kind, lambda s, t: (np.arange(s[0] * s[1]).reshape(s) % 2).astype(t))((B, 4 * ldk), np.uint8)
    full = lambda shape, dt: torch.full(shape, FILL, dtype=dt, device=dev)
    out = dict(num_out=full((B,), torch.int64), locs_out=full((B, n_next, 2), torch.int64), parent_out=full((B, n_next), torch.int64),
               src_row=full((B, n_next), torch.int32), src_cell=full((B, n_next), torch.int32), hp_row=full((B, n_next), torch.int32),
               child_pos=full((B, 4 * ldk), torch.int32))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    dmask = torch.from_numpy(mask).to(dev)
    p = lambda k: out[k].data_ptr()
    _lib.call("paths_admit_children", cc.data_ptr(), cells.data_ptr(), slot.data_ptr(), dmask.data_ptr(), d["keep_idx"].data_ptr(), ldk,
              d["keep_count"].data_ptr(), patch_size, B, n_next, p("num_out"), p("locs_out"), p("parent_out"), p("src_row"), p("src_cell"),
              status.data_ptr(), p("child_pos"), p("hp_row"), _lib.stream())
    torch.cuda.synchronize()
    want = {k: np.full(tuple(v.shape), FILL, v.cpu().numpy().dtype) for k, v in out.items()}
    want_status = R.admit_children(*ref, mask, keep_idx, keep_count, patch_size, n_next, **want)
    for k in out:
        np.testing.assert_array_equal(out[k].cpu().numpy(), want[k], err_msg=k)
    assert int(status.item()) == want_status
    assert want_status & 1, "the slide without kept patches admits nothing"
    if n_next == 5 and mask_kind != "zeros":
        assert want_status & 2 and want["num_out"][3] > 5 and (want["locs_out"][3] == FILL).all() and (want["child_pos"][3] == FILL).all()
        assert (want["src_row"][1, :int(want["num_out"][1])] >= 0).all(), "a slide that fits is written as usual"
    else:
        assert not want_status & 2
    if mask_kind == "ones":
        assert want["num_out"].tolist() == ref[0].tolist()


def test_admit_without_the_optional_tables(dev):
    from paths_amd import _lib
    d, (cc, cells, slot), ref, (B, ldk, keep_idx, keep_count) = _candidates(dev, 256)
    n_next = 4 * ldk
    mask = np.ones((B, 4 * ldk), np.uint8)
    full = lambda shape, dt: torch.full(shape, FILL, dtype=dt, device=dev)
    out = dict(num_out=full((B,), torch.int64), locs_out=full((B, n_next, 2), torch.int64), parent_out=full((B, n_next), torch.int64),
               src_row=full((B, n_next), torch.int32), src_cell=full((B, n_next), torch.int32))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    dmask = torch.from_numpy(mask).to(dev)
    _lib.call("paths_admit_children", cc.data_ptr(), cells.data_ptr(), slot.data_ptr(), dmask.data_ptr(), d["keep_idx"].data_ptr(), ldk,
              d["keep_count"].data_ptr(), 256, B, n_next, *(t.data_ptr() for t in out.values()), status.data_ptr(), None, None, _lib.stream())
    torch.cuda.synchronize()
    want = {k: np.full(tuple(v.shape), FILL, v.cpu().numpy().dtype) for k, v in out.items()}
    assert R.admit_children(*ref, mask, keep_idx, keep_count, 256, n_next, **want) == int(status.item()) == 1
    for k in out:
        np.testing.assert_array_equal(out[k].cpu().numpy(), want[k], err_msg=k)


def test_selection_kernels_reject_bad_arguments(dev):
    from paths_amd import _lib
    z = torch.zeros((64,), dtype=torch.int64, device=dev)
    a, st = z.data_ptr(), _lib.stream()
    cand = lambda **kw: [kw.get("keep_idx", a), kw.get("ldk", 2), a, a, kw.get("n_cur", 4), kw.get("patch", 256), a, a, kw.get("B", 1), a, a,
                         kw.get("slot", a), st]
    for kw in (dict(B=0), dict(patch=0), dict(n_cur=0), dict(ldk=0), dict(ldk=1 << 29), dict(keep_idx=None), dict(slot=None)):
        assert kw.get("keep_idx", 1) is None or kw.get("slot", 1) is None or \
            R.check_candidate_args(kw.get("B", 1), kw.get("n_cur", 4), kw.get("patch", 256), kw.get("ldk", 2)) == -1
        with pytest.raises(_lib.PathsHipError, match=r"paths_candidate_children failed \(-1\)"):
            _lib.call("paths_candidate_children", *cand(**kw))
    adm = lambda **kw: [a, a, a, kw.get("mask", a), a, kw.get("ldk", 2), a, kw.get("patch", 256), kw.get("B", 1), kw.get("n_next", 8), a, a, a, a, a,
                        kw.get("status", a), None, None, st]
    for kw in (dict(B=0), dict(patch=0), dict(n_next=0), dict(ldk=0), dict(ldk=1 << 29), dict(mask=None), dict(status=None)):
        assert kw.get("mask", 1) is None or kw.get("status", 1) is None or \
            R.check_admit_args(kw.get("B", 1), kw.get("n_next", 8), kw.get("patch", 256), kw.get("ldk", 2)) == -1
        with pytest.raises(_lib.PathsHipError, match=r"paths_admit_children failed \(-1\)"):
            _lib.call("paths_admit_children", *adm(**kw))
    torch.cuda.synchronize()


def test_row_predicate_over_a_candidate_buffer(dev):
    """The mask pass over supplied rows: a non-zero row whose fp32 sum is exactly 0 and an all-zero row are both background."""
    from paths_amd import _lib
    for dtype, name in ((torch.float32, "paths_tissue_mask_absmax"), (F16, "paths_tissue_mask_absmax_h16")):
        buf = torch.zeros((2, 3, 64), dtype=dtype, device=dev)
        buf[0, 0, 0], buf[0, 0, 1] = 1.0, -1.0           # [1, -1, 0, ...]
        buf[0, 2, 5] = 0.25
        buf[1, 1] = 0.5
        buf[1, 2, 63] = -3.0
        mask = torch.full((2, 3), 9, dtype=torch.uint8, device=dev)
        bits = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.call(name, buf.data_ptr(), 6, 64, mask.data_ptr(), bits.data_ptr(), _lib.stream())
        assert mask.cpu().tolist() == [[0, 0, 1], [0, 1, 1]]
        assert _lib.float_from_bits(int(bits.item())) == 3.0


# ------------------------------------------------------------------------------------------------
# 2. the recursion on from_slide(s) is the recursion on s, bit for bit
# ------------------------------------------------------------------------------------------------
def _slides(dev, dtype=torch.float32, seed=41, ids=range(2), shape=(7, 6), **kw):
    from paths_amd.data_utils.slide import DeviceSlide, OnDemandSlide
    res = [DeviceSlide.synthetic(seed, sid, shape, device=dev, dtype=dtype, **kw) for sid in ids]
    return [OnDemandSlide.from_slide(s) for s in res], res


def _twin_runs(model, keep, od, res, levels=5, **kw):
    from paths_amd import utils as putils
    ta, tb = [], []
    with torch.no_grad():                    # the weight images are packed once per model and mode: keep those launches out of both lists
        putils.recurse(model, res, keep, levels, trace=[] if kw else None, **kw)
    with spy_calls() as calls, torch.no_grad():
        ob = putils.recurse(model, res, keep, levels, trace=tb, **kw)
        n = len(calls)
        oa = putils.recurse(model, od, keep, levels, trace=ta, **kw)
    torch.cuda.synchronize()
    assert int(ob["status"].item()) == 0, "the resident run itself must not need the careful path (pick another seed otherwise)"
    assert int(oa["status"].item()) == 0
    return ta, tb, oa, ob, calls[n:], calls[:n]


def _check_requests(od, tb, keep, patch=256):
    """Per level: what was asked is a duplicate-free subset of the in-bounds children of the twin's kept patches, at most 4 keep."""
    for j, s in enumerate(od):
        X, Y = s.shape(0)
        assert torch.equal(s.requested[0].cpu(), torch.cartesian_prod(torch.arange(X), torch.arange(Y))), "level 0: every cell, row-major"
        for l in range(1, len(tb)):
            c = int(tb[l - 1]["keep_count"][j])
            kept = tb[l - 1]["locs"][j][tb[l - 1]["keep_idx"][j, :c].long()].cpu().numpy() // patch
            X, Y = s.shape(l)
            allowed = {(2 * x + dx, 2 * y + dy) for x, y in kept.tolist() for dx in (0, 1) for dy in (0, 1) if 2 * x + dx < X and 2 * y + dy < Y}
            asked = [tuple(q) for q in s.requested[l].cpu().tolist()]
            assert len(set(asked)) == len(asked), f"slide {j} level {l}: a cell was asked twice"
            assert set(asked) <= allowed and len(asked) <= 4 * keep[l - 1], f"slide {j} level {l}"
            assert set(asked) == allowed, "every in-bounds child of a kept patch is a candidate"
            assert int(tb[l]["num_ims"][j]) <= len(asked)


@pytest.mark.parametrize("dtype", [torch.float32, F16])
def test_on_demand_recursion_is_bitwise_its_resident_twin(dev, dtype):
    """Two synthetic slides, base (7, 6), top-12, 5 levels, default mode: every trace field of every level and the outputs; the same
    with the attention and rollout exports; what the encoder was asked; the launches of each side."""
    from paths_amd.data_utils.slide import OnDemandSlideBatch, slide_batch
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[12] * 4)
    od, res = _slides(dev, dtype)
    seen = []
    for s in od:
        s.encode = (lambda enc, sid: lambda level, cells: (seen.append((sid, level, len(cells))), enc(level, cells))[1])(s.encode, s.slide_id)
    batch = slide_batch(od)
    assert isinstance(batch, OnDemandSlideBatch) and batch.n0 == 42 and batch.dim == res[0].dim and batch.dtype == dtype
    assert batch.max_dim == [7 << l for l in range(5)] and batch.gx[2].cpu().tolist() == [28, 28] and batch.gy[4].cpu().tolist() == [96, 96]
    ta, tb, oa, ob, ca, cb = _twin_runs(model, cfg.top_k_patches, batch, res)
    assert_same_recursion(ta, tb, oa, ob)
    assert sorted((sid, l) for sid, l, _ in seen) == sorted((s.slide_id, l) for s in od for l in range(5)), "encode sees each level once"
    _check_requests(od, tb, cfg.top_k_patches)
    sfx = "_h16" if dtype == F16 else ""
    assert ca.count("paths_candidate_children") == ca.count("paths_admit_children") == 4 and ca.count("paths_tissue_mask_absmax" + sfx) == 5
    assert "paths_expand_children" not in ca and cb.count("paths_expand_children") == 4
    assert {"paths_level0_batch" + sfx, "paths_gather_rows" + sfx} <= set(ca) & set(cb)
    assert not {"paths_candidate_children", "paths_admit_children"} & set(cb)
    others = lambda c: [n for n in c if n not in ("paths_candidate_children", "paths_admit_children", "paths_expand_children", "paths_tissue_mask_absmax" + sfx)]
    assert others(ca) == others(cb), "everything around the expansion is the resident launch sequence"
    ta, tb, oa, ob, _, _ = _twin_runs(model, cfg.top_k_patches, od, res, attention=True, rollout=True)
    assert_same_recursion(ta, tb, oa, ob)
    for l, (a, b) in enumerate(zip(ta, tb)):
        for key in ("attention", "attention_self", "rollout", "rollout_self"):
            assert torch.equal(a[key], b[key]), f"level {l}: {key}"
        assert float(a["rollout"].sum()) > 0
    _check_requests(od, tb, cfg.top_k_patches)


@pytest.mark.parametrize("variant", ["x6", "f32", "nolstm", "td192"])
def test_on_demand_recursion_other_branches_bitwise(dev, variant, monkeypatch):
    from paths_amd import ops
    over = {"nolstm": {"model_config": {"lstm": False}}, "td192": {"model_config": {"trans_dim": 192}}}.get(variant)
    if variant in ("x6", "f32"):
        monkeypatch.setattr(ops, "GEMM_MODE", variant)
    cfg, model, _ = build_model(dev, 5, over, top_k_patches=[12] * 4)
    od, res = _slides(dev)
    ta, tb, oa, ob, ca, cb = _twin_runs(model, cfg.top_k_patches, od, res)
    assert_same_recursion(ta, tb, oa, ob)
    assert ca.count("paths_admit_children") == 4 and "paths_expand_children" not in ca
    _check_requests(od, tb, cfg.top_k_patches)


def test_on_demand_inference_end2end(dev):
    from paths_amd import utils as putils
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[12] * 4)
    od, res = _slides(dev)
    labels = {"survival_bin": np.array([1, 2]), "censored": np.array([0, 1])}
    with torch.no_grad():
        ha, la = putils.inference_end2end(5, cfg.top_k_patches, model, None, dict(labels, slide=od), "survival")
        hb, lb = putils.inference_end2end(5, cfg.top_k_patches, model, None, dict(labels, slide=res), "survival")
    assert torch.equal(ha, hb) and torch.equal(la, lb)


# ------------------------------------------------------------------------------------------------
# 3. what is refused, the range contract, and that nothing else moved
# ------------------------------------------------------------------------------------------------
def test_no_tissue_among_the_children_is_refused(dev):
    """The slides of the careful-path test (seed 57, (4, 4), p_bg 0.93, top-2): the resident run falls back to every cell of the next
    grid; an on-demand slide would have to encode that whole grid, so the pass raises, naming the slide, and launches nothing more."""
    from paths_amd import _lib, utils as putils
    cfg, model, _ = build_model(dev, 9, None, top_k_patches=[2] * 4)
    od, res = _slides(dev, seed=57, ids=range(4), shape=(4, 4), p_bg=0.93)
    with torch.no_grad():
        fast = putils._recurse(model, res, cfg.top_k_patches, 5, None, careful=False)
        assert int(fast["status"].item()) & 1, "test slides should trigger the fallback (pick another seed otherwise)"
        with spy_calls() as calls, pytest.raises(_lib.PathsHipError, match=r"on-demand slide .*synthetic-57-.*every cell"):
            putils.recurse(model, od, cfg.top_k_patches, 5)
    assert calls[-1] == "paths_admit_children", "no launch follows the raise"
    torch.cuda.synchronize()
    with torch.no_grad():                                   # and the streams are usable afterwards
        out = putils.recurse(model, res, cfg.top_k_patches, 5)
    assert torch.isfinite(out["logits"]).all()


def test_out_of_range_rows_move_the_rest_of_the_pass_to_the_exact_kernels(dev):
    """Rows of the 5,000 scale arrive at level 2: (max|x| + margin) * A_SCALE leaves fp16, levels 2.. run on the three-plane kernels.
    The resident twin (the same values in its level-2 grid) runs every level there; the two agree within the parity bar."""
    from paths_amd import ops, utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, OnDemandSlide
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[12] * 4)
    _, small = _slides(dev)
    res = [DeviceSlide([g * 3000.0 if l == 2 else g for l, g in enumerate(s.grids)], slide_id=s.slide_id) for s in small]
    assert 5000 < res[0].feature_absmax() < 5200 and not ops.h3_in_range(res[0].feature_absmax())
    od = [OnDemandSlide.from_slide(s) for s in res]
    before = ops.RANGE_FALLBACKS[0]
    ta, tb = [], []
    with torch.no_grad():
        oa = putils.recurse(model, od, cfg.top_k_patches, 5, trace=ta)
        mid = ops.RANGE_FALLBACKS[0]
        ob = putils.recurse(model, res, cfg.top_k_patches, 5, trace=tb)
    torch.cuda.synchronize()
    assert mid == before + 1 and ops.GEMM_MODE == "h3", "one fallback, left again when the pass ends"
    assert int(oa["status"].item()) == 0 and int(ob["status"].item()) == 0
    assert torch.isfinite(oa["logits"]).all() and torch.isfinite(oa["ctx_slide"]).all() and torch.isfinite(oa["importance"]).all()
    diff = float((oa["logits"] - ob["logits"]).abs().max())
    print(f"on-demand (h3 levels 0-1, x6 levels 2-4) vs resident twin (x6 throughout): logits max|diff| = {diff:.3e}")
    for a, b in zip(ta, tb):
        assert torch.equal(a["num_ims"], b["num_ims"]) and torch.equal(a["locs"], b["locs"])
    np.testing.assert_allclose(oa["logits"].cpu().numpy(), ob["logits"].cpu().numpy(), atol=LOGIT_TOL, rtol=0)


def test_a_nan_row_raises(dev):
    from paths_amd import _lib, ops, utils as putils
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[12] * 4)
    od, _ = _slides(dev)
    enc = od[1].encode

    def bad(level, cells):
        rows = enc(level, cells)
        if level == 2:
            rows[0, 3] = float("nan")
        return rows

    od[1].encode = bad
    with torch.no_grad(), pytest.raises(_lib.PathsHipError, match="inf or NaN"):
        putils.recurse(model, od, cfg.top_k_patches, 5)
    torch.cuda.synchronize()
    assert ops.GEMM_MODE == "h3"


def test_bad_encode_results_raise_on_the_device_too(dev):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import OnDemandSlide
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[12] * 4)
    od, _ = _slides(dev)
    enc = od[0].encode
    for wrong in (lambda r: r[:-1], lambda r: r.half(), lambda r: r.cpu()):
        od[0].encode = lambda level, cells, w=wrong: w(enc(level, cells)) if level == 1 else enc(level, cells)
        with torch.no_grad(), pytest.raises(ValueError, match="encode"):
            putils.recurse(model, od, cfg.top_k_patches, 5)
    torch.cuda.synchronize()
    assert OnDemandSlide.on_demand


def test_nothing_else_moved(dev):
    """Resident and host-resident recursions launch neither new entry point; the stored-launch and training entry points refuse
    on-demand slides."""
    from paths_amd import saliency, utils as putils
    from paths_amd.data_utils.slide import HostSlide, slide_batch
    from paths_amd.optim import HipAdamW
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[12] * 4)
    keep = cfg.top_k_patches
    od, res = _slides(dev)
    host = [HostSlide.synthetic(41, sid, (7, 6), device=dev) for sid in range(2)]
    with spy_calls() as calls, torch.no_grad():
        putils.recurse(model, res, keep, 5)
        putils.recurse(model, host, keep, 5)
    torch.cuda.synchronize()
    assert calls.count("paths_expand_children") == 8 and not {"paths_candidate_children", "paths_admit_children"} & set(calls)
    for slides in (od, slide_batch(od)):
        for fn in (lambda: putils.TapedRecursion(model, slides, keep, 5), lambda: putils.GraphedRecursion(model, slides, keep, 5),
                   lambda: putils.PipelinedRecursion(model, [slides], keep, 5), lambda: putils.recurse_train(model, slides, keep, 5),
                   lambda: saliency.input_gradients(model, slides, keep, 5),
                   lambda: putils.train_step(model, HipAdamW(model.parameters(), lr=1e-4),
                                             {"slide": slides, "survival_bin": torch.tensor([1, 2]), "censored": torch.tensor([0, 1])}, 5, keep)):
            with pytest.raises(NotImplementedError, match="on-demand"):
                fn()
    tape = putils.TapedRecursion(model, res, keep, 5)
    with pytest.raises(NotImplementedError, match="on-demand"):
        tape.rebind(od)
    tape.close()
    del host
