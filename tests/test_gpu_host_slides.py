"""Host-resident slides on the GPU: the row-staging kernel against its NumPy restatement, the chunked mask pass against the resident
slides' masks, and the recursion / tape / training on pinned host grids against the resident twins of the same slides, bit for bit.
No test holds more than 4 GiB of pinned memory; each frees what it pinned."""
import gc

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import stage_ref
from tests.test_gpu_half_grids import BASE, assert_same_recursion
from tests.test_gpu_parity import build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16 = torch.float16
MiB = 1 << 20


def free_pinned():
    """Give the pinned blocks of dropped grids back (torch caches freed pinned memory like device memory)."""
    gc.collect()
    torch.cuda.synchronize()
    empty = getattr(torch._C, "_host_emptyCache", None)
    if empty is not None:
        empty()


def pinned_bytes(slides):
    return sum(s.host_bytes() for s in slides)


# ------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", [4096, 2048, 512, 6144])
def test_stage_rows_kernel_equals_the_numpy_contract(dev, row_bytes):
    """fp32 / fp16 rows of D = 1024, a narrow row, and a row longer than one 4-KiB piece: valid rows out of order (one source row
    twice), padding entries at both ends and in the middle, a row count that is not a multiple of the workgroup's rows."""
    from paths_amd import _lib
    rng = np.random.default_rng(row_bytes)
    n_src, rows = 1500, 1003
    src = torch.from_numpy(rng.integers(0, 256, size=(n_src, row_bytes), dtype=np.uint8)).pin_memory()
    assert src.is_pinned() and not src.is_cuda
    zero_row = torch.zeros((row_bytes,), dtype=torch.uint8, device=dev)
    pick = rng.permutation(n_src)[:rows].astype(np.int64)
    pick[5] = pick[2]
    pad = np.unique(np.concatenate([[0, 1, 500, rows - 1], rng.integers(0, rows, 120)]))
    valid = np.setdiff1d(np.arange(rows), pad)
    host_ptrs = src.data_ptr() + pick * row_bytes
    host_ptrs[pad] = zero_row.data_ptr()
    ptrs = torch.from_numpy(host_ptrs).to(dev)
    stage = torch.full((rows, row_bytes), 0xAB, dtype=torch.uint8, device=dev)
    _lib.call("paths_stage_rows", ptrs.data_ptr(), rows, row_bytes, stage.data_ptr(), zero_row.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    # the reference works on offsets into one flat memory; ZR is its stand-in for the zero row's address
    memory = np.concatenate([src.numpy().reshape(-1), np.zeros(row_bytes, np.uint8)])
    ZR = n_src * row_bytes
    ref_ptrs = pick * row_bytes
    ref_ptrs[pad] = ZR
    ref_stage, ref_out = stage_ref.stage_rows(memory, ref_ptrs, row_bytes, stage.data_ptr(), ZR)
    got_stage, got_out = stage.cpu().numpy(), ptrs.cpu().numpy()
    np.testing.assert_array_equal(got_stage[valid], ref_stage[valid])
    np.testing.assert_array_equal(got_stage[valid], src.numpy()[pick[valid]])
    np.testing.assert_array_equal(got_out[valid], ref_out[valid])
    np.testing.assert_array_equal(got_out[valid], stage.data_ptr() + valid * row_bytes)
    assert (got_out[pad] == zero_row.data_ptr()).all(), "padding entries keep the zero row's address"
    assert (got_stage[pad] == 0xAB).all(), "rows of padding entries are not written"
    del src
    free_pinned()


def test_stage_rows_rejects_bad_arguments(dev):
    from paths_amd import _lib
    z = torch.zeros((64,), dtype=torch.uint8, device=dev)
    ptrs = torch.full((4,), z.data_ptr(), dtype=torch.int64, device=dev)          # all padding: nothing would be followed anyway
    stage = torch.zeros((4, 64), dtype=torch.uint8, device=dev)
    st = _lib.stream()
    for args, word in (((ptrs.data_ptr(), 4, 4100, stage.data_ptr(), z.data_ptr(), st), "row_bytes"),
                       ((ptrs.data_ptr(), 4, 0, stage.data_ptr(), z.data_ptr(), st), "row_bytes"),
                       ((None, 4, 64, stage.data_ptr(), z.data_ptr(), st), "null"),
                       ((ptrs.data_ptr(), 4, 64, None, z.data_ptr(), st), "null"),
                       ((ptrs.data_ptr(), 4, 64, stage.data_ptr(), None, st), "null"),
                       ((ptrs.data_ptr(), 0, 64, stage.data_ptr(), z.data_ptr(), st), "rows")):
        assert stage_ref.check_args(*args[:5]) == -1
        with pytest.raises(_lib.PathsHipError, match=r"paths_stage_rows failed \(-1\).*" + word):
            _lib.call("paths_stage_rows", *args)
    _lib.call("paths_stage_rows", ptrs.data_ptr(), 4, 64, stage.data_ptr(), z.data_ptr(), st)      # the good call still works
    torch.cuda.synchronize()
    assert not stage.any()


# ------------------------------------------------------------------------------------------------
# 2. masks and max|x| through the bounce buffer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, F16])
@pytest.mark.parametrize("bounce_bytes", [64 << 20, 100_000])
def test_host_slide_masks_equal_the_resident_slides(dev, dtype, bounce_bytes):
    """100,000 bytes hold 97 fp32 (195 fp16) rows of D = 256: level 2 (1,920 cells) goes through many chunks and a last partial one."""
    from paths_amd.data_utils.slide import DeviceSlide, HostSlide, plan_mask_chunks
    spec = dict(dim=256, num_levels=3, p_bg=0.3, device=dev, dtype=dtype)
    h = HostSlide.synthetic(21, 4, (12, 10), bounce_bytes=bounce_bytes, **spec)
    d = DeviceSlide.synthetic(21, 4, (12, 10), **spec)
    if bounce_bytes == 100_000:
        plan = plan_mask_chunks(48 * 40, 256, h.grids[0].element_size(), bounce_bytes)
        assert len(plan) > 4 and plan[-1][1] < plan[0][1]
    assert h.dtype == d.dtype == dtype and h.num_levels == 3 and h.dim == 256 and h.synthetic_spec == d.synthetic_spec
    for l in range(3):
        assert not h.grids[l].is_cuda and h.grids[l].is_pinned() and h.grids[l].dtype == dtype
        assert h.masks[l].is_cuda and h.masks[l].dtype == torch.uint8 and h.shape(l) == d.shape(l)
        assert torch.equal(h.grids[l], d.grids[l].cpu()), f"level {l}: the host generator and the device generator differ"
        assert torch.equal(h.masks[l], d.masks[l]), f"level {l}: masks"
        assert 0 < int(h.masks[l].sum()) <= h.masks[l].numel()
    assert h.feature_absmax() == d.feature_absmax() and 1.7 < h.feature_absmax() < 1.74
    t = h.to_device()
    assert all(torch.equal(a, b) for a, b in zip(t.grids, d.grids)) and all(torch.equal(a, b) for a, b in zip(t.masks, d.masks))
    # cached masks / absmax skip the pass; from_host pins pageable grids (and converts through to_float16)
    c = HostSlide(h.grids, device=dev, masks=h.masks, absmax=h.feature_absmax())
    assert c.feature_absmax() == h.feature_absmax() and c.grids[0].data_ptr() == h.grids[0].data_ptr()
    u = HostSlide.from_host([g.float().numpy().copy() for g in h.grids], dev, dtype=dtype)
    assert all(g.is_pinned() for g in u.grids) and all(torch.equal(a, b) for a, b in zip(u.grids, h.grids))
    assert all(torch.equal(a, b) for a, b in zip(u.masks, d.masks)) and u.feature_absmax() == d.feature_absmax()
    del h, c, u
    free_pinned()


def test_pageable_grids_never_reach_the_pointer_table(dev):
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch, HostSlide
    h = HostSlide.synthetic(3, 0, (4, 4), dim=64, num_levels=2, device=dev)
    h.grids[1] = h.grids[1].clone()                       # somebody swaps in pageable memory behind the constructor's back
    assert not h.grids[1].is_pinned()
    with pytest.raises(AssertionError, match="pinned"):
        DeviceSlideBatch([h])
    with pytest.raises(ValueError):                       # device grids are not host grids
        HostSlide([g.to(dev) for g in h.grids], device=dev)
    with pytest.raises(ValueError, match="all resident"):
        ok = HostSlide.synthetic(3, 0, (4, 4), dim=64, num_levels=2, device=dev)
        DeviceSlideBatch([ok, DeviceSlide.synthetic(3, 0, (4, 4), dim=64, num_levels=2, device=dev)])
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 3. the recursion on pinned grids is its resident twin, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, F16])
def test_host_recursion_is_bitwise_its_resident_twin(dev, dtype):
    """Two slides at K = 1024 x 5 levels, top-K 256, default mode: every trace field of every level and the outputs; one staging
    launch per level on the host batch, none on the twin; the same with the attention and rollout exports."""
    from paths_amd.data_utils.slide import DeviceSlideBatch, HostSlide
    K = 1024
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[K // 4] * 4)
    host = [HostSlide.synthetic(1234, sid, BASE[K], device=dev, dtype=dtype) for sid in (10000, 10001)]
    assert pinned_bytes(host) <= 4 << 30 and all(not g.is_cuda and g.is_pinned() for s in host for g in s.grids)
    twins = [s.to_device() for s in host]
    hb, tb_ = DeviceSlideBatch(host), DeviceSlideBatch(twins)
    assert hb.host_resident and not tb_.host_resident and hb.dtype == dtype
    assert hb.grid_ptrs[4].cpu().tolist() == [s.grids[4].data_ptr() for s in host]
    ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, hb, tb_)
    assert ca.count("paths_stage_rows") == 5 and "paths_stage_rows" not in cb
    sfx = "_h16" if dtype == F16 else ""
    assert {"paths_level0_batch" + sfx, "paths_gather_rows" + sfx} <= set(ca) & set(cb)
    assert int(oa["status"].item()) == 0
    assert_same_recursion(ta, tb, oa, ob)
    ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, hb, tb_, attention=True, rollout=True)
    assert ca.count("paths_stage_rows") == 5 and "paths_stage_rows" not in cb
    assert_same_recursion(ta, tb, oa, ob)
    for l, (a, b) in enumerate(zip(ta, tb)):
        for key in ("attention", "attention_self", "rollout", "rollout_self"):
            assert torch.equal(a[key], b[key]), f"level {l}: {key}"
        assert float(a["rollout"].sum()) > 0
    del host, hb, ta, oa
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 4. the other branches: copying gathers, another aggregator width, the careful re-run
# ------------------------------------------------------------------------------------------------
def _small_pair(dev, seed, ids, shape, **kw):
    from paths_amd.data_utils.slide import HostSlide
    host = [HostSlide.synthetic(seed, sid, shape, device=dev, **kw) for sid in ids]
    return host, [s.to_device() for s in host]


@pytest.mark.parametrize("variant", ["x6", "f32", "nolstm", "td192"])
def test_host_recursion_other_branches_bitwise(dev, variant, monkeypatch):
    from paths_amd import ops
    over = {"nolstm": {"model_config": {"lstm": False}}, "td192": {"model_config": {"trans_dim": 192}}}.get(variant)
    if variant in ("x6", "f32"):
        monkeypatch.setattr(ops, "GEMM_MODE", variant)
    cfg, model, _ = build_model(dev, 5, over, top_k_patches=[12] * 4)
    host, twins = _small_pair(dev, 41, range(2), (7, 6))
    ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, host, twins)
    assert_same_recursion(ta, tb, oa, ob)
    mc = cfg.model_config
    if variant == "td192" and ops.generic_add_route(mc, mc.patch_embed_dim, mc.hierarchical_ctx_mlp_hidden_dim):
        assert ca.count("paths_stage_rows") == 5        # generic geometry, rows still read in place: staged
    if variant in ("x6", "f32", "nolstm"):
        # rows are copied by the gathers themselves (fp32 fts): the only kernels that read a host address; nothing is staged
        assert "paths_stage_rows" not in ca
    assert "paths_stage_rows" not in cb
    del host
    free_pinned()


def test_host_zero_children_fallback_bitwise(dev):
    """The careful re-run (paths_fallback_all_cells) on host slides: its rows go through the same staging."""
    from paths_amd import utils as putils
    cfg, model, _ = build_model(dev, 9, None, top_k_patches=[2] * 4)
    host, twins = _small_pair(dev, 57, range(4), (4, 4), p_bg=0.93)
    with torch.no_grad():
        fast = putils._recurse(model, host, cfg.top_k_patches, 5, None, careful=False)
    assert int(fast["status"].item()) & 1, "test slides should trigger the fallback (pick another seed otherwise)"
    ta, tb, oa, ob, ca, cb = H.twin_runs(model, cfg.top_k_patches, host, twins)
    assert "paths_fallback_all_cells" in ca and "paths_fallback_all_cells" in cb
    assert ca.count("paths_stage_rows") == 10 and "paths_stage_rows" not in cb           # optimistic pass + careful re-run
    assert_same_recursion(ta, tb, oa, ob)
    del host
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 5. launch tape: record, replay, rebind between host batches
# ------------------------------------------------------------------------------------------------
def test_host_tape_replay_rebind_and_pipeline(dev):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlideBatch, HostSlide
    cfg, model, _ = build_model(dev, 3, None, top_k_patches=[24] * 4)
    keep = cfg.top_k_patches
    mk = lambda seed, **kw: DeviceSlideBatch([HostSlide.synthetic(seed, sid, (9, 11), p_bg=0.15, device=dev, **kw) for sid in range(3)])
    ba, bb = mk(99), mk(7)
    keys = ("logits", "ctx_slide", "importance")

    def eager(batch):
        with torch.no_grad():
            o = putils.recurse(model, batch, keep, 5)
        return {k: o[k].clone() for k in keys}

    ra, rb = eager(ba), eager(bb)
    assert not torch.equal(ra["logits"], rb["logits"])
    with torch.no_grad():
        tape = putils.TapedRecursion(model, ba, keep, 5)
        out = tape.replay()
        assert sum(1 for _, _, name in tape.tape if name == "paths_stage_rows") == 5
        assert all(torch.equal(out[k], ra[k]) for k in keys)
        tape0 = tape.tape
        for batch, ref in ((bb, rb), (ba, ra), (bb, rb)):
            out = tape.rebind(batch).run()
            assert tape.tape is tape0, "bound, not recorded again"
            assert all(torch.equal(out[k], ref[k]) for k in keys)
        resident = DeviceSlideBatch([s.to_device() for s in ba.slides])
        with pytest.raises(ValueError, match="host-resident"):
            tape.rebind(resident)
        rt = putils.TapedRecursion(model, resident, keep, 5)
        out = rt.replay()
        assert all(torch.equal(out[k], ra[k]) for k in keys) and not any(name == "paths_stage_rows" for _, _, name in rt.tape)
        with pytest.raises(ValueError, match="host-resident"):
            rt.rebind(bb)
        with pytest.raises(ValueError):
            tape.rebind(mk(99, dtype=F16))
        rt.close()
        tape.close()
        with pytest.raises(NotImplementedError, match="host-resident"):
            putils.GraphedRecursion(model, ba, keep, 5)
        pipe = putils.PipelinedRecursion(model, [ba, bb], keep, 5)
        pipe.submit(0)
        pipe.submit(1)
        o0 = {k: v.clone() for k, v in pipe.result(0).items()}
        o1 = pipe.result(1)
        assert all(torch.equal(o0[k], ra[k]) for k in keys) and all(torch.equal(o1[k], rb[k]) for k in keys)
        pipe.close()
    torch.cuda.synchronize()
    del ba, bb, tape, pipe
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 6. training
# ------------------------------------------------------------------------------------------------
def test_host_training_steps_are_bitwise_the_resident_twin(dev):
    """Training gathers fp32 copies of the rows (over the host link, once): three HipAdamW steps give the twin's losses, gradients
    and parameters."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlideBatch, HostSlide
    from paths_amd.optim import HipAdamW
    host = [HostSlide.synthetic(14, sid, (16, 16), device=dev) for sid in range(3)]
    labels = np.asarray([s.synthetic_spec.label(4) for s in host], np.int64)

    def run(slides):
        cfg, model, _ = build_model(dev, 3, None, top_k_patches=[64] * 4)
        batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
        model.train()
        opt = HipAdamW(model.parameters(), lr=1e-4)
        losses, grads = [], []
        for _ in range(3):
            losses.append(float(putils.train_step(model, opt, batch, 5, cfg.top_k_patches)))
            grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        return losses, grads, {n: p.detach().clone() for n, p in model.named_parameters()}

    la, ga, pa = run(host)
    lb, gb, pb = run([s.to_device() for s in host])
    assert np.isfinite(la).all() and la == lb
    for a, b in zip(ga, gb):
        assert a.keys() == b.keys() and all(torch.equal(a[n], b[n]) for n in a)
    assert all(torch.equal(pa[n], pb[n]) for n in pa)
    del host
    free_pinned()


# ------------------------------------------------------------------------------------------------
# 7. footprint
# ------------------------------------------------------------------------------------------------
def test_host_slide_device_footprint_is_its_masks(dev):
    from paths_amd.data_utils.slide import HostSlide
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    bounce = torch.empty((64 << 20,), dtype=torch.uint8, device=dev)
    s = HostSlide.synthetic(1234, 10000, BASE[1024], device=dev, bounce=bounce)
    torch.cuda.synchronize()
    masks = sum(m.numel() for m in s.masks)
    assert masks == 1024 * (1 + 4 + 16 + 64 + 256)
    assert torch.cuda.memory_allocated(dev) - base <= masks + bounce.numel() + MiB
    del bounce
    assert torch.cuda.memory_allocated(dev) - base <= masks + MiB
    assert all(not g.is_cuda and g.is_pinned() for g in s.grids) and all(m.is_cuda for m in s.masks)
    assert s.host_bytes() == masks * 1024 * 4
    # a slide that allocates its own bounce buffer has released it when the constructor returns
    base = torch.cuda.memory_allocated(dev)
    t = HostSlide.synthetic(1234, 1, (8, 8), device=dev)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) - base <= sum(m.numel() for m in t.masks) + MiB
    del s, t
    free_pinned()
