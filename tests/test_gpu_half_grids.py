"""fp16 feature grids on the GPU: the fp16 selection-chain kernels, the one-plane gate GEMMs and the fp16-row importance / projection
GEMM against (a) the same values stored as fp32 grids (bit-identical) and (b) the oracle on the fp16 synthetic pyramids."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_parity import LOGIT_TOL, STATE_TOL, build_model, dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16 = torch.float16
# fp16 slides screened with the oracle (LazyGrids of the fp16 spec, bench weights seed 0, top-K = K / 4): top-K boundary gap >= 1e-5 at
# every level.  fp16 rounding moves the gaps, so these differ from the fp32 bench ids.
IDS_2048 = [10001, 10007, 10008, 10014, 10017, 10020, 10023, 10024]
IDS_1024 = [10000, 10001]
BASE = {2048: (32, 64), 1024: (32, 32)}


def fp32_twin(s):
    from paths_amd.data_utils.slide import DeviceSlide
    return DeviceSlide([g.float() for g in s.grids], patch_size=s.patch_size, slide_id=s.slide_id + "-fp32")


def assert_same_recursion(ta, tb, oa, ob):
    """Per level: num_ims, locations, parents and kept indices identical; logits, importance, ctx_slide bit-identical."""
    assert len(ta) == len(tb)
    for l, (a, b) in enumerate(zip(ta, tb)):
        na, nb = a["num_ims"].cpu(), b["num_ims"].cpu()
        assert torch.equal(na, nb), f"level {l}: num_ims"
        for j in range(na.shape[0]):
            n = int(na[j])
            assert torch.equal(a["locs"][j, :n], b["locs"][j, :n]), f"level {l} slide {j}: locations"
            assert torch.equal(a["parent_inds"][j, :n], b["parent_inds"][j, :n]), f"level {l} slide {j}: (child -> parent) pairs"
            if "keep_idx" in a:
                c = int(a["keep_count"][j])
                assert c == int(b["keep_count"][j])
                assert torch.equal(a["keep_idx"][j, :c], b["keep_idx"][j, :c]), f"level {l} slide {j}: kept indices"
        for key in ("importance", "logits", "ctx_slide"):
            assert torch.equal(a[key], b[key]), f"level {l}: {key} differs (max {float((a[key] - b[key]).abs().max()):.3g})"
    for key in ("logits", "ctx_slide", "importance"):
        assert torch.equal(oa[key], ob[key]), key
    n_last = ta[-1]["num_ims"].cpu()
    for j in range(n_last.shape[0]):                 # (rows of padding are not written: whole tiles of them are skipped)
        assert torch.equal(oa["ctx_patch"][j, :int(n_last[j])], ob["ctx_patch"][j, :int(n_last[j])]), f"ctx_patch of slide {j}"


def test_fp16_synthetic_grids_match_the_host_replica(dev):
    from paths_amd.data_utils.slide import DeviceSlide
    for sid in (0, 5):
        s = DeviceSlide.synthetic(21, sid, (4, 6), dim=256, num_levels=3, device=dev, dtype=F16)
        t = fp32_twin(s)
        assert s.dtype == F16 and s.synthetic_spec.feature_dtype == "float16"
        for l in range(3):
            g = s.grids[l]
            assert g.dtype == F16
            np.testing.assert_array_equal(g.float().cpu().numpy(), s.synthetic_spec.grid(l))
            assert g.numel() * g.element_size() * 2 == t.grids[l].numel() * t.grids[l].element_size()
            assert torch.equal(s.masks[l], t.masks[l])
            assert torch.equal(s.masks[l].cpu().bool(), torch.from_numpy(~s.synthetic_spec.is_background(l, *np.meshgrid(
                np.arange(g.shape[0]), np.arange(g.shape[1]), indexing="ij"))))
        assert s.feature_absmax() == t.feature_absmax() and 1.7 < s.feature_absmax() < 1.74
        # upload through the host conversion helper: the same grid
        u = DeviceSlide.from_host([g.cpu() for g in t.grids], dev, dtype=F16)
        assert all(torch.equal(a, b) for a, b in zip(u.grids, s.grids)) and all(torch.equal(a, b) for a, b in zip(u.masks, s.masks))


@pytest.fixture(scope="module")
def k2048(dev):
    from paths_amd.data_utils.slide import DeviceSlide
    K = 2048
    cfg, model, params = build_model(dev, 0, None, top_k_patches=[K // 4] * 4)
    slides = [DeviceSlide.synthetic(1234, sid, BASE[K], device=dev, dtype=F16) for sid in IDS_2048]
    return cfg, model, params, slides


def test_fp16_recursion_is_bitwise_its_fp32_twin(dev, k2048):
    """8 slides at K = 2048 x 5 levels, top-K 512, stored fp16, against the same values stored fp32: the one-plane gate GEMMs drop only
    the lo*hi product, which is exactly zero for fp16 operands, and the fp16-row importance / projection GEMM stages the same fp32 sum."""
    from paths_amd import utils as putils
    cfg, model, _, slides = k2048
    twins = [fp32_twin(s) for s in slides]
    ta, tb = [], []
    with H.spy_calls() as calls, torch.no_grad():
        oa = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=ta)
        n16 = len(calls)
        ob = putils.recurse(model, twins, cfg.top_k_patches, 5, trace=tb)
    torch.cuda.synchronize()
    h16, h32 = set(calls[:n16]), set(calls[n16:])
    assert {"paths_lstm_cell_x6_h16", "paths_level0_batch_h16", "paths_gather_rows_h16"} <= h16, sorted(h16)
    assert {"paths_importance_qkv_x6_h16", "paths_importance_proj_x6_h16"} & h16, sorted(h16)
    assert "paths_lstm_cell_x6" not in h16 and not any(c.endswith("_h16") for c in h32)
    assert_same_recursion(ta, tb, oa, ob)


@pytest.mark.parametrize("K", [2048, 1024])
def test_fp16_recursion_vs_oracle(dev, k2048, K):
    """The headline recursion on fp16 slides against the oracle on LazyGrids of the fp16 spec, with the bars of
    test_headline_recursion_vs_oracle."""
    from oracle import paths_oracle as orc
    from oracle.compare import compare_recursion
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide
    if K == 2048:
        cfg, model, params, slides = k2048
        ids = IDS_2048
    else:
        ids = IDS_1024
        cfg, model, params = build_model(dev, 0, None, top_k_patches=[K // 4] * 4)
        slides = [DeviceSlide.synthetic(1234, sid, BASE[K], device=dev, dtype=F16) for sid in ids]
    ocfg = H.oracle_config(top_k_patches=[K // 4] * 4)
    trace, otrace = [], []
    with torch.no_grad():
        out = putils.recurse(model, slides, cfg.top_k_patches, 5, trace=trace)
        hz, _ = orc.inference_end2end(params, ocfg, [orc.LazyGrids(s.synthetic_spec) for s in slides], None, otrace)
    res = compare_recursion(trace, otrace, torch.sigmoid(out["logits"]), hz, imp_tol=STATE_TOL, hazard_tol=LOGIT_TOL)
    assert res["index_sets_identical"] and res["parent_pairs_identical"] and res["near_tie_slides"] == []
    assert res["min_boundary_gap"] >= 1e-5 and res["kept_indices_compared"] == len(ids) * 4 * (K // 4)
    np.testing.assert_allclose(out["logits"].cpu().numpy(), otrace[-1]["logits"].numpy(), atol=1e-4, rtol=0)


def test_fp16_tape_rebind_and_pipeline(dev):
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    K = 1024
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[K // 4] * 4)
    keep = cfg.top_k_patches
    mk = lambda ids: DeviceSlideBatch([DeviceSlide.synthetic(77, sid, BASE[K], device=dev, dtype=F16) for sid in ids])
    ba, bb = mk([0, 1]), mk([2, 3])
    assert ba.dtype == F16
    keys = ("logits", "ctx_slide", "importance")
    with torch.no_grad():
        ra, rb = putils.recurse(model, ba, keep, 5), putils.recurse(model, bb, keep, 5)
        tape = putils.TapedRecursion(model, ba, keep, 5)
        out = tape.replay()
        assert all(torch.equal(out[k], ra[k]) for k in keys)
        tape.rebind(bb)
        assert tape.tape is not None                      # bound, not dropped
        out = tape.replay()
        assert all(torch.equal(out[k], rb[k]) for k in keys)
        with pytest.raises(ValueError):
            tape.rebind(DeviceSlideBatch([fp32_twin(s) for s in ba.slides]))
        tape.close()
        pipe = putils.PipelinedRecursion(model, [ba, bb], keep, 5)
        pipe.submit(0)
        pipe.submit(1)
        o0 = {k: v.clone() for k, v in pipe.result(0).items()}
        o1 = pipe.result(1)
        assert all(torch.equal(o0[k], ra[k]) for k in keys) and all(torch.equal(o1[k], rb[k]) for k in keys)
        pipe.close()
    torch.cuda.synchronize()


def test_fp16_training_steps_are_bitwise_the_fp32_twin(dev):
    """Training gathers fp32 copies of the fp16 rows: three HipAdamW steps give the fp32 twin's losses, gradients and parameters."""
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    from paths_amd.optim import HipAdamW

    def run(dtype):
        cfg, model, _ = build_model(dev, 3, None, top_k_patches=[64] * 4)
        slides = [DeviceSlide.synthetic(14, sid, (16, 16), device=dev, dtype=F16) for sid in range(4)]
        labels = np.asarray([s.synthetic_spec.label(4) for s in slides], np.int64)
        if dtype == torch.float32:
            slides = [fp32_twin(s) for s in slides]
        batch = {"slide": DeviceSlideBatch(slides), "survival_bin": torch.from_numpy(labels[:, 0]), "censored": torch.from_numpy(labels[:, 1])}
        model.train()
        opt = HipAdamW(model.parameters(), lr=1e-4)
        losses, grads = [], []
        for _ in range(3):
            losses.append(float(putils.train_step(model, opt, batch, 5, cfg.top_k_patches)))
            grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        return losses, grads, {n: p.detach().clone() for n, p in model.named_parameters()}

    la, ga, pa = run(F16)
    lb, gb, pb = run(torch.float32)
    assert np.isfinite(la).all() and la == lb
    for a, b in zip(ga, gb):
        assert a.keys() == b.keys() and all(torch.equal(a[n], b[n]) for n in a)
    assert all(torch.equal(pa[n], pb[n]) for n in pa)


def test_fp16_out_of_range_slide_takes_the_fallback(dev):
    """Features near 30,000 leave the fp16-split range of the default mode ((max|x| + margin) * A_SCALE >= 65504): the recursion runs on
    the exact bf16 kernels over fp32 gathered copies of the fp16 rows - the fp32 twin's path exactly."""
    from paths_amd import ops
    from paths_amd import utils as putils
    from paths_amd.data_utils.slide import DeviceSlide, DeviceSlideBatch
    cfg, model, _ = build_model(dev, 0, None, top_k_patches=[64] * 4)
    small = [DeviceSlide.synthetic(5, sid, (16, 16), device=dev, dtype=F16) for sid in range(2)]
    big = [DeviceSlide([g * 16384 for g in s.grids]) for s in small]          # exact in fp16 (a power of two), max|x| ~ 28,400
    assert 28000 < big[0].feature_absmax() < 30000 and not ops.h3_in_range(big[0].feature_absmax())
    twins = [fp32_twin(s) for s in big]
    before = ops.RANGE_FALLBACKS[0]
    ta, tb = [], []
    with H.spy_calls() as calls, torch.no_grad():
        oa = putils.recurse(model, big, cfg.top_k_patches, 5, trace=ta)
        ob = putils.recurse(model, twins, cfg.top_k_patches, 5, trace=tb)
    torch.cuda.synchronize()
    assert ops.RANGE_FALLBACKS[0] >= before + 2                 # (both twins; a careful re-run counts again)
    assert "paths_gather_rows_h16" in calls and "paths_level0_batch_h16" in calls and "paths_lstm_cell_x6_h16" not in calls
    assert torch.isfinite(oa["logits"]).all()
    for a, b in zip(ta, tb):
        assert torch.equal(a["num_ims"], b["num_ims"]) and torch.equal(a["locs"], b["locs"])
    np.testing.assert_allclose(oa["logits"].cpu().numpy(), ob["logits"].cpu().numpy(), atol=LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(oa["importance"].cpu().numpy(), ob["importance"].cpu().numpy(), atol=STATE_TOL, rtol=0)
    with pytest.raises(ValueError):
        DeviceSlideBatch([small[0], twins[0]])
