"""CPU tests of the train/eval harness pieces that need no GPU: metrics, checkpoint format, shuffle semantics."""
import itertools
import os
import pickle

import numpy as np
import pytest
import torch


def brute_cindex(event, time, risk):
    num = conc = 0.0
    n = len(time)
    for i, j in itertools.permutations(range(n), 2):
        if not event[i]:
            continue
        if time[i] < time[j] or (time[i] == time[j] and not event[j]):
            num += 1
            if abs(risk[i] - risk[j]) <= 1e-8:
                conc += 0.5
            elif risk[i] > risk[j]:
                conc += 1
    return conc / num


def test_concordance_index_matches_definition():
    from paths_amd.eval import concordance_index_censored
    rng = np.random.RandomState(0)
    for n in (5, 17, 60):
        event = rng.rand(n) < 0.6
        event[0] = True
        time = rng.randint(0, 8, n).astype(float)          # many tied times
        risk = np.round(rng.randn(n), 1)                   # some tied risks
        assert abs(concordance_index_censored(event, time, risk) - brute_cindex(event, time, risk)) < 1e-12
    # known answers: perfectly ordered / reversed
    e, t = np.ones(4, bool), np.array([1.0, 2, 3, 4])
    assert concordance_index_censored(e, t, np.array([4.0, 3, 2, 1])) == 1.0
    assert concordance_index_censored(e, t, np.array([1.0, 2, 3, 4])) == 0.0
    assert concordance_index_censored(e, t, np.zeros(4)) == 0.5


def test_concordance_index_hand_computed_sksurv_cases():
    """Known answers worked out by hand from the definition sksurv.metrics.concordance_index_censored documents (pair (i, j) is
    comparable iff i had an event and t_i < t_j, or t_i == t_j and j is censored; a pair counts 1 if risk_i > risk_j, 1/2 if the
    risks are within tied_tol; sksurv itself is not installed here)."""
    from paths_amd.eval import concordance_index_censored as ci
    # events at t = 1, 2, 4; censored at t = 2, 3.  Comparable: 0 -> {1, 2, 3, 4} (4 concordant); 1 -> {3 (conc), 4 (disc), 2 (same
    # time, censored: risk tie -> 1/2)}; the last event has nobody after it.  (4 + 1 + 0.5) / 7
    t = np.array([1.0, 2, 2, 3, 4]); e = np.array([1, 1, 0, 0, 1], bool); r = np.array([0.9, 0.5, 0.5, 0.1, 0.7])
    assert abs(ci(e, t, r) - 5.5 / 7.0) < 1e-15
    # tied times: two events at the same time are NOT comparable with each other; an event and a censored sample at that time are
    assert ci(np.array([1, 0], bool), np.array([5.0, 5.0]), np.array([0.2, 0.8])) == 0.0
    assert ci(np.array([1, 0], bool), np.array([5.0, 5.0]), np.array([0.8, 0.2])) == 1.0
    assert abs(ci(np.array([1, 1, 0], bool), np.array([5.0, 5.0, 7.0]), np.array([0.3, 0.9, 0.5])) - 0.5) < 1e-15      # pairs 0->2 (disc), 1->2 (conc)
    # a censored sample never opens a pair, even when it is the earliest
    assert ci(np.array([0, 1, 1], bool), np.array([1.0, 2.0, 3.0]), np.array([0.0, 0.9, 0.1])) == 1.0                  # only 1 -> 2
    # risk ties inside tied_tol count one half, outside it they are ordered
    e3, t3 = np.array([1, 1], bool), np.array([1.0, 2.0])
    assert ci(e3, t3, np.array([0.5, 0.5 + 5e-9])) == 0.5 and ci(e3, t3, np.array([0.5, 0.5 + 5e-8])) == 0.0
    assert ci(e3, t3, np.array([0.5, 0.5 + 5e-8]), tied_tol=1e-7) == 0.5
    # no comparable pair at all: all censored, or every event tied in time with only events
    for ev, tt in ((np.zeros(3, bool), np.array([1.0, 2, 3])), (np.ones(3, bool), np.array([5.0, 5, 5]))):
        with pytest.raises(ValueError):
            ci(ev, tt, np.array([0.1, 0.2, 0.3]))


def test_binary_auroc_matches_pair_counting():
    from paths_amd.eval import binary_auroc
    rng = np.random.RandomState(1)
    for n in (6, 40):
        s = np.round(rng.rand(n), 1)
        y = rng.rand(n) < 0.4
        y[0], y[1] = True, False
        pos, neg = s[y], s[~y]
        ref = ((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg))
        assert abs(binary_auroc(s, y) - ref) < 1e-12
    assert binary_auroc(np.array([0.1, 0.2]), np.array([1, 1])) == 0.5


def test_survival_evaluator_and_train_stats():
    from paths_amd.eval import SurvivalEvaluator
    ev = SurvivalEvaluator("val")
    hz = torch.tensor([[0.9, 0.5, 0.5, 0.5], [0.1, 0.1, 0.1, 0.1], [0.5, 0.5, 0.5, 0.5]])
    batch = {"censored": torch.tensor([0, 0, 1]), "survival": torch.tensor([1.0, 9.0, 5.0])}
    ev.register(batch, hz, torch.tensor(0.7))
    stats = {"val_loss": {}, "val_c-index": {}}
    out = ev.calculate(stats, 3)
    assert out["val_c-index"] == 1.0 and abs(out["val_loss"] - 0.7) < 1e-6      # high hazard <-> short survival
    assert stats["val_c-index"][3] == 1.0


def test_checkpoint_format_roundtrip(tmp_path):
    """model.pt = state_dict, train_stats.pkl = pickled dict with 'epoch' (reference utils.py:169-198)."""
    from paths_amd.config import Config
    from paths_amd.train import load_state, save_state
    cfg = Config.load(os.path.join(os.path.dirname(__file__), "golden", "sample"), test_mode=True)
    torch.manual_seed(1)
    m1 = cfg.get_model()
    save_state(str(tmp_path), m1, {"epoch": 7, "train_loss": {1: 0.5}})
    assert sorted(os.listdir(tmp_path)) == ["model.pt", "train_stats.pkl"]
    assert pickle.load(open(tmp_path / "train_stats.pkl", "rb"))["epoch"] == 7
    torch.manual_seed(2)
    m2 = cfg.get_model()
    stats = load_state(str(tmp_path), m2, map_location="cpu")
    assert stats["epoch"] == 7 and all(torch.equal(a, b) for a, b in zip(m1.state_dict().values(), m2.state_dict().values()))
    assert load_state(str(tmp_path / "nope"), m2) == {"epoch": 1}


def test_epoch_permutation_equals_dataloader_shuffle():
    from paths_amd.train import epoch_permutation
    data = list(range(23))
    torch.manual_seed(123)
    ref = [int(x) for x in torch.utils.data.DataLoader(data, batch_size=1, shuffle=True)]
    ref2 = [int(x) for x in torch.utils.data.DataLoader(data, batch_size=1, shuffle=True)]
    torch.manual_seed(123)
    assert epoch_permutation(23, True) == ref and epoch_permutation(23, True) == ref2
    assert epoch_permutation(5, False) == [0, 1, 2, 3, 4]
    # a non-shuffling loader consumes one draw of the global generator per pass too (its iterator's base seed): the order of the
    # NEXT shuffled epoch depends on it
    torch.manual_seed(5)
    a = [int(x) for x in torch.utils.data.DataLoader(data, batch_size=1, shuffle=True)]
    _ = [x for x in torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)]
    b = [int(x) for x in torch.utils.data.DataLoader(data, batch_size=1, shuffle=True)]
    torch.manual_seed(5)
    assert epoch_permutation(23, True) == a and epoch_permutation(23, False) == data and epoch_permutation(23, True) == b


def test_importance_map_weighting():
    """Two levels: a 2x1 level-0 grid, the second patch expanded into two children."""
    from paths_amd.heatmap import importance_map
    levels = [{"locs": np.array([[0, 0], [256, 0]]), "importance": np.array([0.2, 0.8])},
              {"locs": np.array([[512, 0], [768, 256]]), "importance": np.array([0.5, 0.1])}]
    m = importance_map(levels, (2, 1))
    assert m.shape == (4, 2)
    np.testing.assert_allclose(m[0:2], 0.2 + 1e-4)                                   # never expanded
    np.testing.assert_allclose(m[2, 0], 0.8 + 1e-4 + 0.5 * (0.5 + 1e-4))
    np.testing.assert_allclose(m[3, 1], 0.8 + 1e-4 + 0.5 * (0.1 + 1e-4))
    np.testing.assert_allclose(m[2, 1], 0.8 + 1e-4)                                  # child filtered out (background)


def test_lagged_scale_registry_resets():
    """The training forward's lagged fp16 weight scales are dropped when weights are replaced wholesale."""
    from paths_amd import ops
    a, b = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    ops._lagged_store(a)["w"] = [2.0, None, None]
    assert "w" in ops._lagged_store(a) and "w" not in ops._lagged_store(b)      # kept on the module, not keyed by id()
    ops.reset_lagged_scales()
    assert "w" not in ops._lagged_store(a)


def test_bench_dump_outputs_sample_and_budget(tmp_path):
    """bench.py --dump-outputs: the recursion's outputs whole, ctx_patch as the same seeded row sample in every run with its padding
    rows zeroed, every file float32 / float64, the whole under 64 MB; an array larger than what is left is a seeded element sample."""
    import bench
    B, N, Dp = 8, 2048, 1280                                  # the headline's last level: ctx_patch alone is 84 MB
    g = torch.Generator().manual_seed(1)
    num_ims = torch.tensor([2048, 1900, 1500, 2000, 7, 1024, 2047, 1])
    valid = torch.arange(N)[None, :] < num_ims[:, None]
    out = {"logits": torch.randn(B, 4, generator=g), "ctx_slide": torch.randn(B, 128, generator=g),
           "importance": torch.rand(B, N, generator=g).clamp_min(1e-3) * valid, "ctx_patch": torch.randn(B, N, Dp, generator=g),
           "status": torch.zeros((), dtype=torch.int32)}
    res = bench.recursion_outputs(out)
    assert sum(a.nbytes for a in res.values()) <= bench.DUMP_BYTES
    np.testing.assert_array_equal(res["logits"], out["logits"].numpy())
    np.testing.assert_array_equal(res["importance"], out["importance"].numpy())
    rows = res["ctx_patch_sample_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0)
    want = out["ctx_patch"][:, rows] * valid[:, rows, None]
    np.testing.assert_array_equal(res["ctx_patch_sample"], want.numpy())
    np.testing.assert_array_equal(bench.recursion_outputs(out)["ctx_patch_sample_rows"], res["ctx_patch_sample_rows"])
    # a budget that leaves room for fewer rows: fewer rows, still under it
    small = bench.recursion_outputs(out, budget=4 << 20)
    assert sum(a.nbytes for a in small.values()) <= 4 << 20 and 0 < len(small["ctx_patch_sample_rows"]) < bench.DUMP_ROWS
    bench.write_outputs(str(tmp_path / "d"), dict(res, big=np.arange(10 << 20, dtype=np.float64)))
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == sorted([k + ".npy" for k in res] + ["big_sample.npy"])
    assert sum(os.path.getsize(tmp_path / "d" / f) for f in files) <= 64 << 20
    for f in files:
        assert np.load(tmp_path / "d" / f).dtype in (np.float32, np.float64)
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "ctx_patch_sample.npy"), res["ctx_patch_sample"])
    big = np.load(tmp_path / "d" / "big_sample.npy")
    assert 0 < big.size < 10 << 20 and np.all(np.diff(big) > 0)


def test_bench_line_dtype_follows_the_gemm_split(monkeypatch):
    """bench.py states the recursion's dtype without running an instrumented step: gemm_split() gives what the LSTM output-gate
    launch reports to the kernel timer for each PATHS_GEMM_MODE, the exact bf16 split for a batch outside the fp16 range, and
    plain f32 without an LSTM cell."""
    import types
    import bench
    from paths_amd import ops
    from paths_amd.config import Config
    cfg = Config.load(os.path.join(os.path.dirname(__file__), "golden", "sample"), test_mode=True)
    batch = types.SimpleNamespace(feat_absmax=3.0, dim=1024)
    fallbacks = list(ops.RANGE_FALLBACKS)
    for mode, want in (("h3", (True, 2)), ("x6", (True, 3)), ("f32", (False, 0))):
        monkeypatch.setattr(ops, "GEMM_MODE", mode)
        assert bench.gemm_split(cfg, batch) == want, mode
    monkeypatch.setattr(ops, "GEMM_MODE", "h3")
    assert bench.gemm_split(cfg, types.SimpleNamespace(feat_absmax=1e6, dim=1024)) == (True, 3)
    assert ops.GEMM_MODE == "h3"                                 # (the range guard restores the mode)
    ops.RANGE_FALLBACKS[:] = fallbacks
    cfg.model_config.lstm = False
    assert bench.gemm_split(cfg, batch) == (False, 0)
    assert bench.infer_dtype(True, 2).startswith("f32 (products as 2 fp16 planes") and bench.infer_dtype(False, 0) == "f32"
