"""CPU side of the special token's attention export: host-side argument checks of paths_token0_attention (no launch) and the
rasters of paths_amd.heatmap.attention_map."""
import numpy as np
import pytest
import torch


def test_token0_attention_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    args = lambda B, T, d, H, sl: (None, None, None, None, None, 0, None, 0, None, B, T, d, H, sl, None)
    rc = lib.paths_token0_attention(*args(2, 65, 130, 4, 0))                 # 130 % 4 != 0
    assert rc == -1 and b"d % H" in lib.paths_last_error()
    rc = lib.paths_token0_attention(*args(2, 65, 4096, 4, 0))                # wider than any aggregator
    assert rc == -1 and b"2048" in lib.paths_last_error()
    rc = lib.paths_token0_attention(*args(2, 65, 128, 4, 2))                 # no such token order
    assert rc == -1 and b"special_last" in lib.paths_last_error()
    rc = lib.paths_token0_attention(*args(2, 65, 128, 4, 1))                 # valid geometry, null buffers
    assert rc == -1 and b"null" in lib.paths_last_error()
    with pytest.raises(_lib.PathsHipError):
        _lib.call("paths_token0_attention", *args(2, 65, 128, 3, 0))
    assert lib.paths_token0_attention_workspace(8, 2049, 128, 4) >= 8 * 4 * 128


def test_recurse_attention_needs_a_trace():
    from paths_amd import utils as putils
    with pytest.raises(ValueError):
        putils.recurse(None, [], [], 1, attention=True)


def _two_levels():
    # level 0: 2 x 1 grid, both patches visited; level 1 (4 x 2 grid): two children of patch (0, 0) and one of patch (1, 0)
    # attention [L = 2 layers, H = 2 heads, n]
    lv0 = {"locs": np.array([[0, 0], [256, 0]]), "importance": np.array([0.5, 0.25], np.float32),
           "attention": np.array([[[0.6, 0.2], [0.2, 0.4]], [[0.5, 0.3], [0.1, 0.7]]], np.float32),
           "attention_self": np.array([[0.2, 0.4], [0.2, 0.2]], np.float32)}
    lv1 = {"locs": np.array([[0, 1], [1, 0], [3, 1]]) * 256, "importance": np.array([0.1, 0.2, 0.3], np.float32),
           "attention": np.array([[[0.1, 0.2, 0.3], [0.3, 0.2, 0.1]], [[0.25, 0.25, 0.5], [0.5, 0.125, 0.125]]], np.float32),
           "attention_self": np.zeros((2, 2), np.float32)}
    return [lv0, lv1]


def test_attention_map_two_level_hierarchy():
    from paths_amd.heatmap import attention_map
    levels = _two_levels()
    m0, m1 = attention_map(levels, (2, 1))                         # last layer, mean over heads
    assert m0.shape == m1.shape == (4, 2)
    want0 = np.zeros((4, 2))
    want0[0:2, :] = (0.5 + 0.1) / 2                                # patch (0, 0): footprint 2 x 2 finest cells
    want0[2:4, :] = (np.float32(0.3) + np.float32(0.7)) / 2
    np.testing.assert_allclose(m0, want0, rtol=0, atol=1e-7)
    want1 = np.zeros((4, 2))
    want1[0, 1], want1[1, 0], want1[3, 1] = (0.25 + 0.5) / 2, (0.25 + 0.125) / 2, (0.5 + 0.125) / 2
    np.testing.assert_allclose(m1, want1, rtol=0, atol=1e-7)      # 0 where level 1 did not visit; no fold from level 1 into 0
    h0, h1 = attention_map(levels, (2, 1), layer=0, head=1)
    want0 = np.zeros((4, 2))
    want0[0:2, :], want0[2:4, :] = np.float32(0.2), np.float32(0.4)
    np.testing.assert_array_equal(h0, want0)
    want1 = np.zeros((4, 2))
    want1[0, 1], want1[1, 0], want1[3, 1] = np.float32(0.3), np.float32(0.2), np.float32(0.1)
    np.testing.assert_array_equal(h1, want1)
    with pytest.raises(KeyError):
        attention_map([{k: v for k, v in lv.items() if not k.startswith("attention")} for lv in levels], (2, 1))


def test_hierarchy_from_trace_carries_attention():
    from paths_amd.heatmap import hierarchy_from_trace, importance_map
    L, H, N = 2, 2, 4
    att = torch.arange(2 * L * H * N, dtype=torch.float32).view(2, L, H, N)
    tr = [{"num_ims": torch.tensor([3, 1]), "locs": torch.zeros((2, N, 2), dtype=torch.int64), "importance": torch.rand(2, N),
           "parent_inds": torch.zeros((2, N), dtype=torch.int64), "attention": att, "attention_self": torch.ones(2, L, H)}]
    lv = hierarchy_from_trace(tr, 0)[0]
    np.testing.assert_array_equal(lv["attention"], att[0, :, :, :3].numpy())
    assert lv["attention_self"].shape == (L, H)
    assert "attention" not in hierarchy_from_trace([{k: v for k, v in tr[0].items() if not k.startswith("attention")}], 1)[0]
    # the shared painter leaves importance_map as it was: importance + 1e-4, folded upwards with weight 1/2
    levels = _two_levels()
    m = importance_map(levels, (2, 1))
    want = np.zeros((2, 4, 2))
    for depth, lvl in enumerate(levels):
        size = 2 ** (1 - depth)
        for (cx, cy), v in zip(lvl["locs"] // 256, lvl["importance"]):
            want[depth, cx * size:(cx + 1) * size, cy * size:(cy + 1) * size] = v + 1e-4
    msk = want[1] != 0
    want[0][msk] = want[0][msk] + want[1][msk] * 0.5
    np.testing.assert_array_equal(m, want[0])
