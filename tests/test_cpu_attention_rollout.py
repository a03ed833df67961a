"""CPU side of the special token's attention rollout: the float64 restatement (tests/rollout_ref.py) against the reference's own modules,
host-side argument checks of the paths_attention_rollout_* entry points (no launch), the recursion's flag check and the rasters of
paths_amd.heatmap.rollout_map."""
import numpy as np
import pytest
import torch

from tests import rollout_ref as R


def _decoder(d, nhead, layers, seed):
    torch.manual_seed(seed)
    layer = torch.nn.TransformerDecoderLayer(d, nhead, dim_feedforward=2 * d, dropout=0.0, batch_first=True)
    dec = torch.nn.TransformerDecoder(layer, num_layers=layers).double().eval()
    with torch.no_grad():
        for prm in dec.parameters():
            prm.add_(torch.randn_like(prm) * 0.3)           # (non-trivial biases and norms)
    return dec


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_rollout_ref_matches_the_reference_modules(layers):
    """Layer inputs captured with forward pre-hooks on a float64 nn.TransformerDecoder (batch_first, key padding mask, the empty memory
    PATHS passes); each layer's self_attn(need_weights=True, average_attn_weights=True); the product formed explicitly."""
    d, nhead, T = 16, 4, 7
    dec = _decoder(d, nhead, layers, 11 + layers)
    num_ims = torch.tensor([T - 1, 2, 0])                  # a full slide, a padded one, one without patches
    B = len(num_ims)
    S = torch.randn((B, T, d), dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    mask = torch.arange(T)[None, :] >= (num_ims + 1)[:, None]
    inputs = []
    hooks = [lyr.register_forward_pre_hook(lambda m, args, kw: inputs.append(args[0] if args else kw["tgt"]), with_kwargs=True)
             for lyr in dec.layers]
    with torch.no_grad():
        dec(S, torch.zeros((B, 0, d), dtype=torch.float64), tgt_key_padding_mask=mask)
        for h in hooks:
            h.remove()
        assert len(inputs) == layers
        mats = [dec.layers[l].self_attn(x, x, x, key_padding_mask=mask, need_weights=True, average_attn_weights=True)[1]
                for l, x in enumerate(inputs)]                                           # [B, T, T] each
    want_roll = torch.zeros((B, T - 1), dtype=torch.float64)
    want_self = torch.zeros((B,), dtype=torch.float64)
    for b in range(B):
        n1 = int(num_ims[b]) + 1
        r = torch.zeros((n1,), dtype=torch.float64)
        r[0] = 1.0
        for l in range(layers - 1, -1, -1):
            r = r @ (0.5 * mats[l][b, :n1, :n1] + 0.5 * torch.eye(n1, dtype=torch.float64))
        want_roll[b, : n1 - 1], want_self[b] = r[1:], r[0]
    sd = dec.state_dict()
    roll, self_ = R.decoder_rollout64(sd, "", S, num_ims, nhead, layers)
    assert (roll - want_roll).abs().max() <= 1e-12 and (self_ - want_self).abs().max() <= 1e-12
    assert (roll.sum(1) + self_ - 1).abs().max() <= 1e-12
    assert float(self_[2]) == 1.0 and (roll[1, 2:] == 0).all()
    # one step through layer 0 (both token orders) is the same product
    r_in = torch.zeros((B, T), dtype=torch.float64)
    for b in range(B):
        r_in[b, : int(num_ims[b]) + 1] = torch.rand(int(num_ims[b]) + 1, dtype=torch.float64)
    w, bb = sd["layers.0.self_attn.in_proj_weight"], sd["layers.0.self_attn.in_proj_bias"]
    for b in range(B):
        n1 = int(num_ims[b]) + 1
        want = 0.5 * r_in[b, :n1] + 0.5 * (r_in[b, :n1] @ mats[0][b, :n1, :n1])
        got = R.step64(inputs[0], num_ims, w, bb, nhead, 0, r_in)[b, :n1]
        assert (got - want).abs().max() <= 1e-12
        x_last = inputs[0].clone()                                                        # special token last: patch j at row j
        for bi in range(B):
            n = int(num_ims[bi])
            x_last[bi, :n], x_last[bi, n] = inputs[0][bi, 1:n + 1], inputs[0][bi, 0]
        assert (R.step64(x_last, num_ims, w, bb, nhead, 1, r_in)[b, :n1] - want).abs().max() <= 1e-12


def test_rollout_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    prep = lambda B, T, d, H, sl: lib.paths_attention_rollout_prepare(None, None, None, None, None, B, T, d, H, sl, None)
    assert prep(2, 65, 130, 4, 0) == -1 and b"d % H" in lib.paths_last_error()
    assert prep(2, 65, 4096, 4, 0) == -1 and b"2048" in lib.paths_last_error()
    assert prep(2, 65, 128, 4, 2) == -1 and b"special_last" in lib.paths_last_error()
    assert prep(2, 65, 128, 4, 1) == -1 and b"null" in lib.paths_last_error()
    step = lambda B, T, d, H: lib.paths_attention_rollout_step(None, None, None, None, None, 0, None, B, T, d, H, None)
    assert step(2, 65, 130, 4) == -1 and b"d % H" in lib.paths_last_error()
    assert step(2, 65, 4096, 4) == -1 and b"2048" in lib.paths_last_error()
    assert step(2, 65, 128, 4) == -1 and b"null" in lib.paths_last_error()
    assert lib.paths_attention_rollout_seed(None, 0, None, 0, None, None, None, 0, None, 2, 65, 4, None) == -1
    assert b"null" in lib.paths_last_error()
    with pytest.raises(_lib.PathsHipError):
        _lib.call("paths_attention_rollout_prepare", None, None, None, None, None, 2, 65, 128, 3, 0, None)
    # workspace: Q and K rows (head_dim padded to 16) + (m, l) per query row, per prepared layer
    assert lib.paths_attention_rollout_workspace(8, 2049, 128, 4) == 8 * 4 * 2049 * (2 * 32 + 2)
    assert lib.paths_attention_rollout_workspace(4, 65, 160, 4) == 4 * 4 * 65 * (2 * 48 + 2)
    assert lib.paths_attention_rollout_workspace(4, 8193, 1536, 24) == 4 * 24 * 8193 * (2 * 64 + 2)
    assert lib.paths_attention_rollout_workspace(2, 65, 130, 4) == 0


def test_recurse_rollout_needs_a_trace():
    from paths_amd import utils as putils
    with pytest.raises(ValueError):
        putils.recurse(None, [], [], 1, rollout=True)


def _two_levels():
    # level 0: 2 x 1 grid, both patches visited; level 1 (4 x 2 grid): two children of patch (0, 0) and one of patch (1, 0)
    lv0 = {"locs": np.array([[0, 0], [256, 0]]), "importance": np.array([0.5, 0.25], np.float32),
           "rollout": np.array([0.375, 0.125], np.float32), "rollout_self": 0.5}
    lv1 = {"locs": np.array([[0, 1], [1, 0], [3, 1]]) * 256, "importance": np.array([0.1, 0.2, 0.3], np.float32),
           "rollout": np.array([0.25, 0.0625, 0.1875], np.float32), "rollout_self": 0.5}
    return [lv0, lv1]


def test_rollout_map_two_level_hierarchy():
    from paths_amd.heatmap import rollout_map
    m0, m1 = rollout_map(_two_levels(), (2, 1))
    assert m0.shape == m1.shape == (4, 2)
    want0 = np.zeros((4, 2))
    want0[0:2, :], want0[2:4, :] = 0.375, 0.125                      # a level-0 patch covers 2 x 2 finest cells
    np.testing.assert_array_equal(m0, want0)
    want1 = np.zeros((4, 2))
    want1[0, 1], want1[1, 0], want1[3, 1] = 0.25, 0.0625, 0.1875
    np.testing.assert_array_equal(m1, want1)                         # 0 where level 1 did not visit; no fold into level 0
    with pytest.raises(KeyError):
        rollout_map([{k: v for k, v in lv.items() if not k.startswith("rollout")} for lv in _two_levels()], (2, 1))


def test_hierarchy_from_trace_carries_rollout():
    from paths_amd.heatmap import hierarchy_from_trace
    N = 4
    roll = torch.tensor([[0.25, 0.125, 0.0625, 0.0], [0.5, 0.0, 0.0, 0.0]])
    tr = [{"num_ims": torch.tensor([3, 1]), "locs": torch.zeros((2, N, 2), dtype=torch.int64), "importance": torch.rand(2, N),
           "parent_inds": torch.zeros((2, N), dtype=torch.int64), "rollout": roll, "rollout_self": torch.tensor([0.5625, 0.5])}]
    lv = hierarchy_from_trace(tr, 0)[0]
    np.testing.assert_array_equal(lv["rollout"], roll[0, :3].numpy())
    assert lv["rollout_self"] == 0.5625
    lv1 = hierarchy_from_trace(tr, 1)[0]
    np.testing.assert_array_equal(lv1["rollout"], np.array([0.5], np.float32))
    assert "rollout" not in hierarchy_from_trace([{k: v for k, v in tr[0].items() if not k.startswith("rollout")}], 1)[0]
