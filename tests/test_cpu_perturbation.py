"""CPU side of the deletion / insertion curves (paths_amd/saliency.py:perturbation_curves): the properties of the numpy
restatement of the two kernels (tests/perturb_ref.py), the count formula, the argument checks, the header / binding / source list
of the two entry points and their host-side argument validation."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import perturb_ref as P

SEG = (37, 5, 130)
NUMS = np.array([[0, 37], [5, 1], [130, 64]])
TIES = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32)


def _scores(seed, ties):
    g = np.random.default_rng(seed)
    n = sum(SEG)
    s = TIES[g.integers(0, len(TIES), (2, n))] if ties else g.standard_normal((2, n)).astype(np.float32)
    s[~P.valid_mask(SEG, NUMS)] = np.nan
    return s


# ------------------------------------------------------------------------------------------------
# the restatement's own properties
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("level_on", [None, (1, 0, 1)])
def test_ranks_are_a_permutation_in_the_stated_order(ties, ascending, level_on):
    s = _scores(3, ties)
    rank, count = P.rank_joint(s, SEG, NUMS, level_on, ascending)
    valid = P.valid_mask(SEG, NUMS, level_on)
    assert rank.dtype == np.int32 and (rank[~valid] == -1).all() and count.tolist() == valid.sum(1).tolist()
    for b in range(2):
        idx = np.nonzero(valid[b])[0]
        assert sorted(rank[b, idx].tolist()) == list(range(len(idx)))                  # a permutation of 0 .. n_b - 1
        by_rank = idx[np.argsort(rank[b, idx])]
        v = s[b, by_rank].astype(np.float64) * (1.0 if ascending else -1.0)
        assert not np.isnan(v).any()
        # the values never decrease along the ranks (-0 == +0), and equal values come in ascending joint index
        assert (v[1:] >= v[:-1]).all()
        same = v[1:] == v[:-1]
        assert (by_rank[1:][same] > by_rank[:-1][same]).all()
    if level_on is not None:
        assert (rank[:, SEG[0]:SEG[0] + SEG[1]] == -1).all()


def test_minus_zero_orders_as_plus_zero_and_infinities_are_ordinary():
    s = np.array([[0.0, -0.0, np.inf, -np.inf, -0.0, 1.0]], np.float32)
    rank, count = P.rank_joint(s, (6,), [[6]])
    assert rank.tolist() == [[2, 3, 0, 5, 4, 1]] and count.tolist() == [6]
    rank, _ = P.rank_joint(s, (6,), [[6]], ascending=True)
    assert rank.tolist() == [[1, 2, 5, 0, 3, 4]]


def test_counts_formula():
    for steps in (1, 3, 4, 16):
        for n in (0, 1, 2, 7, 130, 34816):
            c = P.counts([n], steps)[:, 0]
            assert c[0] == 0 and c[steps] == n and (np.diff(c) >= 0).all()
            assert all(abs(int(c[s]) - s * n / steps) <= 0.5 for s in range(steps + 1))
    from paths_amd.saliency import perturbation_counts
    n = [0, 1, 19, 130, 34816]
    for steps in (1, 4, 16):
        np.testing.assert_array_equal(perturbation_counts(n, steps), P.counts(n, steps))


def test_kept_sets_are_nested_and_padded_rows_are_never_kept():
    s = _scores(5, False)
    rank, count = P.rank_joint(s, SEG, NUMS, (1, 0, 1))
    steps = 4
    thr, ins = P.curve_members(count, steps)
    off = 0
    for l, n in enumerate(SEG):
        k = P.kept(rank[:, off:off + n], thr, ins, NUMS[l])
        off += n
        valid = np.arange(n)[None, :] < NUMS[l][:, None]
        assert not k[:, ~valid].any()
        dele, inse = k[:steps + 1], k[steps + 1:]
        for a, b in zip(dele[:-1], dele[1:]):
            assert not (b & ~a).any()                                                   # deletion only removes
        for a, b in zip(inse[:-1], inse[1:]):
            assert not (a & ~b).any()                                                   # insertion only adds
        if l == 1:                                                                      # a level that is not chosen stays as recorded
            assert (k == valid[None]).all()
        else:
            assert (dele[0] == valid).all() and not dele[-1].any() and not inse[0].any() and (inse[-1] == valid).all()
            assert (dele[1:-1] != inse[1:-1]).any()
    # over all levels a member removes exactly its threshold
    removed = sum((~P.kept(rank[:, o:o + n], thr, ins, NUMS[l]) & (np.arange(n)[None, :] < NUMS[l][:, None])[None]).sum(-1)
                  for l, (o, n) in enumerate(zip(np.cumsum((0,) + SEG[:-1]), SEG)))
    np.testing.assert_array_equal(removed[:steps + 1], thr[:steps + 1])
    np.testing.assert_array_equal(removed[steps + 1:], count[None, :] - thr[steps + 1:])


def test_deletion_on_v_is_insertion_on_minus_v():
    """Without ties: deleting the first k ranks of v leaves the rows that inserting the first n - k ranks of -v presents."""
    s = _scores(9, False)
    r1, count = P.rank_joint(s, SEG, NUMS)
    r2, _ = P.rank_joint(-s, SEG, NUMS)
    valid = P.valid_mask(SEG, NUMS)
    for b in range(2):
        assert (r1[b, valid[b]] + r2[b, valid[b]] == count[b] - 1).all()
    ks = np.array([[0, 0], [1, 1], [40, 17], [count[0], count[1]]])
    off = SEG[0] + SEG[1]
    d = P.kept(r1[:, off:], ks, np.zeros(len(ks), int), NUMS[2])
    i = P.kept(r2[:, off:], count[None, :] - ks, np.ones(len(ks), int), NUMS[2])
    assert (d == i).all() and d.any() and not d.all()


def test_mask_points_copies_bits():
    g = np.random.default_rng(1)
    x = g.standard_normal((2, 7, 8)).astype(np.float32)
    x[0, 0, 0] = -0.0
    x[1, 3:] = np.nan
    base = g.standard_normal(8).astype(np.float32)
    rank = np.array([[3, 0, -1, 2, 1, 4, 5], [1, 0, 2, -1, -1, -1, -1]], np.int32)
    thr, ins, num = np.array([[2, 1], [2, 1], [0, 3]]), np.array([0, 1, 0]), [7, 3]
    for bs in (base, None):
        out = P.mask_points(x, bs, rank, thr, ins, num).reshape(3, 2, 7, 8)
        k = P.kept(rank, thr, ins, num)
        assert out.dtype == np.float32
        want = np.zeros(8, np.float32) if bs is None else bs
        for c in range(3):
            for b in range(2):
                for r in range(7):
                    row = out[c, b, r].view(np.uint32)
                    if r >= num[b]:
                        assert not row.any()
                    else:
                        assert (row == (x[b, r] if k[c, b, r] else want).view(np.uint32)).all()
    assert k[0, 0].tolist() == [True, False, True, True, False, True, True] and k[1, 0].tolist() == [False, True, True, False, True, False, False]


# ------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    from paths_amd import saliency
    from paths_amd.data_utils import slide as S
    model = types.SimpleNamespace(use_lstm=True)
    fn = saliency.perturbation_curves
    with pytest.raises(NotImplementedError, match="lstm=false"):
        fn(types.SimpleNamespace(use_lstm=False), [], [2], 2, "importance")
    od = [S.OnDemandSlide([(2, 2)], lambda l, c: torch.zeros(len(c), 8), 8, "cpu")]
    with pytest.raises(NotImplementedError, match="on-demand"):
        fn(model, od, [2], 2, "importance")
    with pytest.raises(ValueError, match="unknown target"):
        fn(model, [], [2], 2, "importance", target="hazard")
    for steps in (0, -3, 2.0):
        with pytest.raises(ValueError, match="steps"):
            fn(model, [], [2], 2, "importance", steps=steps)
    with pytest.raises(ValueError, match="mode"):
        fn(model, [], [2], 2, "importance", mode="removal")
    for levels in ([2], [-1], [0, 5]):
        with pytest.raises(ValueError, match="levels"):
            fn(model, [], [2], 2, "importance", levels=levels)
    for bad in (torch.zeros(2, 3), torch.zeros(()), [0.0] * 8):
        with pytest.raises(ValueError, match="baseline"):
            fn(model, [], [2], 2, "importance", baseline=bad)
    for bad in ([torch.zeros(1, 4)], torch.zeros(2, 1, 4), 3):
        with pytest.raises(ValueError, match="scores"):
            fn(model, [], [2], 2, bad)
    for bad in ([{}], [{}, {}]):
        with pytest.raises(ValueError, match="trace"):
            fn(model, [], [2], 2, "importance", trace=bad)


# ------------------------------------------------------------------------------------------------
# the C surface
# ------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_binding_matches():
    from paths_amd import _lib
    for name, nargs in (("paths_rank_joint", 11), ("paths_path_mask_points", 14), ("paths_rank_joint_tile", 0)):
        assert name in _lib.DECLARATIONS, f"{name} is not declared in include/paths_hip.h"
        res, args = _lib.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == len(_lib.SIGNATURES[name]) == nargs
    assert _lib.ABI_VERSION == 3                                      # no existing signature changed
    import __graft_entry__ as g
    assert "perturb_rows.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "perturb_rows.hip"))


def test_build_compiles_the_new_file_and_exports_the_entry_points():
    import __graft_entry__ as g
    from paths_amd import _lib
    g.build()
    lib = _lib.load()
    assert lib.paths_abi_version() == 3
    for name in ("paths_rank_joint", "paths_path_mask_points", "paths_rank_joint_tile"):
        assert hasattr(lib, name)
    tile = lib.paths_rank_joint_tile()
    assert tile >= 8 and tile % 8 == 0 and tile * 8 <= 64 * 1024
    if os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        assert os.path.getmtime(os.path.join(g.OBJDIR, "perturb_rows.o")) >= os.path.getmtime(os.path.join(g.CSRC, "perturb_rows.hip"))


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    from paths_amd import _lib
    lib = _lib.load()
    A = 4096                                    # (an aligned non-null address: never dereferenced, every call below is rejected)
    rj = lambda sc, se, on, ni, L, B, n, asc, rk, ct: lib.paths_rank_joint(sc, se, on, ni, L, B, n, asc, rk, ct, None)
    assert rj(None, A, A, A, 3, 2, 100, 0, A, A) == -1 and b"null" in lib.paths_last_error()
    assert rj(A, A, A, A, 3, 2, 100, 0, A, None) == -1 and b"null" in lib.paths_last_error()
    assert rj(A, A, A, A, 0, 2, 100, 0, A, A) == -1 and b"L (0)" in lib.paths_last_error()
    assert rj(A, A, A, A, 17, 2, 100, 0, A, A) == -1 and b"L (17)" in lib.paths_last_error()
    assert rj(A, A, A, A, 3, 0, 100, 0, A, A) == -1 and b"B (0)" in lib.paths_last_error()
    assert rj(A, A, A, A, 3, 2, 0, 0, A, A) == -1 and b"n_tot" in lib.paths_last_error()
    assert rj(A, A, A, A, 3, 2, (1 << 30) + 1, 0, A, A) == -1 and b"n_tot" in lib.paths_last_error()
    assert rj(A + 2, A, A, A, 3, 2, 100, 0, A, A) == -1 and b"aligned" in lib.paths_last_error()
    assert rj(A, A, A, A + 4, 3, 2, 100, 0, A, A) == -1 and b"aligned" in lib.paths_last_error()
    mp = lambda x, ldx, base, rk, ldr, thr, ins, ni, N, D, B, C, out: lib.paths_path_mask_points(x, ldx, base, rk, ldr, thr, ins, ni, N, D, B,
                                                                                               C, out, None)
    assert mp(None, 128, None, A, 4, A, A, A, 4, 128, 2, 1, A) == -1 and b"null" in lib.paths_last_error()
    assert mp(A, 128, None, None, 4, A, A, A, 4, 128, 2, 1, A) == -1 and b"null" in lib.paths_last_error()
    assert mp(A, 128, None, A, 4, A, None, A, 4, 128, 2, 1, A) == -1 and b"null" in lib.paths_last_error()
    assert mp(A, 128, None, A, 4, A, A, A, 4, 64, 2, 1, A) == -1 and b"multiple of 128" in lib.paths_last_error()
    assert mp(A, 128, None, A, 4, A, A, A, 4, 128, 2, 0, A) == -1 and b"positive" in lib.paths_last_error()
    assert mp(A, 128, None, A, 4, A, A, A, 0, 128, 2, 1, A) == -1 and b"positive" in lib.paths_last_error()
    assert mp(A, 126, None, A, 4, A, A, A, 4, 128, 2, 1, A) == -1 and b"row stride" in lib.paths_last_error()
    assert mp(A, 128, None, A, 3, A, A, A, 4, 128, 2, 1, A) == -1 and b"rank stride" in lib.paths_last_error()
    assert mp(A, 128, A + 4, A, 4, A, A, A, 4, 128, 2, 1, A) == -1 and b"aligned" in lib.paths_last_error()
    assert mp(A, 128, None, A + 2, 4, A, A, A, 4, 128, 2, 1, A) == -1 and b"aligned" in lib.paths_last_error()
    with pytest.raises(_lib.PathsHipError, match=r"paths_rank_joint failed \(-1\)"):
        _lib.call("paths_rank_joint", None, None, None, None, 3, 2, 100, 0, None, None, None)
