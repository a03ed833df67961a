"""The memory-cell gate GEMM of paths_lstm_cell_x6 / paths_lstm_cell_x6_h16 at depth 0 (no h0, c0, hp, no training save, two-plane
split): it computes the remember | map column groups only (EpiLstmC0, csrc/gemm_epi.h; the forget groups of the packed image are
skipped while W is staged, w_group() in csrc/gemm_x6.hip), because c0 = 0 never meets the forget gate.

What it writes must equal the full-width form bit for bit.  The full-width form is reached through the same entry point with a zero c0
buffer and parent partials whose every hp_row is -1 (zero seeds): all three gates are computed and 0 * sigmoid(f) is added.  float64
(tests/chain_ref.py, at the tolerances of tests/test_gpu_chain_forward.py) is the reference of the values, and a recording of the
previous commit's kernels on the same seeded inputs (tests/golden/gate_launch.npz) the reference across commits.

Shapes: D = 256, Hc = 128 (the smallest the split kernels accept); M = 8448 = 22 slides x 384 rows for the 256-row tile family
(just above its switch at 8192 rows) and M = 384 = 2 slides x 192 rows for the 128-row family.  The ragged counts put the last valid
row of slide 0 on the FIRST row of a tile and leave the tile after it without a valid row (the padding exit)."""
import hashlib
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_chain_forward as C
from tests.test_gpu_parity import dev  # noqa: F401  (fixture)

D, HC = 256, 128
SHAPES = {8448: (384, 256), 384: (192, 128)}          # M -> (rows per slide of the ragged runs, rows of a tile of its family)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gate_launch.npz")


def _counts(M, rps, tile):
    """Slide 0 ends on the first row of the second tile; slide 1 is empty, so the tile [2 tile, 3 tile) inside it has no valid row."""
    assert tile < rps <= 2 * tile and 3 * tile <= 2 * rps
    base = [tile + 1, 0, rps, rps // 3, 1, rps - 1]
    return torch.tensor([base[b % len(base)] for b in range(M // rps)], dtype=torch.int64, device=C.DEV)


def _run(pr, a_form, phases=(7,), num_ims=None, rps=None, full_width=False):
    """One inference cell evaluation of the depth-0 problem ``pr``; full_width: the same values through the three-gate form."""
    bufs = C._lstm_buffers(pr, "inf")
    keep = []
    for ph in phases:
        a = C._lstm_args(pr, bufs, 2, a_form, num_ims, rps, ph)
        if full_width:
            M = pr["M"]
            hp = torch.full((2, 3 * HC + D), float("nan"), device=C.DEV)          # never selected: every row is an orphan
            row = torch.full((M,), -1, dtype=torch.int32, device=C.DEV)
            c0 = torch.zeros((M, HC), device=C.DEV)
            a.update(hp=hp.data_ptr(), hp_row=row.data_ptr(), c0=c0.data_ptr(), ldc0=HC)
            keep += [hp, row, c0]
        C._lstm_call(C._lstm_entry(2, a_form), a)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.gpu
@pytest.mark.parametrize("a_form", ["matrix", "rows", "h16"])
@pytest.mark.parametrize("M", sorted(SHAPES))
def test_depth0_cell_equals_the_full_width_form(dev, M, a_form):
    """h1 | c1 and the raw gate scratch of the depth-0 form are bit-identical to the three-gate form's at both tile families, for
    fp32 matrices, row pointers and fp16 rows, with phases 7 and 1, 2, 4, without num_ims and with the ragged counts (where rows
    of skipped tiles keep the sentinel in both); the depth-0 run is also checked against float64 and for writes out of bounds."""
    pr = C._lstm_problem(D, HC, M, "none", False, a_form in ("rows", "h16"))
    label = f"depth0 {M}-{a_form}"
    got = _run(pr, a_form)
    C._lstm_check(pr, got, "inf", label)
    full = _run(pr, a_form, full_width=True)
    C._same_buffers(got, full, label + " against the full-width form")
    C._same_buffers(got, _run(pr, a_form, phases=(1, 2, 4)), label + " phases 1, 2, 4")
    rps, tile = SHAPES[M]
    num_ims = _counts(M, rps, tile)
    ragged = _run(pr, a_form, num_ims=num_ims, rps=rps)
    C._same_buffers(ragged, _run(pr, a_form, num_ims=num_ims, rps=rps, full_width=True), label + " ragged")
    # the tile that ends slide 0 was computed (its first row is valid), the all-padding tile behind it was left alone
    so = ragged["state_out"]
    assert torch.equal(C._bits(so[tile, :D + HC]), C._bits(got["state_out"][tile, :D + HC])), f"{label}: the last valid row of slide 0"
    assert C._untouched(so[2 * tile:3 * tile]), f"{label}: a tile of padding was written"
    C._lstm_guards(pr, ragged, "inf", label + " ragged")


@pytest.mark.gpu
def test_depth0_cell_with_saturated_gates(dev):
    """Biases at +-{20, 50, 100}: the remember gate and the map saturate on both sides; still bit-identical to the full-width form
    (whose forget gate saturates too: 0 * sigmoid(f) stays an exact zero) and inside the float64 bounds."""
    pr = C._lstm_problem(D, HC, 300, "none", True, False)
    got = _run(pr, "matrix")
    C._lstm_check(pr, got, "inf", "depth0 saturated")
    C._same_buffers(got, _run(pr, "matrix", full_width=True), "depth0 saturated against the full-width form")


def golden_outputs():
    """name -> the h1 | c1 rows of one inference call (phases 7) on fp16 rows per tile family and state (depth 0, parent partials):
    what tests/golden/gate_launch.npz records (24 evenly spaced rows, and the SHA-256 of all of them)."""
    out = {}
    for M in sorted(SHAPES):
        for state in ("none", "hp"):
            pr = C._lstm_problem(D, HC, M, state, False, True)
            bufs = C._lstm_run(pr, 2, "h16", "inf")
            so = bufs["state_out"][:M, :D + HC].contiguous().cpu().numpy()
            out[f"{state}_m{M}_rows"] = so[::M // 24].copy()
            out[f"{state}_m{M}_sha256"] = np.frombuffer(hashlib.sha256(so.tobytes()).digest(), dtype=np.uint8).copy()
    return out


@pytest.mark.gpu
def test_gate_outputs_equal_the_recorded_ones(dev):
    """h1 | c1 at depth 0 and from parent partials, both tile families, are bit-identical to the recording made with the kernels of
    the commit before the depth-0 form (the inputs are regenerated from their seeds; the recording holds 24 evenly spaced rows and the
    hash of the whole block)."""
    want = np.load(GOLDEN)
    got = golden_outputs()
    assert sorted(want.files) == sorted(got)
    for k in sorted(got):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), f"{k} differs from the recording"


def test_depth0_column_groups_are_the_remember_and_map_rows():
    """No GPU: column group g of the depth-0 product reads 32-row group 3 (g // 2) + 1 + g % 2 of the packed gate image (w_group() in
    csrc/gemm_x6.hip) and the bias entries of the same rows; in ops.pack_lstm's layout of the module's own weights those are the
    remember-gate rows (g even) and the remember-map rows (g odd) of memory units 32 (g // 2) .. + 31, x half in columns [0, D)."""
    from paths_amd import ops
    d, hc = 64, 128
    g = torch.Generator().manual_seed(3)
    lstm = torch.nn.Module()
    for name, rows, cols in (("forget_gate", hc, 2 * d), ("remember_gate", hc, 2 * d), ("remember_map", hc, 2 * d),
                             ("out_select_gate", d, 2 * d), ("mem_to_out", d, hc)):
        lin = torch.nn.Linear(cols, rows)
        with torch.no_grad():
            lin.weight.copy_(torch.rand((rows, cols), generator=g))
            lin.bias.copy_(torch.rand((rows,), generator=g))
        setattr(lstm, name, torch.nn.Sequential(lin))
    pk = ops.pack_lstm(lstm)
    assert pk["w_gates"].shape == (3 * hc + d, 2 * d)
    for grp in range(2 * hc // 32):
        src = 3 * (grp // 2) + 1 + grp % 2
        mod = (lstm.remember_gate if grp % 2 == 0 else lstm.remember_map)[0]
        units = slice(32 * (grp // 2), 32 * (grp // 2) + 32)
        assert torch.equal(pk["w_gates"][32 * src:32 * src + 32], mod.weight[units]), grp
        assert torch.equal(pk["b_gates"][32 * src:32 * src + 32], mod.bias[units]), grp
        assert src < 3 * hc // 32 and src % 3 != 0                          # inside the c part, never a forget group
    covered = sorted(3 * (grp // 2) + 1 + grp % 2 for grp in range(2 * hc // 32))
    assert covered == [s for s in range(3 * hc // 32) if s % 3 != 0]        # every remember / map group once
