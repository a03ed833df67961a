"""CPU checks of tests/rows_ref.py: every closed form against torch.autograd in float64 over the oracle's forward formulas (LSTM cell,
importance MLP + sigmoid scaling + proj_in with and without the LSTM, F.layer_norm), at well-conditioned random points with a padded
slide and a slide without patches; the plumbing references against a plain Python loop."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import paths_oracle as orc
from tests import rows_ref as R

F64 = torch.float64


def close(a, b, tol=1e-10):
    a, b = a.detach().to(F64), b.detach().to(F64)
    scale = float(b.abs().max()) or 1.0
    return float((a - b).abs().max()) / scale < tol


def _u(g, *shape, s=1.0):
    return (torch.rand(*shape, generator=g, dtype=F64) * 2 - 1) * s


NUM_IMS = [5, 0, 3]          # a full slide, one without patches, a padded one
N = 5


def _lstm_params(g, D, Hc):
    p = {}
    for name in ("forget_gate", "remember_gate", "remember_map", "out_select_gate"):
        p[f"lstm.{name}.0.weight"] = _u(g, Hc if name != "out_select_gate" else D, 2 * D, s=1 / math.sqrt(2 * D)).requires_grad_(True)
        p[f"lstm.{name}.0.bias"] = _u(g, Hc if name != "out_select_gate" else D, s=0.5).requires_grad_(True)
    p["lstm.mem_to_out.0.weight"] = _u(g, D, Hc, s=1 / math.sqrt(Hc)).requires_grad_(True)
    p["lstm.mem_to_out.0.bias"] = _u(g, D, s=0.5).requires_grad_(True)
    return p


@pytest.mark.parametrize("depth0", [True, False])
@pytest.mark.parametrize("ext", [True, False])
def test_lstm_closed_forms_match_autograd_of_the_oracle_cell(depth0, ext):
    """lstm_bwd_a_ref + the mem_to_out product + lstm_bwd_b_ref give autograd's gradients of oracle.lstm_cell: dx, dh0, dc0 per row
    (which sum the four gate gradients through the weights) and every weight / bias gradient (each gate on its own)."""
    g = torch.Generator().manual_seed(11 + 2 * depth0 + ext)
    D, Hc = 64, 64
    M = len(NUM_IMS) * N
    valid = R.valid_rows(NUM_IMS, N)
    p = _lstm_params(g, D, Hc)
    x = _u(g, M, D).requires_grad_(True)
    h0 = (torch.zeros(M, D, dtype=F64) if depth0 else _u(g, M, D)).requires_grad_(True)
    c0 = (torch.zeros(M, Hc, dtype=F64) if depth0 else _u(g, M, Hc)).requires_grad_(True)
    gh, gc = _u(g, M, D), _u(g, M, Hc)                      # upstream gradients of h1 and c1
    gh_ext = _u(g, M, D) if ext else None                   # the h half of d_state_out (lstm_bwd_a's dh1b)
    h1, c1 = orc.lstm_cell(p, x, h0, c0)
    v = valid[:, None].to(F64)                              # padded rows receive no gradient
    loss = (h1 * (gh + (gh_ext if ext else 0)) * v).sum() + ((c1 * gc * v).sum() if ext else 0)
    loss.backward()
    # saved activations, as the forward kernel keeps them
    with torch.no_grad():
        xh = torch.cat((x, h0), 1)
        lin = lambda n: F.linear(xh, p[f"lstm.{n}.0.weight"], p[f"lstm.{n}.0.bias"])   # noqa: E731
        f, r, m = torch.sigmoid(lin("forget_gate")), torch.sigmoid(lin("remember_gate")), torch.tanh(lin("remember_map"))
        o = torch.sigmoid(lin("out_select_gate"))
        cc = c0 * f + r * m
        tc = torch.tanh(F.linear(cc, p["lstm.mem_to_out.0.weight"], p["lstm.mem_to_out.0.bias"]))
        frm = R.pack_gates(f, r, m)
        dpre_o, dpre_h = R.lstm_bwd_a_ref(gh, gh_ext, o, tc, valid)
        dc1_h = dpre_h @ p["lstm.mem_to_out.0.weight"]
        dgates, dc0 = R.lstm_bwd_b_ref(dc1_h, gc if ext else None, frm, None if depth0 else c0, valid)
        df, dr, dm = R.unpack_gates(dgates)
    W = {n: p[f"lstm.{n}.0.weight"] for n in ("forget_gate", "remember_gate", "remember_map", "out_select_gate")}
    pre = {"forget_gate": df, "remember_gate": dr, "remember_map": dm, "out_select_gate": dpre_o}
    dxh = sum(pre[n] @ W[n] for n in pre)
    assert close(dxh[:, :D], x.grad) and close(dxh[:, D:], h0.grad)
    if not depth0:
        assert close(dc0, c0.grad)
    else:                       # c0 = 0 at depth 0: df vanishes, and so does the forget-gate gradient
        assert float(df.abs().max()) == 0.0
    for n, dp in pre.items():
        assert close(dp.t() @ xh, p[f"lstm.{n}.0.weight"].grad), n
        assert close(dp.sum(0), p[f"lstm.{n}.0.bias"].grad), n
    assert close(dpre_h.t() @ cc, p["lstm.mem_to_out.0.weight"].grad)
    assert close(dpre_h.sum(0), p["lstm.mem_to_out.0.bias"].grad)
    for t in (dpre_o, dpre_h, dgates, dc0):
        assert not t[~valid].any()


def test_gate_packing_round_trip():
    """pack_gates puts unit 32 blk + jj at 96 blk + jj / + 32 / + 64 (the layout of csrc/bwd_rows.hip:lstm_bwd_b_kernel)."""
    Hc = 96
    f, r, m = (torch.arange(Hc, dtype=F64)[None, :] + k * 1000 for k in (1, 2, 3))
    x = R.pack_gates(f, r, m)
    for j in range(Hc):
        blk, jj = divmod(j, 32)
        assert x[0, 96 * blk + jj] == 1000 + j and x[0, 96 * blk + 32 + jj] == 2000 + j and x[0, 96 * blk + 64 + jj] == 3000 + j
    assert all(torch.equal(a, b) for a, b in zip(R.unpack_gates(x), (f, r, m)))


def _importance_forward(g, M, D, Hi, d, valid):
    Y = _u(g, M, D)
    W1, b1 = _u(g, Hi, D, s=1 / math.sqrt(D)), _u(g, Hi, s=0.3)
    w2, b2 = _u(g, Hi, s=1 / math.sqrt(Hi)), _u(g, 1, s=0.3)
    Wp = _u(g, d, D, s=1 / math.sqrt(D))
    return Y, W1, b1, w2, b2, Wp


@pytest.mark.parametrize("imp_mul", [1, 0])
def test_importance_closed_form_matches_autograd_lstm_form(imp_mul):
    """tokens[b, 1 + i] = alpha P + bp (alpha = valid sigmoid(w2 . relu(Y W1^T + b1) + b2), P = Y Wp^T; reference model/paths.py:95-98,
    119-124 as oracle.process_level evaluates them): importance_bwd_ref's dhid, dP, da and dah are autograd's gradients of the
    pre-relu, of P, of the sigmoid's input and of a per-row copy of w2, and [dhid | dP] [W1; Wp] is autograd's dY."""
    g = torch.Generator().manual_seed(3 + imp_mul)
    D, Hi, d = 48, 36, 40
    B = len(NUM_IMS)
    M = B * N
    valid = R.valid_rows(NUM_IMS, N)
    Y, W1, b1, w2, b2, Wp = _importance_forward(g, M, D, Hi, d, valid)
    Y = Y.requires_grad_(True)
    pre1 = (Y @ W1.t() + b1).detach().requires_grad_(True)
    P = (Y @ Wp.t()).detach().requires_grad_(True)
    w2r = w2.expand(M, Hi).clone().requires_grad_(True)
    hid = torch.relu(pre1)
    a = ((hid * w2r).sum(1) + b2).detach().requires_grad_(True)
    alpha = torch.where(valid, torch.sigmoid(a), 0.0)
    a2 = (hid * w2r).sum(1) + b2
    alpha2 = torch.where(valid, torch.sigmoid(a2), 0.0)
    tok = alpha2[:, None] * P if imp_mul else P
    dtok = _u(g, B, N + 1, d)
    dtok[:, 0] = 1e30                                       # row 0 is the special token: never read
    gr = torch.where(valid[:, None], dtok[:, 1:].reshape(M, d), 0.0)   # padded token rows carry zero gradient (masked keys)
    (tok * gr).sum().backward()
    da_auto = torch.autograd.grad((torch.where(valid, torch.sigmoid(a), 0.0)[:, None] * P.detach() * gr).sum(), a)[0] if imp_mul else torch.zeros(M, dtype=F64)
    dhid, dP, da, dah, _ = R.importance_bwd_ref(dtok, P.detach(), hid.detach(), alpha.detach(), w2, valid, N, imp_mul)
    zero = lambda t, like: torch.zeros_like(like) if t is None else t      # noqa: E731  (no path to the loss: importance_mode none)
    assert close(dhid, zero(pre1.grad, dhid)) and close(dP, P.grad)
    assert close(da, da_auto, 1e-10) and close(dah, zero(w2r.grad, dah))
    # the full Y path: dY = dU W_ip with W_ip = [W1; Wp] (paths_amd/backward.py: dy = du W_ip)
    Y2 = Y.detach().clone().requires_grad_(True)
    hid2 = torch.relu(Y2 @ W1.t() + b1)
    al2 = torch.where(valid, torch.sigmoid(hid2 @ w2 + b2), 0.0)
    P2 = Y2 @ Wp.t()
    ((al2[:, None] * P2 if imp_mul else P2) * gr).sum().backward()
    assert close(torch.cat((dhid, dP), 1) @ torch.cat((W1, Wp), 0), Y2.grad)
    for t in (dhid, dP, da, dah):
        assert not t[~valid].any()


def test_importance_closed_form_matches_autograd_without_lstm():
    """lstm = false (reference model/paths.py:95-109): Z = alpha X, so dalpha = dZ . X; importance_rows_bwd_ref's dh, da, dah against
    autograd, with dZ garbage on the padded rows (they must not matter)."""
    g = torch.Generator().manual_seed(7)
    D, Hi = 64, 36
    M = len(NUM_IMS) * N
    valid = R.valid_rows(NUM_IMS, N)
    X, W1, b1, w2, b2, _ = _importance_forward(g, M, D, Hi, 8, valid)
    pre1 = (X @ W1.t() + b1).requires_grad_(True)
    w2r = w2.expand(M, Hi).clone().requires_grad_(True)
    b2r = b2.expand(M).clone().requires_grad_(True)
    hid = torch.relu(pre1)
    alpha = torch.where(valid, torch.sigmoid((hid * w2r).sum(1) + b2r), 0.0)
    dZ = _u(g, M, D)
    (alpha[:, None] * X * dZ).sum().backward()
    dZ_garbage = torch.where(valid[:, None], dZ, 1e6)
    dh, da, dah, _ = R.importance_rows_bwd_ref(dZ_garbage, X, hid.detach(), alpha.detach(), w2, valid)
    assert close(dh, pre1.grad) and close(da, b2r.grad) and close(dah, w2r.grad)
    for t in (dh, da, dah):
        assert not t[~valid].any()


@pytest.mark.parametrize("d", [36, 128, 1540])
@pytest.mark.parametrize("with_add", [False, True])
def test_layernorm_closed_forms_match_f_layer_norm(d, with_add):
    """ln_fwd_ref against F.layer_norm (eps 1e-5); ln_bwd_ref's dx, dgamma, dbeta against autograd, from the saved xhat / rstd; the
    slab sums are column sums of dx, dy xhat and dy.  gamma has zero entries."""
    g = torch.Generator().manual_seed(d + with_add)
    rows = 7
    x = (_u(g, rows, d) * 2 + 0.5).requires_grad_(True)
    add = _u(g, d) if with_add else None
    gamma = _u(g, d).requires_grad_(True)
    with torch.no_grad():
        gamma[::7] = 0
    beta = _u(g, d).requires_grad_(True)
    y = F.layer_norm(x + (add if with_add else 0), (d,), gamma, beta, 1e-5)
    dy = _u(g, rows, d)
    (y * dy).sum().backward()
    y_ref, xh, rs = R.ln_fwd_ref(x.detach(), add, gamma.detach(), beta.detach())
    assert close(y_ref, y.detach(), 1e-12)
    o = R.ln_bwd_ref(dy, xh, rs, gamma.detach())
    assert close(o["dx"], x.grad) and close(o["dgamma"], gamma.grad) and close(o["dbeta"], beta.grad)
    assert close(o["dxsum"], x.grad.sum(0)) and torch.equal(o["dyxhat"], dy * xh)
    assert torch.all(o["dgamma_abs"] >= o["dgamma"].abs()) and torch.all(o["dx_abs"] >= o["dx"].abs())
    assert torch.all(o["dxsum_abs"] >= o["dx"].abs().sum(0))
    # the variance over d - 1 is a different function
    _, xh1, rs1 = R.ln_fwd_ref(x.detach(), add, None, None, ddof=1)
    assert float((rs1 - rs).abs().max() / rs.abs().max()) > 0.1 / d


def test_layernorm_constant_row_has_rstd_of_eps():
    x = torch.full((2, 64), 3.0, dtype=F64)
    _, xh, rs = R.ln_fwd_ref(x, None, None, None)
    assert not xh.any() and torch.allclose(rs, torch.full((2,), 1e-5 ** -0.5, dtype=F64))


def _plumbing_case(seed, B=3, ldk=4, n_cur=9, n_next=20, holes=True):
    """keep_idx / keep_count / child_pos as paths_expand_children writes them: counts 0, ldk - 1 and ldk; child_pos indexed
    blk * count + i; every child row distinct; -1 holes in each of the four blocks."""
    g = torch.Generator().manual_seed(seed)
    counts = [0, ldk - 1, ldk][:B]
    keep_idx = torch.full((B, ldk), -7, dtype=torch.int32)
    child_pos = torch.full((B, 4 * ldk), -9, dtype=torch.int32)
    for b, c in enumerate(counts):
        keep_idx[b, :c] = torch.randperm(n_cur, generator=g)[:c].to(torch.int32)
        pos = torch.randperm(n_next, generator=g)[:4 * c].to(torch.int32)
        if holes and c > 0:
            for blk in range(4):
                pos[blk * c + (blk * 3) % c] = -1
        child_pos[b, :4 * c] = pos
    return keep_idx, torch.tensor(counts, dtype=torch.int32), child_pos


def test_plumbing_references_match_a_python_loop():
    """sibling_sum_ref (with keep_idx and compact), scatter_kept_rows_ref and gather_kept_rows_ref against element loops."""
    B, ldk, n_cur, n_next, W = 3, 4, 9, 20, 8
    keep_idx, kc, cp = _plumbing_case(1, B, ldk, n_cur, n_next)
    g = torch.Generator().manual_seed(2)
    src = torch.rand(B, n_next, W + 4, generator=g)
    sentinel = torch.full((B, n_cur, W + 4), -3.0)
    got = R.sibling_sum_ref(src, cp, kc, ldk, W, sentinel, keep_idx)
    compact = R.sibling_sum_ref(src, cp, kc, ldk, W, torch.full((B, ldk, W + 4), -3.0))
    want = sentinel.clone()
    want_c = torch.full((B, ldk, W + 4), -3.0)
    for b in range(B):
        c = int(kc[b])
        for i in range(c):
            for col in range(W):
                s = torch.tensor(0.0)
                for blk in range(4):
                    p = int(cp[b, blk * c + i])
                    if p >= 0:
                        s = s + src[b, p, col]
                want[b, int(keep_idx[b, i]), col] = s
                want_c[b, i, col] = s
    assert torch.equal(got, want) and torch.equal(compact, want_c)
    assert int((cp[:, :] == -1).sum()) == 8                 # holes in every block of both non-empty slides
    hk = torch.rand(B, ldk, W, generator=g)
    sc = R.scatter_kept_rows_ref(hk, keep_idx, kc, sentinel, W - 4)
    want = sentinel.clone()
    for b in range(B):
        for i in range(int(kc[b])):
            want[b, int(keep_idx[b, i]), :W - 4] = hk[b, i, :W - 4]
    assert torch.equal(sc, want)
    st = torch.rand(B, n_cur, W + 4, generator=g)
    gk = R.gather_kept_rows_ref(st, keep_idx, kc, ldk, W)
    for b in range(B):
        for i in range(ldk):
            exp = st[b, int(keep_idx[b, i]), :W] if i < int(kc[b]) else torch.zeros(W)
            assert torch.equal(gk[b, i], exp)
