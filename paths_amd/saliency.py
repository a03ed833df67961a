"""Gradient patch attributions: gradient x input, integrated gradients and SmoothGrad along the frozen path,
the gradient-weighted attention relevance of the special token, and the deletion / insertion curves that tell which
per-patch map is faithful.

The importance, attention and rollout exports say what the model looked at; :func:`input_gradients` says what moved the prediction:
the gradient of a slide's score with respect to every visited patch's feature vector, reduced per patch to

    grad_x_input[r] = sum_d dX[r,d] X[r,d]          grad_norm[r] = sqrt(sum_d dX[r,d]^2)

The pass is the training recursion (utils.recurse_train) with dropout off and the parameters detached: the hand-written backward
carries dG and dY through every level anyway and forms dX = dG W_gates[:, :D] + dY on top (backward.selection_backward ``want_dx``);
no weight-gradient product runs (backward.no_weight_grads) and no parameter's ``.grad`` is touched.  The per-patch reductions are
one launch per level (paths_saliency_rows).  The top-K selection is not differentiable: the gradient is that of the score along
the path the model took.  lstm = false is not covered.

:func:`integrated_gradients` and :func:`smooth_grad` go beyond the one point: once a pass has been made its path is known (every
level's keep_idx / keep_count, and with them every level's locations, parents and tissue filter), and with the top-K held at that
recorded result (utils.recurse_train ``path``) the model is an ordinary differentiable function of the visited rows.  Every point of
either method visits the same patches, so their maps can be summed; the S points of one slide run as virtual slides that share the
path, ``chunk`` at a time through the level kernels.  The points are built and the gradients folded by two more row kernels
(paths_path_points, paths_path_accumulate).  These are attributions of the function along the path taken - not of the selection itself.

:func:`perturbation_curves` judges a map - any of the above, importance, attention, rollout - on the same frozen path: the visited
patches are ranked jointly over the levels (paths_rank_joint, csrc/perturb_rows.hip) and removed from, or restored to, the rows in
that order (paths_path_mask_points), one no-grad forward along the path per point.
The four per-row kernels share csrc/path_rows.hip; every call along a frozen path is one :class:`_FrozenPath`.

:func:`removal_curves` leaves the frozen path: the ranked patches are turned to BACKGROUND - masked views of the slides
(DeviceSlide.with_masks; paths_removal_masks, csrc/perturb_rows.hip), no row is touched - and every point is an ordinary free pass
in which the top-K reacts; paths_visited_overlap says how far its path moved.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

Target = Union[str, Callable[[torch.Tensor], torch.Tensor]]


def risk_score(logits: torch.Tensor) -> torch.Tensor:
    """The reference's risk score (eval.py:60-61): -sum_k S_k with the survival curve S = cumprod(1 - sigmoid(logits)).  [B,C] -> [B]."""
    return -torch.cumprod(1 - torch.sigmoid(logits), dim=1).sum(dim=1)


def parse_target(target: Target) -> Callable[[torch.Tensor], torch.Tensor]:
    """``"risk"`` | ``"logit:<k>"`` | a callable [B,C] -> [B]: the function of the last level's logits that is differentiated."""
    if callable(target):
        return target
    if target == "risk":
        return risk_score
    if isinstance(target, str) and target.startswith("logit:"):
        try:
            k = int(target[len("logit:"):])
        except ValueError:
            raise ValueError(f"target {target!r}: the class index after 'logit:' must be an integer") from None

        def one_logit(logits, k=k):
            if not -logits.shape[1] <= k < logits.shape[1]:
                raise ValueError(f"target 'logit:{k}': the model has {logits.shape[1]} logits")
            return logits[:, k]
        return one_logit
    raise ValueError(f"unknown target {target!r}: 'risk', 'logit:<k>' or a callable [B,C] -> [B]")


# ---- argument checks shared by the entry points (all before anything touches the device)
def _positive_int(name: str, value):
    if not isinstance(value, int) or value < 1:
        raise ValueError(f"{name} must be a positive integer, got {value!r}")


def _require_lstm(model, what: str):
    if not model.use_lstm:
        raise NotImplementedError(f"{what}: feature gradients are not implemented for the lstm=false variant "
                                  "(selection_backward_nolstm)")


def _baseline_arg(baseline, batch=None) -> Optional[torch.Tensor]:
    """``baseline`` is None (zeros) or one [D] tensor; once the batch is known, D is the batch's and the result is that vector as a
    contiguous fp32 device tensor."""
    if baseline is None:
        return None
    if not (torch.is_tensor(baseline) and baseline.dim() == 1 and (batch is None or baseline.shape[0] == batch.dim)):
        raise ValueError(f"baseline must be None or a [{'D' if batch is None else batch.dim}] tensor, got "
                         + (str(tuple(baseline.shape)) if torch.is_tensor(baseline) else repr(type(baseline))))
    return None if batch is None else baseline.detach().to(device=batch.device, dtype=torch.float32).contiguous()


def _target_of(fn, logits: torch.Tensor) -> torch.Tensor:
    tgt = fn(logits)
    if tgt.shape != (logits.shape[0],):
        raise ValueError(f"the target must map logits [B,C] to [B]; got {tuple(tgt.shape)}")
    return tgt


# ---- operand assertions shared by the ctypes wrappers of the per-row kernels
def _rows_ok(x: torch.Tensor, *rows: torch.Tensor, num_ims: torch.Tensor, base: Optional[torch.Tensor] = None):
    """x [B,N,D] and the other ``rows`` (each [k*B,N,D]): fp32, evenly strided; num_ims int64 [B]; base None or fp32 [D] contiguous."""
    B, N, D = x.shape
    for t in (x,) + rows:
        assert t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(0) == N * t.stride(1), "rows must be fp32 and evenly strided"
    assert num_ims.dtype == torch.int64 and num_ims.shape == (B,)
    assert base is None or (base.shape == (D,) and base.dtype == torch.float32 and base.is_contiguous())
    return B, N, D


def _tables_ok(dtype, *tables: Optional[torch.Tensor]):
    assert all(t is None or (t.dtype == dtype and t.is_contiguous()) for t in tables), "device tables must be contiguous"


def saliency_rows(dx: torch.Tensor, x: torch.Tensor, num_ims: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad_x_input [B,N], grad_norm [B,N]) of dx / x [B,N,D] fp32 (rows may be strided; rows at or beyond num_ims[b]: exact zeros)."""
    _lib.require_cuda(dx, x, num_ims)
    B, N, D = _rows_ok(x, dx, num_ims=num_ims)
    assert x.shape == dx.shape
    gxi = torch.empty((B, N), device=dx.device, dtype=torch.float32)
    gnorm = torch.empty((B, N), device=dx.device, dtype=torch.float32)
    p = _lib.ptr
    _lib.call("paths_saliency_rows", p(dx), dx.stride(1), p(x), x.stride(1), p(num_ims.contiguous()), N, D, B, p(gxi), p(gnorm), _lib.stream())
    return gxi, gnorm


def _pass(model, batch, keep_patches, num_levels, fn, keep_gradients: bool, careful: bool, keep_rows: bool = False,
          relevance: bool = False):
    from . import backward as bw, utils as putils
    trace: List[dict] = []
    out = putils.recurse_train(model, batch, keep_patches, num_levels, careful=careful, trace=trace)
    tgt = _target_of(fn, out["logits"])
    # slides do not interact: the gradient of the batch sum is every slide's own gradient
    sink: List[Tuple[torch.Tensor, torch.Tensor]] = []
    with (bw.attention_relevance(sink) if relevance else contextlib.nullcontext()):
        grads = torch.autograd.grad(tgt.sum(), [rec["fts"] for rec in trace])
    if relevance:
        _relevance_records(model, trace, sink)
    for rec, dx in zip(trace, grads):
        rec["grad_x_input"], rec["grad_norm"] = saliency_rows(dx, rec["fts"] if keep_rows else rec.pop("fts"), rec["num_ims"])
        if keep_gradients:
            rec["grad"] = dx
    return {"logits": out["logits"].detach(), "target": tgt.detach(), "status": out["status"]}, trace


def _relevance_records(model, trace: List[dict], sink):
    """``sink``: what the backward appended, the last level first, one pair per level whose aggregator has a path to the target.
    A level without one (non-final levels under slide_ctx_mode "none") gets r = e_s: zeros on the patches, 1 for self."""
    L = len(trace)
    with_agg = [l for l in range(L) if l == L - 1 or model.procs[l].config.slide_ctx_mode != "none"]
    if len(sink) != len(with_agg):
        raise RuntimeError(f"attention_relevance: {len(sink)} levels reported a relevance, {len(with_agg)} have an aggregator gradient")
    got = dict(zip(reversed(with_agg), sink))
    for l, rec in enumerate(trace):
        B, N = rec["importance"].shape
        if l in got:
            rec["attention_relevance"], rec["attention_relevance_self"] = got[l]
            assert rec["attention_relevance"].shape == (B, N) and rec["attention_relevance_self"].shape == (B,)
        else:
            rec["attention_relevance"] = torch.zeros((B, N), device=rec["importance"].device, dtype=torch.float32)
            rec["attention_relevance_self"] = torch.ones((B,), device=rec["importance"].device, dtype=torch.float32)


def _careful_repeat(run):
    """``run(careful)`` makes one pass and returns a tuple that starts with its output dict.  Run it, read the status word, and when a
    slide had no tissue children repeat it on the careful path and check again, as training does.  Returns (the tuple, careful)."""
    from . import utils as putils
    res = run(False)
    if not putils.check_status_word(res[0]["status"]):
        return res, False
    res = run(True)
    putils.check_status_word(res[0]["status"], fallback_done=True)
    return res, True


def input_gradients(model, slides, keep_patches: Sequence[int], num_levels: int, target: Target = "risk",
                    keep_gradients: bool = False) -> Tuple[Dict[str, torch.Tensor], List[dict]]:
    """Gradient of ``target`` (of the last level's logits) with respect to the feature vector of every patch the recursion visits.

    ``slides``: a list of DeviceSlide (fp32 or fp16 grids) or of HostSlide, or a DeviceSlideBatch.  ``target``: ``"risk"`` (the
    reference's risk score, :func:`risk_score`), ``"logit:<k>"`` or a callable [B,C] -> [B].  Returns (out, trace): ``out`` =
    {"logits", "target" [B], "status"}; ``trace`` has one record per level in the format heatmap.hierarchy_from_trace reads (num_ims /
    locs / parent_inds / importance, keep_idx / keep_count below the last level) plus ``grad_x_input`` [B,N] and ``grad_norm`` [B,N]
    (zero on padded rows) and, with ``keep_gradients``, ``grad`` [B,N,D] (valid rows only are meaningful).

    Dropout is off for the call (the model is switched to eval and its mode restored); no parameter's ``.grad`` is created or
    changed.  A slide whose kept patches have no tissue children repeats the pass on the careful path, as training does."""
    from . import utils as putils
    _require_lstm(model, "input_gradients")
    fn = parse_target(target)
    batch = putils._stored_batch(slides, "input_gradients")
    was_training = model.training
    model.eval()
    try:
        with torch.enable_grad():
            (out, trace), _ = _careful_repeat(lambda careful: _pass(model, batch, keep_patches, num_levels, fn, keep_gradients, careful))
    finally:
        model.train(was_training)
    return out, trace


# ------------------------------------------------------------------------------------------------
# gradient-weighted attention relevance of the special token
# ------------------------------------------------------------------------------------------------
def _qkv_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_ims: torch.Tensor):
    """q / k / v [B, H, T, hd] fp32 views (any strides along B / H / T, unit stride along hd, the three alike: head-major tensors or
    the three slices of a token-major qkv): (B, H, T, hd, sb, sh, st)."""
    B, H, T, hd = q.shape
    for t in (q, k, v):
        assert t.dtype == torch.float32 and t.shape == (B, H, T, hd) and t.stride(3) == 1 and t.stride() == q.stride(), \
            "q, k, v must be fp32 [B, H, T, hd] views with the same strides"
    assert hd in (16, 32, 48, 64), "head_dim must be 16, 32, 48 or 64"
    assert num_ims.dtype == torch.int64 and num_ims.shape == (B,) and num_ims.is_contiguous()
    return (B, H, T, hd) + tuple(q.stride()[:3])


def _relevance_outputs(B: int, T: int, outputs: bool, dev):
    if not outputs:
        r = torch.empty((B, T), device=dev, dtype=torch.float32)
        return r, (_lib.ptr(r), None, 0, None)
    rel = torch.empty((B, T - 1), device=dev, dtype=torch.float32)
    rel_self = torch.empty((B,), device=dev, dtype=torch.float32)
    return (rel, rel_self), (None, _lib.ptr(rel) if T > 1 else None, T - 1, _lib.ptr(rel_self))


def relevance_seed(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, qscale: float, da0: torch.Tensor, lse0: torch.Tensor,
                   num_ims: torch.Tensor, outputs: bool = False):
    """The relevance row of the last layer, read at token 0 (include/paths_hip.h: paths_attention_relevance_seed): q / k / v
    [B, H, T, hd] views (:func:`_qkv_ok`), da0 [B, H*hd] (rows may be strided), lse0 [B, H] (any strides; log2 domain), num_ims [B]
    int64.  Returns r [B, T], or with ``outputs`` (relevance [B, T-1], relevance_self [B])."""
    _lib.require_cuda(q, k, v, da0, lse0, num_ims)
    B, H, T, hd, sb, sh, st = _qkv_ok(q, k, v, num_ims)
    assert da0.dtype == torch.float32 and da0.shape == (B, H * hd) and da0.stride(1) == 1
    assert lse0.dtype == torch.float32 and lse0.shape == (B, H)
    res, out_args = _relevance_outputs(B, T, outputs, q.device)
    p = _lib.ptr
    _lib.call("paths_attention_relevance_seed", p(q), p(k), p(v), sb, sh, st, float(qscale), p(da0), da0.stride(0), p(lse0), lse0.stride(0),
              lse0.stride(1), p(num_ims), *out_args, B, T, H, hd, _lib.stream())
    return res


def relevance_step(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, qscale: float, d_o: torch.Tensor, lse: torch.Tensor,
                   num_ims: torch.Tensor, r_in: torch.Tensor, outputs: bool = False):
    """One relevance step through a full layer (include/paths_hip.h: paths_attention_relevance_step): q / k / v as for
    :func:`relevance_seed`, d_o [B, T, ld] fp32 with head h at columns [h*hd, (h+1)*hd) (ld >= H*hd), lse [B, H, T] contiguous (log2
    domain), r_in [B, T] contiguous.  Returns r_out [B, T], or with ``outputs`` (relevance [B, T-1], relevance_self [B])."""
    _lib.require_cuda(q, k, v, d_o, lse, num_ims, r_in)
    B, H, T, hd, sb, sh, st = _qkv_ok(q, k, v, num_ims)
    assert d_o.dtype == torch.float32 and d_o.shape[:2] == (B, T) and d_o.shape[2] >= H * hd and d_o.is_contiguous()
    assert lse.dtype == torch.float32 and lse.shape == (B, H, T) and lse.is_contiguous()
    assert r_in.dtype == torch.float32 and r_in.shape == (B, T) and r_in.is_contiguous()
    res, out_args = _relevance_outputs(B, T, outputs, q.device)
    p = _lib.ptr
    _lib.call("paths_attention_relevance_step", p(q), p(k), p(v), sb, sh, st, float(qscale), p(d_o), d_o.shape[2], p(lse), p(num_ims), p(r_in),
              *out_args, B, T, H, hd, _lib.stream())
    return res


def attention_relevance(model, slides, keep_patches: Sequence[int], num_levels: int,
                        target: Target = "risk") -> Tuple[Dict[str, torch.Tensor], List[dict]]:
    """Gradient-weighted attention relevance of the special token (Chefer, Gur & Wolf 2021) per level: "what the aggregator looked
    at" weighted by "what moved the prediction".

    With A_l^h layer l's attention of head h over a slide's valid tokens and gradA_l^h the gradient of ``target`` with respect to it
    (entry (i, j) = dO_i^h . V_j^h), Abar_l = mean_h (A_l^h * gradA_l^h)^+ and r = e_s^T (I + Abar_{L-1}) ... (I + Abar_0).  The
    pass is :func:`input_gradients`' - same slides, same ``target``, same careful repeat for a slide without tissue children, the
    model's mode restored, no ``.grad`` touched - with the relevance kernels launched from inside the hand-written backward
    (backward.attention_relevance; csrc/attn_relevance.hip) where each layer's q / k / v, lse and output gradient are alive: one
    seed per level plus one T x T step per full decoder layer, no T x T matrix stored.  Earlier levels receive their gradient
    through the slide-context chain as in training; a level whose aggregator has no path to the target (non-final levels under
    slide_ctx_mode "none") gets r = e_s.  FFN, LayerNorms and the degenerate cross-attention are ignored, as in the published
    method.

    Returns (out, trace) as :func:`input_gradients` (``grad_x_input`` / ``grad_norm`` are that function's, bit for bit); the records
    gain ``attention_relevance`` [B, N] (>= 0, in the order of ``importance`` / ``locs``, exactly 0 on padded rows) and
    ``attention_relevance_self`` [B] (>= 1).  Head widths above 64 and the fp8 variants are not covered."""
    from . import backward as bw, ops, utils as putils
    _require_lstm(model, "attention_relevance")
    fn = parse_target(target)
    for proc in list(getattr(model, "procs", ()))[:num_levels]:
        mc = proc.config
        why = bw.relevance_unsupported(ops.padded_head_dim(mc.trans_dim // mc.trans_heads))
        if why:
            raise NotImplementedError(why)
    batch = putils._stored_batch(slides, "attention_relevance")
    was_training = model.training
    model.eval()
    try:
        with torch.enable_grad():
            (out, trace), _ = _careful_repeat(lambda careful: _pass(model, batch, keep_patches, num_levels, fn, False, careful,
                                                                    relevance=True))
    finally:
        model.train(was_training)
    return out, trace


# ------------------------------------------------------------------------------------------------
# integrated gradients and SmoothGrad along the frozen path
# ------------------------------------------------------------------------------------------------
def path_points(x: torch.Tensor, base: Optional[torch.Tensor], alpha: torch.Tensor, sigma: torch.Tensor, keys: Optional[torch.Tensor],
                num_ims: torch.Tensor) -> torch.Tensor:
    """The points of C chunk members for B slides (include/paths_hip.h: paths_path_points): x [B,N,D] fp32 (rows may be strided),
    base [D] or None, alpha / sigma [C] fp32 device tables, keys [C*B] (or [C,B]) int64 device table (None: every sigma is 0),
    num_ims [B] int64.  Returns [C*B, N, D], virtual slide c * B + b; rows at or beyond num_ims[b] are exact zeros."""
    _lib.require_cuda(x, base, alpha, sigma, keys, num_ims)
    B, N, D = _rows_ok(x, num_ims=num_ims, base=base)
    C = alpha.numel()
    _tables_ok(torch.float32, alpha, sigma)
    _tables_ok(torch.int64, keys)
    assert sigma.numel() == C and (keys is None or keys.numel() == C * B)
    out = torch.empty((C * B, N, D), device=x.device, dtype=torch.float32)
    p = _lib.ptr
    _lib.call("paths_path_points", p(x), x.stride(1), p(base), p(alpha), p(sigma), p(keys), p(num_ims.contiguous()), N, D, B, C, p(out),
              _lib.stream())
    return out


def path_accumulate(dx: torch.Tensor, x: torch.Tensor, base: Optional[torch.Tensor], w: torch.Tensor, num_ims: torch.Tensor, init: bool,
                    acc_gxi: torch.Tensor, acc_sq: torch.Tensor, acc_dx: Optional[torch.Tensor] = None):
    """Fold the gradients dx [C*B, N, D] of C chunk members into the running sums acc_gxi / acc_sq [B,N] (and acc_dx [B,N,D]) with the
    weights w [C] (fp32 device table), against the recorded rows x [B,N,D] (include/paths_hip.h: paths_path_accumulate).  In place."""
    _lib.require_cuda(dx, x, base, w, num_ims, acc_gxi, acc_sq, acc_dx)
    B, N, D = _rows_ok(x, dx, num_ims=num_ims, base=base)
    C = w.numel()
    _tables_ok(torch.float32, w, acc_gxi, acc_sq, acc_dx)
    assert dx.shape == (C * B, N, D) and acc_gxi.shape == acc_sq.shape == (B, N) and (acc_dx is None or acc_dx.shape == (B, N, D))
    p = _lib.ptr
    _lib.call("paths_path_accumulate", p(dx), dx.stride(1), p(x), x.stride(1), p(base), p(w), p(num_ims.contiguous()), N, D, B, C,
              1 if init else 0, p(acc_gxi), p(acc_sq), p(acc_dx), _lib.stream())


def quadrature(rule: str, steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """(nodes alpha_s in (0, 1), weights w_s) in float64 of the rule over [0, 1]: ``"midpoint"`` (alpha_s = (s + 1/2) / S, w = 1 / S) or
    ``"gausslegendre"`` (numpy's leggauss mapped from [-1, 1]; exact for polynomials in alpha up to degree 2 S - 1)."""
    _positive_int("steps", steps)
    if rule == "midpoint":
        return (np.arange(steps, dtype=np.float64) + 0.5) / steps, np.full(steps, 1.0 / steps)
    if rule == "gausslegendre":
        t, w = np.polynomial.legendre.leggauss(steps)
        return (t + 1.0) / 2.0, w / 2.0
    raise ValueError(f"unknown rule {rule!r}: 'gausslegendre' or 'midpoint'")


def _fmix32(h: int) -> int:
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def noise_key(seed: int, level: int, sample: int, slide: int) -> int:
    """The 64-bit key (low word key_lo, high word key_hi) of SmoothGrad's draw for (seed, level, sample, slide in the batch): two
    murmur3 finaliser chains over the four numbers, so levels, samples, slides and seeds draw independent noise."""
    s = _fmix32((seed & 0xFFFFFFFF) ^ _fmix32((seed >> 32) + 0x5BD1E995))
    a = _fmix32(s ^ _fmix32(0x9E3779B1 * (level + 1) + sample))
    lo = _fmix32(a + 0x85EBCA77 * (slide + 1))
    hi = _fmix32((lo ^ s) + 0xC2B2AE3D * (sample + 1) + level)
    return lo | (hi << 32)


class _FrozenPath:
    """One call along a frozen path, as a context manager: what integrated_gradients / smooth_grad and perturbation_curves share.

    Entering resolves ``slides``, settles ``chunk`` (members per frozen pass, default max(1, 8 // B)) and ``base`` (the baseline as
    a contiguous fp32 [D] device tensor; None: zeros), switches the model to eval and finds the path: without a ``trace`` it is that
    of the :func:`input_gradients` pass, its rows kept; a given trace's keep_idx / keep_count are the path, and one no-grad pass
    along them must reproduce its num_ims / locs.  Then ``xs`` / ``nums`` hold every level's recorded rows and valid counts,
    ``path`` the selection, ``careful`` whether a slide had no tissue children, ``out`` = {"logits", "target", "status"} and
    ``trace``.  :meth:`frozen` runs inside ops.range_guard(what its rows can reach): a convex combination stays within max(max|x|,
    max|base|), a noisy copy within max|x| (1 + 5.89 sigma) (rms <= max|x|, |z| <= 5.89).  Leaving checks the status words of the
    frozen passes and restores the model's mode - the latter on every way out."""

    def __init__(self, what: str, model, slides, keep_patches, num_levels: int, fn, baseline=None, chunk: Optional[int] = None,
                 trace: Optional[List[dict]] = None, sigma: float = 0.0):
        if chunk is not None:
            _positive_int("chunk", chunk)
        _baseline_arg(baseline)
        self.what, self.model, self.slides, self.keep_patches, self.num_levels, self.fn = what, model, slides, keep_patches, num_levels, fn
        self.baseline, self.chunk, self.trace, self.sigma = baseline, chunk, trace, sigma
        self.statuses: List[torch.Tensor] = []
        self._virtual: dict = {}                               # c -> (the batch repeated c times, the path repeated c times)

    def __enter__(self):
        from . import ops, utils as putils
        batch = self.batch = putils._stored_batch(self.slides, self.what)
        if self.chunk is None:
            self.chunk = max(1, 8 // len(batch))
        base = self.base = _baseline_arg(self.baseline, batch)
        with contextlib.ExitStack() as stack:
            stack.callback(self.model.train, self.model.training)
            self.model.eval()
            given = self.trace is not None
            if not given:                                      # (outside the guard: the free pass keeps the range contract of its own rows)
                with torch.enable_grad():
                    (self.out, self.trace), self.careful = _careful_repeat(
                        lambda careful: _pass(self.model, batch, self.keep_patches, self.num_levels, self.fn, False, careful, keep_rows=True))
                self.xs = [rec.pop("fts").detach() for rec in self.trace]
            stack.enter_context(ops.range_guard(max(batch.feat_absmax * (1.0 + 5.89 * self.sigma),
                                                    float(base.abs().max()) if base is not None else 0.0)))
            self.path = [(rec["keep_idx"], rec["keep_count"]) for rec in self.trace[:-1]]
            self.nums = [rec["num_ims"] for rec in self.trace]
            if given:
                with torch.no_grad():
                    self._along_the_given_trace()
            self._stack = stack.pop_all()
        return self

    def _along_the_given_trace(self):
        """One frozen pass without points collects the rows and F(X), and shows that the trace belongs to these slides."""
        from . import utils as putils

        def run(careful):
            t2: List[dict] = []
            return putils.recurse_train(self.model, self.batch, self.keep_patches, self.num_levels, careful=careful, trace=t2, path=self.path), t2
        (o, t2), self.careful = _careful_repeat(run)
        for l, (rec, r2) in enumerate(zip(self.trace, t2)):
            same = rec["num_ims"].shape == r2["num_ims"].shape and rec["locs"].shape == r2["locs"].shape
            if same:                                           # (the locations of the valid rows: padding is nobody's)
                valid = (torch.arange(r2["locs"].shape[1], device=self.batch.device)[None, :] < r2["num_ims"][:, None])[..., None]
                same = torch.equal(rec["num_ims"], r2["num_ims"]) and torch.equal(rec["locs"] * valid, r2["locs"] * valid)
            if not same:
                raise ValueError(f"trace: a pass along its path does not reproduce its num_ims / locs at level {l}: it belongs to "
                                 "other slides, keep_patches or levels")
        self.xs = [r2["fts"].detach() for r2 in t2]
        self.out = {"logits": o["logits"].detach(), "target": _target_of(self.fn, o["logits"]).detach(), "status": o["status"]}

    def frozen(self, c: int, build_points, trace: Optional[list] = None):
        """One pass of B * c virtual slides (c members of every slide, virtual slide c' * B + b) along the path, the rows of every
        level supplied by ``build_points(level)`` [c*B, N, D].  Returns the pass's output; its records go to ``trace``."""
        from . import utils as putils
        from .data_utils.slide import DeviceSlideBatch
        if c not in self._virtual:
            self._virtual[c] = (self.batch if c == 1 else DeviceSlideBatch(list(self.batch.slides) * c),
                                [(ki.repeat(c, 1), kc.repeat(c)) for ki, kc in self.path])
        vb, vpath = self._virtual[c]
        o = putils.recurse_train(self.model, vb, self.keep_patches, self.num_levels, careful=self.careful, trace=trace, path=vpath,
                                 points=lambda level, fts, num_ims: build_points(level))
        self.statuses.append(o["status"])
        return o

    def __exit__(self, exc_type, exc, tb):
        from . import utils as putils
        with self._stack:                                      # leaves the range guard, restores the model's mode
            if exc_type is None:
                for st in self.statuses:                       # bit 0 repeats what the careful path pass already handled
                    putils.check_status_word(st, fallback_done=True)
        return False


def _along_path(model, slides, keep_patches, num_levels, fn, what, alphas, sigmas, weights, baseline, seed, chunk, want_dx, want_points,
                want_baseline_target):
    """The shared sequence of both methods on a :class:`_FrozenPath`: ceil(S / chunk) frozen passes of B * chunk virtual slides, each
    one autograd.grad of the summed target with respect to the level leaves and one paths_path_accumulate per level.  Returns (out,
    trace, per-level (acc_gxi, acc_sq, acc_dx or None), per-level points [S,B,N,D] or None)."""
    S = len(alphas)
    with _FrozenPath(what, model, slides, keep_patches, num_levels, fn, baseline, chunk, sigma=float(np.max(np.abs(sigmas)))) as fp, \
            torch.enable_grad():
        B, xs, out = len(fp.batch), fp.xs, fp.out
        f32 = dict(device=fp.batch.device, dtype=torch.float32)
        # ONE upload per call: nodes, noise scales and weights of all S members, and the keys of every (level, sample, slide)
        tab = torch.tensor(np.stack([alphas, sigmas, weights]), **f32)
        keys = None
        if np.any(np.asarray(sigmas) != 0):
            k = np.array([[[noise_key(seed, l, s, b) for b in range(B)] for s in range(S)] for l in range(num_levels)], dtype=np.uint64)
            keys = torch.from_numpy(k.view(np.int64)).to(fp.batch.device)
        accs = [(torch.empty(x.shape[:2], **f32), torch.empty(x.shape[:2], **f32), torch.empty(x.shape, **f32) if want_dx else None)
                for x in xs]
        pts = [[] for _ in xs] if want_points else None

        def points(s0, c):                                     # the rows of members s0 .. s0 + c - 1
            return lambda level: path_points(xs[level], fp.base, tab[0, s0:s0 + c], tab[1, s0:s0 + c],
                                             None if keys is None else keys[level, s0:s0 + c], fp.nums[level])

        for s0 in range(0, S, fp.chunk):
            c, t2 = min(fp.chunk, S - s0), []
            o = fp.frozen(c, points(s0, c), trace=t2)
            # virtual slides do not interact either: the gradient of the sum is every member's own gradient
            grads = torch.autograd.grad(fn(o["logits"]).sum(), [rec["fts"] for rec in t2])
            for l, dx in enumerate(grads):
                path_accumulate(dx, xs[l], fp.base, tab[2, s0:s0 + c], fp.nums[l], s0 == 0, *accs[l])
                if want_points:
                    pts[l].append(t2[l]["fts"].detach().view(c, B, *xs[l].shape[1:]))
            del o, t2, grads
        if want_baseline_target:
            with torch.no_grad():
                zero = torch.zeros((1,), **f32)
                out["target_baseline"] = fn(fp.frozen(1, lambda level: path_points(xs[level], fp.base, zero, zero, None, fp.nums[level]))
                                            ["logits"]).detach()
    return out, fp.trace, accs, ([torch.cat(p) for p in pts] if want_points else None)


def integrated_gradients(model, slides, keep_patches: Sequence[int], num_levels: int, target: Target = "risk", steps: int = 32,
                         baseline: Optional[torch.Tensor] = None, rule: str = "gausslegendre", chunk: Optional[int] = None,
                         keep_gradients: bool = False) -> Tuple[Dict[str, torch.Tensor], List[dict]]:
    """Integrated gradients (Sundararajan et al. 2017) of ``target`` over every patch the recursion visits, along the frozen path.

    A first pass (exactly :func:`input_gradients`': the records also carry ``grad_x_input`` / ``grad_norm``) fixes the path; the
    ``steps`` points baseline + alpha_s (X - baseline) of ``rule`` (:func:`quadrature`) then run along it as virtual slides, ``chunk``
    members at a time (default max(1, 8 // B); the last chunk may be short).  ``baseline``: None (zeros) or a [D] tensor, the same for
    every patch.  Records gain ``integrated_gradients`` [B,N] = sum_s w_s sum_d dX_s (X - baseline) (zero on padded rows) and, with
    ``keep_gradients``, ``integrated_gradient`` [B,N,D] = sum_s w_s dX_s.  ``out`` gains ``target_baseline`` [B] (one no-grad forward
    along the path at alpha = 0) and ``completeness_gap`` [B] = the sum of integrated_gradients over all levels and rows minus
    (target - target_baseline): the quadrature error plus rounding.

    This is the attribution of the function along the path the model took, not of the selection.  Dropout is off, the model's mode is
    restored, no weight-gradient product runs and no ``.grad`` is touched; slides as for :func:`input_gradients`."""
    _require_lstm(model, "integrated_gradients")
    fn = parse_target(target)
    alphas, weights = quadrature(rule, steps)
    out, trace, accs, _ = _along_path(model, slides, keep_patches, num_levels, fn, "integrated_gradients", alphas, np.zeros(steps), weights,
                                      baseline, 0, chunk, keep_gradients, False, True)
    total = None
    for rec, (gxi, _, adx) in zip(trace, accs):
        rec["integrated_gradients"] = gxi
        if keep_gradients:
            rec["integrated_gradient"] = adx
        s = gxi.double().sum(dim=1)
        total = s if total is None else total + s
    out["completeness_gap"] = (total - (out["target"].double() - out["target_baseline"].double())).float()
    return out, trace


def smooth_grad(model, slides, keep_patches: Sequence[int], num_levels: int, target: Target = "risk", samples: int = 16,
                sigma: float = 0.15, seed: int = 0, chunk: Optional[int] = None, keep_gradients: bool = False,
                keep_points: bool = False) -> Tuple[Dict[str, torch.Tensor], List[dict]]:
    """SmoothGrad (Smilkov et al. 2017) of ``target`` over every patch the recursion visits, along the frozen path.

    A first pass (exactly :func:`input_gradients`') fixes the path; ``samples`` noisy copies X + sigma rms(X_r) z of every visited
    row (z standard normal, counter-based on (:func:`noise_key` (seed, level, sample, slide), element): nothing is stored and a
    repeat with the same seed gives the same bits) then run along it as virtual slides, ``chunk`` at a time.  The noise does not
    change the path.  Records gain ``smooth_grad_x_input`` [B,N], the mean over samples of sum_d dX_s X, and ``smooth_grad_sq``
    [B,N], the mean of ||dX_s||^2 (SmoothGrad-squared); ``keep_gradients`` adds ``smooth_grad`` [B,N,D], the mean gradient;
    ``keep_points`` adds ``points`` [S,B,N,D], the noisy rows themselves - S copies of every level: for tests and small slides.
    Everything else as :func:`integrated_gradients`."""
    _require_lstm(model, "smooth_grad")
    fn = parse_target(target)
    _positive_int("samples", samples)
    if not sigma >= 0:
        raise ValueError(f"sigma must not be negative, got {sigma!r}")
    out, trace, accs, pts = _along_path(model, slides, keep_patches, num_levels, fn, "smooth_grad", np.ones(samples),
                                        np.full(samples, float(sigma)), np.full(samples, 1.0 / samples), None, int(seed), chunk,
                                        keep_gradients, keep_points, False)
    for l, (rec, (gxi, sq, adx)) in enumerate(zip(trace, accs)):
        rec["smooth_grad_x_input"], rec["smooth_grad_sq"] = gxi, sq
        if keep_gradients:
            rec["smooth_grad"] = adx
        if keep_points:
            rec["points"] = pts[l]
    return out, trace


# ------------------------------------------------------------------------------------------------
# deletion and insertion curves along the frozen path
# ------------------------------------------------------------------------------------------------
MODES = ("deletion", "insertion", "both")


def rank_joint_tile() -> int:
    """Keys per LDS tile of paths_rank_joint (csrc/perturb_rows.hip: RJ_TILE)."""
    return int(_lib.load().paths_rank_joint_tile())


def rank_joint(scores: torch.Tensor, seg_end: torch.Tensor, level_on: torch.Tensor, num_ims: torch.Tensor,
               ascending: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rank [B, Ntot] int32, count [B] int32) of scores [B, Ntot] fp32 (the levels' capacities end to end), jointly over the chosen
    levels (include/paths_hip.h: paths_rank_joint): seg_end / level_on [L] int32 device tables, num_ims [L, B] int64.  -1 on padded
    rows and on levels that are not chosen; their scores are not read."""
    _lib.require_cuda(scores, seg_end, level_on, num_ims)
    B, Ntot = scores.shape
    L = seg_end.numel()
    _tables_ok(torch.float32, scores)
    _tables_ok(torch.int32, seg_end, level_on)
    _tables_ok(torch.int64, num_ims)
    assert level_on.numel() == L and num_ims.shape == (L, B)
    rank = torch.empty((B, Ntot), device=scores.device, dtype=torch.int32)
    count = torch.empty((B,), device=scores.device, dtype=torch.int32)
    p = _lib.ptr
    _lib.call("paths_rank_joint", p(scores), p(seg_end), p(level_on), p(num_ims), L, B, Ntot, 1 if ascending else 0, p(rank), p(count),
              _lib.stream())
    return rank, count


def path_mask_points(x: torch.Tensor, base: Optional[torch.Tensor], rank: torch.Tensor, thr: torch.Tensor, insert: torch.Tensor,
                     num_ims: torch.Tensor) -> torch.Tensor:
    """The rows of C chunk members for B slides (include/paths_hip.h: paths_path_mask_points): x [B,N,D] fp32 (rows may be strided),
    base [D] or None, rank [B,N] int32 (a level's slice of the joint rank: the slide stride is free), thr [C,B] / insert [C] int32
    device tables, num_ims [B] int64.  Returns [C*B, N, D], virtual slide c * B + b: a copy of the row or of the baseline, exact
    zeros at or beyond num_ims[b]."""
    _lib.require_cuda(x, base, rank, thr, insert, num_ims)
    B, N, D = _rows_ok(x, num_ims=num_ims, base=base)
    C = insert.numel()
    _tables_ok(torch.int32, thr, insert)
    assert rank.dtype == torch.int32 and rank.shape == (B, N) and rank.stride(1) == 1 and (B == 1 or rank.stride(0) >= N)
    assert thr.shape == (C, B)
    out = torch.empty((C * B, N, D), device=x.device, dtype=torch.float32)
    p = _lib.ptr
    _lib.call("paths_path_mask_points", p(x), x.stride(1), p(base), p(rank), rank.stride(0) if B > 1 else N, p(thr), p(insert),
              p(num_ims.contiguous()), N, D, B, C, p(out), _lib.stream())
    return out


def perturbation_counts(n: Sequence[int], steps: int) -> np.ndarray:
    """counts [steps + 1, B] int64: the patches removed (inserted) at fraction s / steps of a slide with n_b ranked patches,
    (2 s n_b + steps) // (2 steps) - s n_b / steps rounded half up, so counts[0] = 0 and counts[steps] = n_b."""
    s = np.arange(steps + 1, dtype=np.int64)[:, None]
    return (2 * s * np.asarray(n, dtype=np.int64)[None, :] + steps) // (2 * steps)


def _level_scores(scores, trace, num_levels: int, shapes, dev) -> List[torch.Tensor]:
    """The per-level score tensors [B, N_l] (fp32, on the device) of ``scores``: the name of a trace entry or a sequence of tensors."""
    if isinstance(scores, str):
        missing = [l for l, rec in enumerate(trace) if scores not in rec]
        if missing:
            raise ValueError(f"scores {scores!r}: the trace has no such entry at level(s) {missing}; it has {sorted(trace[missing[0]])}")
        per_level = [rec[scores] for rec in trace]
    else:
        per_level = list(scores)
        if len(per_level) != num_levels:
            raise ValueError(f"scores: one [B, N] tensor per level ({num_levels}) expected, got {len(per_level)}")
    out = []
    for l, (t, shape) in enumerate(zip(per_level, shapes)):
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"scores{'' if not isinstance(scores, str) else ' ' + repr(scores)}: level {l} needs one value per patch, "
                             f"[B, N] = {list(shape)}, got {got}")
        _lib.require_cuda(t)
        out.append(t.detach().to(device=dev, dtype=torch.float32))
    return out


def _rank_levels(fp: _FrozenPath, scores, chosen: Sequence[int], descending: bool, key: str = "perturbation_rank"):
    """The joint rank of the visited patches of the ``chosen`` levels by ``scores`` (one launch), with the call's ONE host check.
    Returns (rank per level [B, N_l] - the records gain it as ``key`` -, the ranked patches per slide [B] on the host)."""
    B, dev = len(fp.batch), fp.batch.device
    Ns = [int(x.shape[1]) for x in fp.xs]
    sc = torch.cat(_level_scores(scores, fp.trace, fp.num_levels, [(B, n) for n in Ns], dev), dim=1).contiguous()
    seg = np.cumsum(Ns)
    seg_tab = torch.tensor(np.stack([seg, [1 if l in chosen else 0 for l in range(fp.num_levels)]]), device=dev, dtype=torch.int32)
    rank, count = rank_joint(sc, seg_tab[0], seg_tab[1], torch.stack(fp.nums), ascending=not descending)
    # ONE host check: the valid counts and whether a valid score is NaN (its rank would mean nothing)
    host = torch.cat([count.long(), (torch.isnan(sc) & (rank >= 0)).any(dim=1).long()]).cpu().numpy()
    if host[B:].any():
        raise ValueError(f"scores: NaN among the valid patches of slide(s) {np.nonzero(host[B:])[0].tolist()}")
    ranks = [rank[:, e - n:e] for e, n in zip(seg, Ns)]
    for rec, rk in zip(fp.trace, ranks):
        rec[key] = rk
    return ranks, host[:B]


def _member_tables(counts: np.ndarray, steps: int, names: Sequence[str], dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """(thr [M, B], insert [M]) int32 of every member, ONE upload per call: [s = 1 .. steps - 1 of each curve in ``names`` | everything
    removed]; the end points are F(X) and F(baseline), shared by both curves."""
    inner, B = counts[1:steps], counts.shape[1]
    thr = np.concatenate([inner] * len(names) + [counts[steps:]])
    ins = np.concatenate([np.full(steps - 1, float(name == "insertion")) for name in names] + [np.zeros(1)])
    tab = torch.tensor(np.concatenate([thr.reshape(-1), ins]), device=dev, dtype=torch.int32)
    return tab[:len(ins) * B].view(len(ins), B), tab[len(ins) * B:]


def _auc(curve: torch.Tensor, frac: np.ndarray) -> torch.Tensor:
    """Trapezoid of curve [B, steps + 1] over frac, in float64."""
    d, w = curve.double(), torch.from_numpy(np.diff(frac)).to(curve.device)
    return ((d[:, :-1] + d[:, 1:]) * 0.5 * w[None, :]).sum(dim=1)


def _chosen_levels(levels, num_levels: int) -> List[int]:
    chosen = list(range(num_levels)) if levels is None else [int(l) for l in levels]
    if any(not 0 <= l < num_levels for l in chosen):
        raise ValueError(f"levels {list(levels)}: level indices must be in [0, {num_levels})")
    return chosen


def _scores_trace_args(scores, trace, num_levels: int):
    if not isinstance(scores, str) and (torch.is_tensor(scores) or not hasattr(scores, "__len__") or len(scores) != num_levels):
        raise ValueError(f"scores: the name of a trace entry or a sequence of {num_levels} tensors [B, N_l] expected")
    if trace is not None and (len(trace) != num_levels or any("keep_idx" not in rec or "keep_count" not in rec for rec in trace[:-1])):
        raise ValueError(f"trace: {num_levels} records with keep_idx / keep_count below the last level expected")


def perturbation_curves(model, slides, keep_patches: Sequence[int], num_levels: int, scores, trace: Optional[List[dict]] = None,
                        target: Target = "risk", steps: int = 16, mode: str = "both", levels: Optional[Sequence[int]] = None,
                        baseline: Optional[torch.Tensor] = None, descending: bool = True,
                        chunk: Optional[int] = None) -> Tuple[Dict[str, torch.Tensor], List[dict]]:
    """Deletion and insertion curves (Petsiuk et al. 2018; Samek et al. 2017) of ``target`` for a per-patch map, along the frozen path.

    The visited patches of the chosen ``levels`` (None: all) are ranked jointly by ``scores`` (most relevant first: highest first with
    ``descending``; ties by level, then row).  The deletion curve replaces the first counts[s] of them by ``baseline`` (None: zeros,
    or one [D] vector) and records the target; the insertion curve starts from the baseline on all of them and restores the first
    counts[s].  fractions[s] = s / steps, counts[s, b] = (2 s n_b + steps) // (2 steps) with n_b the slide's ranked patches.  A
    faithful map has a small ``deletion_auc`` and a large ``insertion_auc``.  The selection is held at the recorded path: every
    point visits the same patches, a removed row is a token with baseline features (not background), and curves of different maps
    over the same path are comparable point by point.

    ``scores``: the name of a [B, N] entry of the trace records, or a sequence of ``num_levels`` device tensors [B, N_l].  ``trace``
    None: the call makes the :func:`input_gradients` pass itself (entries "importance", "grad_x_input", "grad_norm").  ``trace``
    given (from recurse(..., trace=[]), the functions of this module or the model's exports): its keep_idx / keep_count are the path;
    a no-grad pass along it must reproduce its num_ims and locs, else ValueError.  Records gain ``perturbation_rank`` [B, N] int32
    (-1 on padded rows and levels not chosen).

    Returns (out, trace): ``fractions`` [steps + 1] (float64, CPU), ``counts`` [steps + 1, B] (int64, CPU), ``deletion`` /
    ``insertion`` [B, steps + 1] fp32 and ``deletion_auc`` / ``insertion_auc`` [B] float64 (trapezoid over fractions) as ``mode``
    asks, ``target`` = F(X), ``target_baseline`` = F(baseline on the chosen levels), ``status``.  The end points are computed once:
    deletion[:, 0] and insertion[:, steps] are ``target``, deletion[:, steps] and insertion[:, 0] are ``target_baseline``.  The
    points between run as virtual slides, ``chunk`` at a time (default max(1, 8 // B)), each curve's members in chunks of their own
    so that a curve has the same bits whichever ``mode`` asked for it.  No gradient is taken beyond the path pass; dropout is off,
    the model's mode is restored and no ``.grad`` is touched."""
    _require_lstm(model, "perturbation_curves")
    fn = parse_target(target)
    _positive_int("steps", steps)
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r}: 'deletion', 'insertion' or 'both'")
    chosen = _chosen_levels(levels, num_levels)
    fp = _FrozenPath("perturbation_curves", model, slides, keep_patches, num_levels, fn, baseline, chunk, trace)
    _scores_trace_args(scores, trace, num_levels)
    names = [name for name in ("deletion", "insertion") if mode in (name, "both")]
    with fp, torch.no_grad():
        B, out = len(fp.batch), fp.out
        ranks, n = _rank_levels(fp, scores, chosen, descending)
        counts = perturbation_counts(n, steps)
        thr, ins = _member_tables(counts, steps, names, fp.batch.device)

        def targets(m0, c):                                    # [c, B] of members m0 .. m0 + c - 1
            o = fp.frozen(c, lambda level: path_mask_points(fp.xs[level], fp.base, ranks[level], thr[m0:m0 + c], ins[m0:m0 + c], fp.nums[level]))
            return fn(o["logits"]).detach().view(c, B)

        out["target_baseline"] = targets(len(ins) - 1, 1)[0]
        curves = {}
        for k, name in enumerate(names):                       # each curve's members in chunks of their own
            ends = [out["target"][None], out["target_baseline"][None]]
            inner = [targets(k * (steps - 1) + s0, min(fp.chunk, steps - 1 - s0)) for s0 in range(0, steps - 1, fp.chunk)]
            curves[name] = torch.cat(ends[:1] + inner + ends[1:] if name == "deletion" else ends[1:] + inner + ends[:1]).t().contiguous()
    frac = np.arange(steps + 1, dtype=np.float64) / steps
    out["fractions"] = torch.from_numpy(frac)
    out["counts"] = torch.from_numpy(counts)
    for name, cv in curves.items():
        out[name], out[name + "_auc"] = cv, _auc(cv, frac)
    return out, fp.trace


# ------------------------------------------------------------------------------------------------
# removal curves on the free path
# ------------------------------------------------------------------------------------------------
ORDERS = ("morf", "lerf", "both")


def removal_masks(src_ptrs: Optional[torch.Tensor], gx: torch.Tensor, gy: torch.Tensor, max_cells: int, locs: torch.Tensor, patch_size: int,
                  num_ims: torch.Tensor, rank: Optional[torch.Tensor], thr: Optional[torch.Tensor],
                  set_cells: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(masks [C, B, ldm] uint8, left [C, B] int32) of one level (include/paths_hip.h: paths_removal_masks): src_ptrs [B] int64 device
    table of the source masks' addresses (None: all-zero sources), gx / gy [B] int32 device tables, locs [B, N, 2] int64 in pixels,
    num_ims [B] int64, rank [B, N] int32 (a level's slice of the joint rank: the slide stride is free), thr [C, B] int32 device table
    (rank and thr None: C = 1, every valid row is chosen).  ldm = max_cells rounded up to 16; the bytes of a member beyond its
    slide's gx * gy cells are not written."""
    _lib.require_cuda(src_ptrs, gx, gy, locs, num_ims, rank, thr)
    B, N = locs.shape[:2]
    _tables_ok(torch.int64, src_ptrs, locs, num_ims)
    _tables_ok(torch.int32, gx, gy, thr)
    assert locs.shape == (B, N, 2) and num_ims.shape == gx.shape == gy.shape == (B,) and (src_ptrs is None or src_ptrs.shape == (B,))
    assert (rank is None) == (thr is None)
    C, ldr = 1, N
    if rank is not None:
        assert rank.dtype == torch.int32 and rank.shape == (B, N) and rank.stride(1) == 1 and (B == 1 or rank.stride(0) >= N)
        assert thr.dim() == 2 and thr.shape[1] == B
        C, ldr = thr.shape[0], (rank.stride(0) if B > 1 else N)
    ldm = (int(max_cells) + 15) // 16 * 16
    masks = torch.empty((C, B, ldm), device=locs.device, dtype=torch.uint8)
    left = torch.empty((C, B), device=locs.device, dtype=torch.int32)
    p = _lib.ptr
    _lib.call("paths_removal_masks", p(src_ptrs), p(gx), p(gy), int(max_cells), p(locs), int(patch_size), p(num_ims), p(rank), ldr, p(thr), N, B,
              C, 1 if set_cells else 0, p(masks), ldm, p(left), _lib.stream())
    return masks, left


def visited_overlap(bitmap: torch.Tensor, gx: torch.Tensor, gy: torch.Tensor, locs_m: torch.Tensor, num_m: torch.Tensor,
                    patch_size: int) -> torch.Tensor:
    """overlap [C * B] int32 (include/paths_hip.h: paths_visited_overlap): bitmap [B, ldb] uint8 (the recorded cells of this level),
    gx / gy [B] int32 device tables, locs_m [C * B, Nm, 2] int64 in pixels and num_m [C * B] int64 of the members' passes."""
    _lib.require_cuda(bitmap, gx, gy, locs_m, num_m)
    B, ldb = bitmap.shape
    V, Nm = locs_m.shape[:2]
    _tables_ok(torch.uint8, bitmap)
    _tables_ok(torch.int32, gx, gy)
    _tables_ok(torch.int64, locs_m, num_m)
    assert V % B == 0 and locs_m.shape == (V, Nm, 2) and num_m.shape == (V,) and gx.shape == gy.shape == (B,)
    overlap = torch.empty((V,), device=bitmap.device, dtype=torch.int32)
    p = _lib.ptr
    _lib.call("paths_visited_overlap", p(bitmap), ldb, p(gx), p(gy), p(locs_m), p(num_m), int(patch_size), Nm, B, V // B, p(overlap), _lib.stream())
    return overlap


def removal_counts(n: Sequence[int], steps: int, max_fraction: float) -> np.ndarray:
    """counts [steps + 1, B] int64: the cells turned to background at point s of a slide with n_b ranked patches,
    (2 s m_b + steps) // (2 steps) with m_b = floor(max_fraction * n_b) - s m_b / steps rounded half up."""
    m = np.array([int(np.floor(max_fraction * int(nb))) for nb in n], dtype=np.int64)
    return perturbation_counts(m, steps)


def removal_curves(model, slides, keep_patches: Sequence[int], num_levels: int, scores, trace: Optional[List[dict]] = None,
                   target: Target = "risk", steps: int = 8, order: str = "both", max_fraction: float = 0.5,
                   levels: Optional[Sequence[int]] = None, chunk: Optional[int] = None) -> Tuple[Dict[str, torch.Tensor], List[dict]]:
    """Removal curves (Samek et al. 2017) of ``target`` for a per-patch map on the FREE path: removed patches become background and
    the selection reacts.

    The visited patches of the chosen ``levels`` (None: all) are ranked jointly by ``scores`` as for :func:`perturbation_curves` -
    ``order`` "morf": most relevant (highest) first, "lerf": least relevant first, "both".  Point s of a curve is the slide with the
    cells of the counts[s, b] first-ranked patches turned to background, counts[s, b] = (2 s m_b + steps) // (2 steps), m_b =
    floor(max_fraction n_b), fractions[s] = s / steps * max_fraction.  A point is a masked view of the slide (same grids, other tissue
    masks) run through the ordinary no-grad :func:`paths_amd.utils.recurse`: a background cell is dropped by the child filter, its
    subtree is unreachable, the top-K of the remaining patches picks others, and a member whose kept patches have no tissue children
    takes the careful re-run; at level 0, where every cell is loaded, a removed cell reads as the all-zero row of a background cell.
    It is what the model computes on the slide with those rows zeroed.  There is no insertion curve: restoring a patch whose
    ancestors are absent has no meaning here.  A map that ranks what the prediction depends on has a small ``morf_auc`` and a large
    ``lerf_auc``.

    ``scores`` / ``trace`` / ``levels`` / ``target`` as for :func:`perturbation_curves` (``trace`` None: the :func:`input_gradients`
    pass is made; a given trace must be reproduced by a pass along its path); with a given trace the lstm = false variant runs too.
    The records gain ``removal_rank_morf`` / ``removal_rank_lerf`` [B, N] int32.  A member that leaves a slide without level-0 tissue
    raises ValueError before any point runs.

    Returns (out, trace): ``fractions`` [steps + 1] (float64, CPU), ``counts`` [steps + 1, B] (int64, CPU), ``morf`` / ``lerf``
    [B, steps + 1] fp32 with ``morf_auc`` / ``lerf_auc`` [B] float64 (trapezoid over fractions) and, with both, ``aopc_gap`` =
    lerf_auc - morf_auc; ``visited`` / ``path_overlap`` {order: [B, steps + 1, L] int32}: the member's valid rows per level and how
    many of them sit on a cell the recorded pass visited at that level; ``masks`` {order: per level uint8 [steps, B, ldm]}: the
    members' masks (member s + 1 of slide b: the first X * Y bytes of [s, b]); ``logits`` / ``target``: the unperturbed free pass
    (point 0 of both orders, bit for bit); ``status``: the OR of every point's status word.  Points run ``chunk`` members at a time
    (default max(1, 8 // B)), each order in chunks of its own.  Dropout is off, the model's mode is restored, no ``.grad`` is touched."""
    from . import utils as putils
    from .data_utils.slide import DeviceSlideBatch
    fn = parse_target(target)
    _positive_int("steps", steps)
    if order not in ORDERS:
        raise ValueError(f"unknown order {order!r}: 'morf', 'lerf' or 'both'")
    if isinstance(max_fraction, bool) or not isinstance(max_fraction, (int, float)) or not 0 < max_fraction <= 1:
        raise ValueError(f"max_fraction must be in (0, 1], got {max_fraction!r}")
    chosen = _chosen_levels(levels, num_levels)
    if trace is None:
        _require_lstm(model, "removal_curves")
    fp = _FrozenPath("removal_curves", model, slides, keep_patches, num_levels, fn, None, chunk, trace)
    _scores_trace_args(scores, trace, num_levels)
    names = [name for name in ("morf", "lerf") if order in (name, "both")]
    L = num_levels
    with fp, torch.no_grad():
        batch, B, dev = fp.batch, len(fp.batch), fp.batch.device
        ps = model.procs[0].config.patch_size
        shapes = [[s.shape(l) for s in batch.slides] for l in range(L)]
        max_cells = [max(x * y for x, y in sh) for sh in shapes]
        ranks = {}
        for name in names:                                     # one paths_rank_joint (and its host check) per order
            ranks[name], n = _rank_levels(fp, scores, chosen, name == "morf", key="removal_rank_" + name)
        counts = removal_counts(n, steps, float(max_fraction))
        thr = torch.tensor(counts[1:], device=dev, dtype=torch.int32)        # ONE upload: members s = 1 .. steps, the same for both orders
        locs = [rec["locs"].contiguous() for rec in fp.trace]
        masks, left0 = {}, []
        for name in names:                                     # every member's masks, all levels: L launches per order
            built = [removal_masks(batch.mask_ptrs[l], batch.gx[l], batch.gy[l], max_cells[l], locs[l], ps, fp.nums[l], ranks[name][l], thr)
                     for l in range(L)]
            masks[name] = [m for m, _ in built]
            left0.append(built[0][1])
        left = torch.stack(left0).cpu().numpy()                # ONE host read: [orders, steps, B]
        gone = np.argwhere(left <= 0)
        if len(gone):
            k, s, b = (int(v) for v in gone[0])
            raise ValueError(f"removal_curves: order {names[k]!r}, step {s + 1} (of {steps}) leaves slide {b} without level-0 tissue: "
                             f"{int(counts[s + 1, b])} cells removed; lower max_fraction or leave level 0 out of levels")
        bitmaps = [removal_masks(None, batch.gx[l], batch.gy[l], max_cells[l], locs[l], ps, fp.nums[l], None, None, set_cells=True)[0][0]
                   for l in range(L)]                          # the cells the recorded pass visited, per level [B, ldm]

        def run(vb, c):                                        # one free pass of c members of every slide
            t: List[dict] = []
            o = putils.recurse(model, vb, keep_patches, L, trace=t)
            vis = torch.stack([rec["num_ims"] for rec in t], dim=-1).view(c, B, L).to(torch.int32)
            ov = torch.stack([visited_overlap(bitmaps[l], batch.gx[l], batch.gy[l], t[l]["locs"].contiguous(), t[l]["num_ims"], ps)
                              for l in range(L)], dim=-1).view(c, B, L)
            return o, _target_of(fn, o["logits"]).view(c, B), vis, ov

        def member_view(name, s, b):                          # slide b behind member s + 1's masks (levels beyond L keep its own)
            slide = batch.slides[b]
            own = [masks[name][l][s, b, :x * y].view(x, y) for l, (x, y) in enumerate(sh[b] for sh in shapes)]
            return slide.with_masks(own + list(slide.masks[L:]))

        o0, tg0, vis0, ov0 = run(batch, 1)
        out = {"logits": o0["logits"], "target": tg0[0], "status": o0["status"].clone()}
        curves, visited, overlap = {}, {}, {}
        for name in names:                                     # each order's members in chunks of their own
            tgs, vis, ovs = [tg0], [vis0], [ov0]
            for s0 in range(0, steps, fp.chunk):
                c = min(fp.chunk, steps - s0)
                views = [member_view(name, s0 + ci, b) for ci in range(c) for b in range(B)]
                o, tg, vi, ov = run(DeviceSlideBatch(views), c)
                out["status"] |= o["status"]
                tgs.append(tg), vis.append(vi), ovs.append(ov)
            curves[name] = torch.cat(tgs).t().contiguous()
            visited[name] = torch.cat(vis).permute(1, 0, 2).contiguous()
            overlap[name] = torch.cat(ovs).permute(1, 0, 2).contiguous()
    frac = np.arange(steps + 1, dtype=np.float64) / steps * float(max_fraction)
    out["fractions"] = torch.from_numpy(frac)
    out["counts"] = torch.from_numpy(counts)
    for name, cv in curves.items():
        out[name], out[name + "_auc"] = cv, _auc(cv, frac)
    if len(names) == 2:
        out["aopc_gap"] = out["lerf_auc"] - out["morf_auc"]
    out["visited"], out["path_overlap"], out["masks"] = visited, overlap, masks
    return out, fp.trace
