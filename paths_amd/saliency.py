"""Gradient patch attributions: gradient x input, integrated gradients and SmoothGrad along the frozen path.

The importance, attention and rollout exports say what the model looked at; :func:`input_gradients` says what moved the prediction:
the gradient of a slide's score with respect to every visited patch's feature vector, reduced per patch to

    grad_x_input[r] = sum_d dX[r,d] X[r,d]          grad_norm[r] = sqrt(sum_d dX[r,d]^2)

The pass is the training recursion (utils.recurse_train) with dropout off and the parameters detached: the hand-written backward
carries dG and dY through every level anyway and forms dX = dG W_gates[:, :D] + dY on top (backward.selection_backward ``want_dx``);
no weight-gradient product runs (backward.no_weight_grads) and no parameter's ``.grad`` is touched.  The per-patch reductions are
one launch per level (csrc/saliency_rows.hip).  The top-K selection is not differentiable: the gradient is that of the score along
the path the model took.  lstm = false is not covered.

:func:`integrated_gradients` and :func:`smooth_grad` go beyond the one point: once a pass has been made its path is known (every
level's keep_idx / keep_count, and with them every level's locations, parents and tissue filter), and with the top-K held at that
recorded result (utils.recurse_train ``path``) the model is an ordinary differentiable function of the visited rows.  Every point of
either method visits the same patches, so their maps can be summed; the S points of one slide run as virtual slides that share the
path, ``chunk`` at a time through the level kernels.  The points are built and the gradients folded by the two row kernels of
csrc/path_rows.hip.  These are attributions of the function along the path taken - not of the selection itself.
"""
from __future__ import annotations

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


def saliency_rows(dx: torch.Tensor, x: torch.Tensor, num_ims: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad_x_input [B,N], grad_norm [B,N]) of dx / x [B,N,D] fp32 (rows may be strided; rows at or beyond num_ims[b]: exact zeros)."""
    _lib.require_cuda(dx, x, num_ims)
    B, N, D = dx.shape
    assert x.shape == dx.shape and dx.dtype == x.dtype == torch.float32 and num_ims.dtype == torch.int64 and num_ims.shape == (B,)
    for t in (dx, x):
        assert t.stride(2) == 1 and t.stride(0) == N * t.stride(1), "rows must be evenly strided"
    gxi = torch.empty((B, N), device=dx.device, dtype=torch.float32)
    gnorm = torch.empty((B, N), device=dx.device, dtype=torch.float32)
    p = _lib.ptr
    _lib.call("paths_saliency_rows", p(dx), dx.stride(1), p(x), x.stride(1), p(num_ims.contiguous()), N, D, B, p(gxi), p(gnorm), _lib.stream())
    return gxi, gnorm


def _pass(model, batch, keep_patches, num_levels, fn, keep_gradients: bool, careful: bool, keep_rows: bool = False):
    from . import utils as putils
    trace: List[dict] = []
    out = putils.recurse_train(model, batch, keep_patches, num_levels, careful=careful, trace=trace)
    tgt = fn(out["logits"])
    if tgt.shape != (out["logits"].shape[0],):
        raise ValueError(f"the target must map logits [B,C] to [B]; got {tuple(tgt.shape)}")
    # slides do not interact: the gradient of the batch sum is every slide's own gradient
    grads = torch.autograd.grad(tgt.sum(), [rec["fts"] for rec in trace])
    for rec, dx in zip(trace, grads):
        rec["grad_x_input"], rec["grad_norm"] = saliency_rows(dx, rec["fts"] if keep_rows else rec.pop("fts"), rec["num_ims"])
        if keep_gradients:
            rec["grad"] = dx
    return {"logits": out["logits"].detach(), "target": tgt.detach(), "status": out["status"]}, trace


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
    if not model.use_lstm:
        raise NotImplementedError("input_gradients: feature gradients are not implemented for the lstm=false variant "
                                  "(selection_backward_nolstm)")
    fn = parse_target(target)
    batch = putils._stored_batch(slides, "input_gradients")
    was_training = model.training
    model.eval()
    try:
        with torch.enable_grad():
            out, trace = _pass(model, batch, keep_patches, num_levels, fn, keep_gradients, careful=False)
            if putils.check_status_word(out["status"]):
                out, trace = _pass(model, batch, keep_patches, num_levels, fn, keep_gradients, careful=True)
                putils.check_status_word(out["status"], fallback_done=True)
    finally:
        model.train(was_training)
    return out, trace


# ------------------------------------------------------------------------------------------------
# integrated gradients and SmoothGrad along the frozen path
# ------------------------------------------------------------------------------------------------
def _rows_ok(t: torch.Tensor, N: int):
    assert t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(0) == N * t.stride(1), "rows must be fp32 and evenly strided"


def path_points(x: torch.Tensor, base: Optional[torch.Tensor], alpha: torch.Tensor, sigma: torch.Tensor, keys: Optional[torch.Tensor],
                num_ims: torch.Tensor) -> torch.Tensor:
    """The points of C chunk members for B slides (include/paths_hip.h: paths_path_points): x [B,N,D] fp32 (rows may be strided),
    base [D] or None, alpha / sigma [C] fp32 device tables, keys [C*B] (or [C,B]) int64 device table (None: every sigma is 0),
    num_ims [B] int64.  Returns [C*B, N, D], virtual slide c * B + b; rows at or beyond num_ims[b] are exact zeros."""
    _lib.require_cuda(x, base, alpha, sigma, keys, num_ims)
    B, N, D = x.shape
    C = alpha.numel()
    _rows_ok(x, N)
    assert alpha.dtype == sigma.dtype == torch.float32 and sigma.numel() == C and alpha.is_contiguous() and sigma.is_contiguous()
    assert num_ims.dtype == torch.int64 and num_ims.shape == (B,)
    assert base is None or (base.shape == (D,) and base.dtype == torch.float32 and base.is_contiguous())
    assert keys is None or (keys.dtype == torch.int64 and keys.numel() == C * B and keys.is_contiguous())
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
    B, N, D = x.shape
    C = w.numel()
    assert dx.shape == (C * B, N, D) and w.dtype == torch.float32 and w.is_contiguous()
    _rows_ok(x, N)
    _rows_ok(dx, N)
    assert num_ims.dtype == torch.int64 and num_ims.shape == (B,)
    assert base is None or (base.shape == (D,) and base.dtype == torch.float32 and base.is_contiguous())
    for a in (acc_gxi, acc_sq):
        assert a.shape == (B, N) and a.dtype == torch.float32 and a.is_contiguous()
    assert acc_dx is None or (acc_dx.shape == (B, N, D) and acc_dx.dtype == torch.float32 and acc_dx.is_contiguous())
    p = _lib.ptr
    _lib.call("paths_path_accumulate", p(dx), dx.stride(1), p(x), x.stride(1), p(base), p(w), p(num_ims.contiguous()), N, D, B, C,
              1 if init else 0, p(acc_gxi), p(acc_sq), p(acc_dx), _lib.stream())


def quadrature(rule: str, steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """(nodes alpha_s in (0, 1), weights w_s) in float64 of the rule over [0, 1]: ``"midpoint"`` (alpha_s = (s + 1/2) / S, w = 1 / S) or
    ``"gausslegendre"`` (numpy's leggauss mapped from [-1, 1]; exact for polynomials in alpha up to degree 2 S - 1)."""
    if not isinstance(steps, int) or steps < 1:
        raise ValueError(f"steps must be a positive integer, got {steps!r}")
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


def _along_path(model, slides, keep_patches, num_levels, fn, what, alphas, sigmas, weights, baseline, seed, chunk, want_dx, want_points,
                want_baseline_target):
    """The shared sequence of both methods: the path pass (today's input_gradients pass, its rows kept), its careful repeat when a
    slide had no tissue children, then ceil(S / chunk) frozen passes of B * chunk virtual slides, each one autograd.grad of the
    summed target with respect to the level leaves and one paths_path_accumulate per level.  Returns (out, trace, per-level
    (acc_gxi, acc_sq, acc_dx or None), per-level points [S,B,N,D] or None)."""
    from . import ops, utils as putils
    from .data_utils.slide import DeviceSlideBatch
    batch = putils._stored_batch(slides, what)
    B, D, dev, S = len(batch), batch.dim, batch.device, len(alphas)
    if chunk is None:
        chunk = max(1, 8 // B)
    if not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"chunk must be a positive integer, got {chunk!r}")
    base = None
    if baseline is not None:
        if baseline.shape != (D,):
            raise ValueError(f"baseline must be None or a [{D}] tensor, got {tuple(baseline.shape)}")
        base = baseline.detach().to(device=dev, dtype=torch.float32).contiguous()
    was_training = model.training
    model.eval()
    guard = None
    try:
        with torch.enable_grad():
            careful = False
            out, trace = _pass(model, batch, keep_patches, num_levels, fn, False, careful=False, keep_rows=True)
            if putils.check_status_word(out["status"]):
                careful = True
                out, trace = _pass(model, batch, keep_patches, num_levels, fn, False, careful=True, keep_rows=True)
                putils.check_status_word(out["status"], fallback_done=True)
            xs = [rec.pop("fts").detach() for rec in trace]
            nums = [rec["num_ims"] for rec in trace]
            path = [(rec["keep_idx"], rec["keep_count"]) for rec in trace[:-1]]
            f32 = dict(device=dev, dtype=torch.float32)
            # ONE upload per call: nodes, noise scales and weights of all S members, and the keys of every (level, sample, slide)
            tab = torch.tensor(np.stack([alphas, sigmas, weights]), **f32)
            noisy = bool(np.any(np.asarray(sigmas) != 0))
            keys = None
            if noisy:
                k = np.array([[[noise_key(seed, l, s, b) for b in range(B)] for s in range(S)] for l in range(num_levels)], dtype=np.uint64)
                keys = torch.from_numpy(k.view(np.int64)).to(dev)
            accs = [(torch.empty(x.shape[:2], **f32), torch.empty(x.shape[:2], **f32), torch.empty(x.shape, **f32) if want_dx else None)
                    for x in xs]
            pts = [[] for _ in xs] if want_points else None
            virtual = {}                                       # chunk size -> (the batch repeated, the path repeated)
            statuses = []

            def frozen(c, alpha, sigma, key_of, grad):
                """One pass of B * c virtual slides along the path, their rows built by paths_path_points from alpha / sigma [c]."""
                if c not in virtual:
                    virtual[c] = (batch if c == 1 else DeviceSlideBatch(list(batch.slides) * c),
                                  [(ki.repeat(c, 1), kc.repeat(c)) for ki, kc in path])
                vb, vpath = virtual[c]
                t2 = [] if grad else None
                o = putils.recurse_train(model, vb, keep_patches, num_levels, careful=careful, trace=t2, path=vpath,
                                         points=lambda level, fts, num_ims: path_points(xs[level], base, alpha, sigma, key_of(level), nums[level]))
                statuses.append(o["status"])
                return o, t2

            # the range contract (ops.range_guard) for what the points can reach: a convex combination stays within max(max|x|, max|base|),
            # a noisy copy within max|x| (1 + 5.89 sigma) (rms <= max|x|, |z| <= 5.89)
            reach = max(batch.feat_absmax * (1.0 + 5.89 * float(np.max(np.abs(sigmas)))), float(base.abs().max()) if base is not None else 0.0)
            guard = ops.range_guard(reach)
            guard.__enter__()
            for s0 in range(0, S, chunk):
                c = min(chunk, S - s0)
                o, t2 = frozen(c, tab[0, s0:s0 + c], tab[1, s0:s0 + c], lambda level: keys[level, s0:s0 + c] if noisy else None, True)
                # virtual slides do not interact either: the gradient of the sum is every member's own gradient
                grads = torch.autograd.grad(fn(o["logits"]).sum(), [rec["fts"] for rec in t2])
                for l, dx in enumerate(grads):
                    path_accumulate(dx, xs[l], base, tab[2, s0:s0 + c], nums[l], s0 == 0, *accs[l])
                    if want_points:
                        pts[l].append(t2[l]["fts"].detach().view(c, B, *xs[l].shape[1:]))
                del o, t2, grads
            if want_baseline_target:
                with torch.no_grad():
                    zero = torch.zeros((1,), **f32)
                    o, _ = frozen(1, zero, zero, lambda level: None, False)
                    out["target_baseline"] = fn(o["logits"]).detach()
            for st in statuses:                                # bit 0 repeats what the careful path pass already handled
                putils.check_status_word(st, fallback_done=True)
    finally:
        if guard is not None:
            guard.__exit__(None, None, None)
        model.train(was_training)
    return out, trace, accs, ([torch.cat(p) for p in pts] if want_points else None)


def _check_model(model, what: str):
    if not model.use_lstm:
        raise NotImplementedError(f"{what}: feature gradients are not implemented for the lstm=false variant "
                                  "(selection_backward_nolstm)")


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
    _check_model(model, "integrated_gradients")
    fn = parse_target(target)
    alphas, weights = quadrature(rule, steps)
    if baseline is not None and not (torch.is_tensor(baseline) and baseline.dim() == 1):
        raise ValueError("baseline must be None or a [D] tensor, got "
                         + (str(tuple(baseline.shape)) if torch.is_tensor(baseline) else repr(type(baseline))))
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
    _check_model(model, "smooth_grad")
    fn = parse_target(target)
    if not isinstance(samples, int) or samples < 1:
        raise ValueError(f"samples must be a positive integer, got {samples!r}")
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
