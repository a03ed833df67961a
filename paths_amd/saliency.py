"""Gradient x input patch attributions.

The importance, attention and rollout exports say what the model looked at; :func:`input_gradients` says what moved the prediction:
the gradient of a slide's score with respect to every visited patch's feature vector, reduced per patch to

    grad_x_input[r] = sum_d dX[r,d] X[r,d]          grad_norm[r] = sqrt(sum_d dX[r,d]^2)

The pass is the training recursion (utils.recurse_train) with dropout off and the parameters detached: the hand-written backward
carries dG and dY through every level anyway and forms dX = dG W_gates[:, :D] + dY on top (backward.selection_backward ``want_dx``);
no weight-gradient product runs (backward.no_weight_grads) and no parameter's ``.grad`` is touched.  The per-patch reductions are
one launch per level (csrc/saliency_rows.hip).  The top-K selection is not differentiable: the gradient is that of the score along
the path the model took.  lstm = false is not covered.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Sequence, Tuple, Union

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


def _pass(model, batch, keep_patches, num_levels, fn, keep_gradients: bool, careful: bool):
    from . import utils as putils
    trace: List[dict] = []
    out = putils.recurse_train(model, batch, keep_patches, num_levels, careful=careful, trace=trace)
    tgt = fn(out["logits"])
    if tgt.shape != (out["logits"].shape[0],):
        raise ValueError(f"the target must map logits [B,C] to [B]; got {tuple(tgt.shape)}")
    # slides do not interact: the gradient of the batch sum is every slide's own gradient
    grads = torch.autograd.grad(tgt.sum(), [rec["fts"] for rec in trace])
    for rec, dx in zip(trace, grads):
        rec["grad_x_input"], rec["grad_norm"] = saliency_rows(dx, rec.pop("fts"), rec["num_ims"])
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
