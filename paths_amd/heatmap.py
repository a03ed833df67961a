"""Heat-map export (the data consumed by reference heatmap_visualise.py:113-175; drawing is out of scope).

``hierarchy_from_trace`` pulls one slide's per-level patch locations / importances / selected indices (and, from a
``recurse(..., attention=True)`` trace, the special token's attention; from a ``recurse(..., rollout=True)`` trace, its attention
rollout; from the trace of :func:`paths_amd.saliency.input_gradients`, every patch's gradient x input and gradient norm) out of the
trace of :func:`paths_amd.utils.recurse`.

``importance_map`` rasterises the importances exactly like the reference's overlay code: every patch of depth d paints
``importance + 1e-4`` over its footprint, then deeper levels are folded upwards with weight 1/2 wherever they exist
(heatmap_visualise.py:147-171).  ``attention_map`` rasterises the special token's attention of one decoder layer (one head or
the mean over heads), one raster per level and no fold across levels; ``rollout_map`` does the same for the attention rollout,
``relevance_map`` for the gradient-weighted attention relevance (:func:`paths_amd.saliency.attention_relevance`),
``saliency_map`` for the gradient attributions and ``removed_map`` for the cells a member of
:func:`paths_amd.saliency.removal_curves` turned to background.  Rasters are in units of the FINEST level's patches (one
cell = one patch of the last level), i.e. level-0 pixel space divided by ``patch_size / 2**(L-1)``.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np


# per-row attributions a saliency trace may carry: input_gradients', integrated_gradients' and smooth_grad's
SALIENCY_KINDS = ("grad_x_input", "grad_norm", "integrated_gradients", "smooth_grad_x_input", "smooth_grad_sq")
# the joint ranks saliency.removal_curves leaves in its trace, per order
REMOVAL_RANKS = ("removal_rank_morf", "removal_rank_lerf")


def hierarchy_from_trace(trace: List[dict], slide: int) -> List[Dict[str, np.ndarray]]:
    out = []
    for lv in trace:
        n = int(lv["num_ims"][slide])
        d = {"locs": lv["locs"][slide, :n].cpu().numpy(), "importance": lv["importance"][slide, :n].cpu().numpy(),
             "parent_inds": lv["parent_inds"][slide, :n].cpu().numpy()}
        if "keep_idx" in lv:
            d["keep_inds"] = lv["keep_idx"][slide, : int(lv["keep_count"][slide])].cpu().numpy()
        if "attention" in lv:
            d["attention"] = lv["attention"][slide, :, :, :n].cpu().numpy()          # [L, H, n]
            d["attention_self"] = lv["attention_self"][slide].cpu().numpy()          # [L, H]
        if "rollout" in lv:
            d["rollout"] = lv["rollout"][slide, :n].cpu().numpy()                      # [n]
            d["rollout_self"] = float(lv["rollout_self"][slide])
        if "attention_relevance" in lv:
            d["attention_relevance"] = lv["attention_relevance"][slide, :n].cpu().numpy()  # [n]
            d["attention_relevance_self"] = float(lv["attention_relevance_self"][slide])
        for key in SALIENCY_KINDS + REMOVAL_RANKS:                  # (the attribution functions' and removal_curves' per-row entries)
            if key in lv:
                d[key] = lv[key][slide, :n].cpu().numpy()                              # [n]
        out.append(d)
    return out


def _paint(dst: np.ndarray, locs: np.ndarray, values, size: int, patch_size: int, offset: float = 0.0):
    """dst[footprint of patch i] = values[i] + offset; a footprint is size x size finest cells."""
    cells = locs // patch_size
    for (cx, cy), v in zip(cells, values):
        dst[cx * size:(cx + 1) * size, cy * size:(cy + 1) * size] = v + offset


def importance_map(levels: List[Dict[str, np.ndarray]], base_grid, patch_size: int = 256, magnification_factor: int = 2) -> np.ndarray:
    """[X0 * f, Y0 * f] float map, f = magnification_factor**(L-1); 0 where no patch was visited."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    overall = np.zeros((L,) + shape, dtype=np.float64)
    for depth, lv in enumerate(levels):
        size = magnification_factor ** (L - 1 - depth)                       # footprint of one patch, in finest cells
        _paint(overall[depth], lv["locs"], lv["importance"], size, patch_size, 1e-4)
    for depth in range(L - 2, -1, -1):                                        # heatmap_visualise.py:167-169
        m = overall[depth + 1] != 0
        overall[depth][m] = overall[depth][m] + overall[depth + 1][m] * 0.5
    return overall[0]


def attention_map(levels: List[Dict[str, np.ndarray]], base_grid, layer: int = -1, head: Optional[int] = None, patch_size: int = 256,
                  magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): the special token's attention on each patch of
    decoder layer ``layer``, head ``head`` (None: the mean over heads), painted over the patch's footprint; 0 where the level did
    not visit.  ``levels`` from :func:`hierarchy_from_trace` of a ``recurse(..., attention=True)`` trace."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if "attention" not in lv:
            raise KeyError("level %d carries no attention: run recurse(..., attention=True)" % depth)
        a = lv["attention"][layer]                                            # [H, n]
        w = a.mean(axis=0, dtype=np.float64) if head is None else a[head]
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], w, magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def rollout_map(levels: List[Dict[str, np.ndarray]], base_grid, patch_size: int = 256, magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): the special token's attention rollout on each
    patch, painted over the patch's footprint like :func:`attention_map`; 0 where the level did not visit, no fold across levels.
    ``levels`` from :func:`hierarchy_from_trace` of a ``recurse(..., rollout=True)`` trace."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if "rollout" not in lv:
            raise KeyError("level %d carries no rollout: run recurse(..., rollout=True)" % depth)
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], lv["rollout"], magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def relevance_map(levels: List[Dict[str, np.ndarray]], base_grid, patch_size: int = 256, magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): the special token's gradient-weighted attention
    relevance on each patch, painted over the patch's footprint like :func:`rollout_map`; 0 where the level did not visit, no fold
    across levels.  ``levels`` from :func:`hierarchy_from_trace` of a :func:`paths_amd.saliency.attention_relevance` trace."""
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if "attention_relevance" not in lv:
            raise KeyError("level %d carries no attention relevance: run saliency.attention_relevance" % depth)
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], lv["attention_relevance"], magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def saliency_map(levels: List[Dict[str, np.ndarray]], base_grid, kind: str = "grad_x_input", patch_size: int = 256,
                 magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] float map per level (f = magnification_factor**(L-1)): every patch's gradient x input (``kind``
    "grad_x_input", signed) or gradient norm ("grad_norm"), painted over the patch's footprint like :func:`rollout_map`; 0 where the
    level did not visit, no fold across levels.  ``levels`` from :func:`hierarchy_from_trace` of a
    :func:`paths_amd.saliency.input_gradients` trace.  The traces of :func:`paths_amd.saliency.integrated_gradients` and
    :func:`paths_amd.saliency.smooth_grad` also carry "integrated_gradients" (signed), "smooth_grad_x_input" (signed) and
    "smooth_grad_sq"."""
    if kind not in SALIENCY_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(repr(k) for k in SALIENCY_KINDS), kind))
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if kind not in lv:
            raise KeyError("level %d carries no %s: take the trace from saliency.input_gradients / integrated_gradients / smooth_grad"
                           % (depth, kind))
        raster = np.zeros(shape, dtype=np.float64)
        _paint(raster, lv["locs"], lv[kind], magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps


def removed_map(levels: List[Dict[str, np.ndarray]], base_grid, count: int, order: str = "morf", patch_size: int = 256,
                magnification_factor: int = 2) -> List[np.ndarray]:
    """One [X0 * f, Y0 * f] uint8 map per level (f = magnification_factor**(L-1)): 1 over the footprint of every cell the member of
    :func:`paths_amd.saliency.removal_curves` that removes ``count`` patches (``out["counts"][s, slide]``) turned to background at
    that level - the patches of joint rank below ``count`` in ``order`` ("morf" / "lerf") -, 0 elsewhere; no fold across levels.
    ``levels`` from :func:`hierarchy_from_trace` of the trace removal_curves returns."""
    key = "removal_rank_" + order
    if key not in REMOVAL_RANKS:
        raise ValueError("order must be 'morf' or 'lerf', got %r" % (order,))
    L = len(levels)
    f = magnification_factor ** (L - 1)
    shape = (base_grid[0] * f, base_grid[1] * f)
    maps = []
    for depth, lv in enumerate(levels):
        if key not in lv:
            raise KeyError("level %d carries no %s: take the trace from saliency.removal_curves(order=%r or 'both')" % (depth, key, order))
        gone = (lv[key] >= 0) & (lv[key] < count)
        raster = np.zeros(shape, dtype=np.uint8)
        _paint(raster, lv["locs"][gone], np.ones(int(gone.sum()), np.uint8), magnification_factor ** (L - 1 - depth), patch_size)
        maps.append(raster)
    return maps
