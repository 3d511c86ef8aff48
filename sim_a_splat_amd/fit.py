"""Fit the resident Gaussians to pictures ("Optimiser step").

``fit_scene`` is the loop around three calls of a ``Rasterizer``: ``render`` a view, ``render_backward`` the loss gradient (several views
accumulate through ``out=``), ``adam_step`` the scene where it lives.  Nothing is uploaded between steps, so the storage order, the
groups, the features and the meshes of the context stay as they are.

Out of scope, and why: densification, pruning and opacity reset (N is fixed); an SSIM term (pass one through ``loss_and_grad``);
re-sorting the storage order as the means move (the order is a locality heuristic: ``r.upload(**r.read_scene(), ...)`` renews it);
gradients for K, the group poses and meshes (the limits of the backward pass).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .autograd import prechain

# The published 3DGS rates (Kerbl et al. 2023, their arguments' defaults): the means' rate is times the scene extent and decays
# exponentially to a hundredth over the run; the SH bands above DC step at a twentieth of DC's rate.
DEFAULT_LRS = dict(means=1.6e-4, opacities=5e-2, sh_dc=2.5e-3, sh_rest=2.5e-3 / 20.0, quats=1e-3, scales=5e-3)
MEANS_FINAL_FRACTION = 0.01
_WHAT = ("means", "opacities", "colors", "quats", "scales")
_RATES_OF = dict(means=("means",), opacities=("opacities",), colors=("sh_dc", "sh_rest"), quats=("quats",), scales=("scales",))


@dataclass
class FitResult:
    """``history[t]``: the mean loss over the views of step ``t + 1``, before that step; ``steps``: steps taken.  The fitted scene stays in
    the rasterizer (``read_scene`` returns it)."""
    history: List[float] = field(default_factory=list)
    steps: int = 0

    @property
    def loss(self) -> float:
        return self.history[-1] if self.history else float("nan")


def l1_loss_and_grad(rgb: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The default loss: mean absolute colour difference over the mask, and its gradient with respect to ``rgb``."""
    diff = rgb - target
    if mask is None:
        return diff.abs().mean(), torch.sign(diff) / diff.numel()
    w = mask.to(rgb.dtype).reshape(rgb.shape[0], rgb.shape[1], 1)
    denom = torch.clamp(3.0 * w.sum(), min=1.0)
    return (w * diff.abs()).sum() / denom, w * torch.sign(diff) / denom


def step_rates(lrs: Dict[str, float], what: Sequence[str], extent: float, t: int, iters: int) -> Dict[str, float]:
    """The rates of 1-based step ``t`` for the groups ``what``: ``lrs`` with the means' rate scaled by the scene extent and decayed."""
    out = {k: float(lrs[k]) for g in what for k in _RATES_OF[g]}
    if "means" in out:
        out["means"] *= float(extent) * MEANS_FINAL_FRACTION ** ((t - 1) / max(iters - 1, 1))
    return out


def mean_loss(r, viewmats, Ks, W: int, H: int, images, masks=None, background: Sequence[float] = (0.0, 0.0, 0.0),
              loss_and_grad: Optional[Callable] = None) -> float:
    """The loss ``fit_scene`` descends, averaged over ALL the views, for the scene as it stands in ``r`` (or a stand-in)."""
    lg = l1_loss_and_grad if loss_and_grad is None else loss_and_grad
    bg = tuple(float(v) for v in background)
    V = np.asarray(viewmats, dtype=np.float32).reshape(-1, 4, 4)
    K = np.asarray(Ks, dtype=np.float32).reshape(-1, 3, 3)
    total = 0.0
    for v in range(V.shape[0]):
        rgb = r.render(V[v], K[v], W, H, bg)["rgb"]
        mask = None if masks is None else torch.as_tensor(masks[v]).to(rgb.device)
        total += float(torch.as_tensor(lg(rgb, torch.as_tensor(images[v]).to(device=rgb.device, dtype=rgb.dtype).reshape(rgb.shape), mask)[0]))
    return total / max(V.shape[0], 1)


def fit_scene(r, viewmats, Ks, W: int, H: int, images, iters: int, what: Sequence[str] = ("colors", "opacities"),
              lrs: Optional[Dict[str, float]] = None, masks=None, views_per_step: int = 1,
              background: Sequence[float] = (0.0, 0.0, 0.0), loss_and_grad: Optional[Callable] = None, renderer=None, seed: int = 0,
              extent: Optional[float] = None, visible_only: bool = True) -> FitResult:
    """``iters`` Adam steps of the scene resident in ``r`` towards ``images [C,H,W,3]`` (float, 0..1) seen from ``viewmats [C,4,4]``,
    ``Ks [C,3,3]``.  Each step draws ``views_per_step`` views (without replacement, ``seed``), renders each, takes the loss gradient
    with respect to the delivered frame in torch on the frame's device, runs it through ``autograd.prechain``, accumulates
    ``render_backward(..., out=acc, want=what)`` and calls ``adam_step``.

    ``what``: the variable groups, of ``means``, ``opacities``, ``colors``, ``quats``, ``scales``.  ``lrs``: rates under
    ``Rasterizer.adam_step``'s keys, over ``DEFAULT_LRS``; the means' rate is times ``extent`` (default: the largest distance of a
    mean from the means' centre, from ``read_scene``) and decays to a hundredth.  ``masks [C,H,W]``: pixels that count.
    ``loss_and_grad(rgb, target, mask) -> (loss, g_rgb)`` replaces the default, the mean absolute colour difference over the mask.
    ``renderer``: an object with ``render``, ``render_backward`` and ``adam_step`` of ``Rasterizer``'s signatures used in ``r``'s
    place (a CPU stand-in runs the loop in tests).  ``visible_only``: Gaussians no view of a step saw keep their moments.
    Moments left by an earlier fit are dropped first where the renderer has ``adam_reset``."""
    R = r if renderer is None else renderer
    what = tuple(what)
    bad = [k for k in what if k not in _WHAT]
    if bad or not what:
        raise ValueError(f"fit_scene: what must name some of {_WHAT}, got {what}")
    rates = dict(DEFAULT_LRS, **(lrs or {}))
    V = np.asarray(viewmats.detach().cpu() if isinstance(viewmats, torch.Tensor) else viewmats, dtype=np.float32).reshape(-1, 4, 4)
    K = np.asarray(Ks.detach().cpu() if isinstance(Ks, torch.Tensor) else Ks, dtype=np.float32).reshape(-1, 3, 3)
    C = V.shape[0]
    if K.shape[0] != C or len(images) != C or (masks is not None and len(masks) != C):
        raise ValueError(f"fit_scene: {C} views, {K.shape[0]} Ks, {len(images)} images" + ("" if masks is None else f", {len(masks)} masks"))
    per = int(views_per_step)
    if not 1 <= per <= C:
        raise ValueError(f"fit_scene: views_per_step {per} out of [1, {C}]")
    if extent is None:
        extent = 1.0
        if "means" in what:
            m = R.read_scene()["means"]
            extent = float((m - m.mean(dim=0)).norm(dim=1).max()) if m.shape[0] else 1.0
    lg = l1_loss_and_grad if loss_and_grad is None else loss_and_grad
    bg = tuple(float(v) for v in background)
    if hasattr(R, "adam_reset"):
        R.adam_reset()
    rng = np.random.default_rng(seed)
    targets: Dict[int, Tuple[torch.Tensor, Optional[torch.Tensor]]] = {}
    losses = []
    for t in range(1, int(iters) + 1):
        acc = None
        total = None
        for v in rng.choice(C, size=per, replace=False):
            v = int(v)
            out = R.render(V[v], K[v], W, H, bg)
            rgb = out["rgb"]
            if v not in targets:   # a view's target and mask move to the frames' device once
                tm = None if masks is None else torch.as_tensor(masks[v]).to(rgb.device)
                targets[v] = (torch.as_tensor(images[v]).to(device=rgb.device, dtype=rgb.dtype).reshape(rgb.shape), tm)
            loss, g_rgb = lg(rgb, *targets[v])
            g_acc, g_a, _ = prechain(rgb, out["alpha"], out["depth"], bg, g_rgb, None, None)
            acc = R.render_backward(V[v], K[v], W, H, g_acc, g_a, None, out=acc, want=what)
            loss = torch.as_tensor(loss).detach().reshape(())
            total = loss if total is None else total + loss
        R.adam_step(acc, step_rates(rates, what, extent, t, int(iters)), t, visible_only=visible_only)
        losses.append(total / per)
    history = [float(x) for x in torch.stack(losses).cpu()] if losses else []   # (one read-back for the run: no step waits for its loss)
    return FitResult(history=history, steps=len(history))
