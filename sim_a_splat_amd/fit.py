"""Fit the resident Gaussians to pictures ("Optimiser step").

``fit_scene`` is the loop around three calls of a ``Rasterizer``: ``render`` a view, ``render_backward`` the loss gradient (several views
accumulate through ``out=``), ``adam_step`` the scene where it lives.  Nothing is uploaded between steps, so the storage order, the
groups, the features and the meshes of the context stay as they are.  With ``densify=DensifyConfig(...)`` the loop also keeps the density
statistics (``density_accumulate`` after every backward pass) and, on the config's schedule, calls ``densify`` and ``reset_opacity``: N changes
where the scene lives, the optimiser state follows the survivors ("Density control").  With ``densify=McmcConfig(cap_max, ...)``
the number of Gaussians is a budget instead: opacity and scale regularisers let Gaussians die, ``mcmc_refine`` re-births the dead on live
ones and grows the set by 5 % a time up to ``cap_max``, and ``mcmc_noise`` after every step does the exploring ("MCMC
density control").  That path keeps no statistics; ``mcmc_refine`` renews the storage order as ``densify`` does, on the device ("Storage order").

The loss: ``loss=None`` descends a mean absolute difference (or the caller's ``loss_and_grad``) with the chain to the raw accumulators in
torch; ``loss="dssim"`` descends the 3DGS photometric loss ``(1 - lambda) L1 + lambda (1 - SSIM)`` through ``Rasterizer.photometric_loss``,
whose kernels deliver the gradients ``render_backward`` takes ("Photometric loss").  ``image_metrics`` reports L1, SSIM and
PSNR of the scene as it stands.  ``init_scene`` makes the first scene from a point cloud ("Scene from points").

Out of scope, and why: multi-scale SSIM, LPIPS, depth and alpha loss terms (pass one through ``loss_and_grad``); screen-size splits and
prunes and ``revised_opacity`` of gsplat's strategy; gradients for K and meshes (the limits of the backward pass).  The group poses are
not variables of this loop: ``register.refine_group_poses`` fits them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

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
    n_history: List[int] = field(default_factory=list)   # with ``densify``: the scene's N after step ``t + 1`` (empty without)
    refines: List[Tuple[int, int, int, int]] = field(default_factory=list)   # with a ``McmcConfig``: (step, N, relocated, added) of every ``mcmc_refine``

    @property
    def loss(self) -> float:
        return self.history[-1] if self.history else float("nan")


@dataclass
class DensifyConfig:
    """The schedule and thresholds of density control in ``fit_scene``, gsplat's default strategy's: after step ``t`` (1-based) with
    ``start <= t < stop`` and ``t % every == 0`` the scene is densified and pruned by the statistics gathered since the last time; after
    every ``reset_every``-th step (0: never) below ``stop`` the opacities are reset to at most ``reset_opacity``.  Scales are pruned only
    once a reset has happened.  ``grow_scale3d`` and ``prune_scale3d`` are fractions of the scene extent."""
    start: int = 500
    stop: int = 15000
    every: int = 100
    reset_every: int = 3000
    grow_grad2d: float = 2e-4
    grow_scale3d: float = 0.01
    prune_opacity: float = 0.005
    prune_scale3d: float = 0.1
    max_gaussians: int = 0
    seed: int = 0
    split_factor: float = 1.6
    reset_opacity: float = 0.01

    def densify_at(self, t: int) -> bool:
        return self.start <= t < self.stop and self.every > 0 and t % self.every == 0

    def reset_at(self, t: int) -> bool:
        return self.reset_every > 0 and t < self.stop and t % self.reset_every == 0

    def check(self) -> None:
        if self.every < 1 or self.start < 0 or self.reset_every < 0:
            raise ValueError(f"DensifyConfig: every {self.every} < 1, or a negative start {self.start} / reset_every {self.reset_every}")
        for k in ("grow_grad2d", "grow_scale3d", "prune_opacity", "prune_scale3d"):
            if not (0.0 <= float(getattr(self, k)) < float("inf")):
                raise ValueError(f"DensifyConfig: {k} {getattr(self, k)} is negative or not finite")
        if not float(self.split_factor) > 1.0 or self.max_gaussians < 0 or not 0.0 < float(self.reset_opacity) < 1.0:
            raise ValueError(f"DensifyConfig: split_factor {self.split_factor} <= 1, max_gaussians {self.max_gaussians} < 0 or reset_opacity "
                             f"{self.reset_opacity} outside (0, 1)")


@dataclass
class McmcConfig:
    """The budget and schedule of MCMC density control in ``fit_scene``, gsplat's ``MCMCStrategy``'s: after step ``t`` (1-based) with
    ``start < t < stop`` and ``t % every == 0`` the dead Gaussians (opacity at most ``min_opacity``) are relocated onto alive ones and the
    set grows by ``grow_factor`` up to ``cap_max`` (``Rasterizer.mcmc_refine``); after EVERY step the means get noise of scale
    ``noise_lr`` times the means' current rate (``Rasterizer.mcmc_noise``).  ``opacity_reg`` and ``scale_reg`` weigh the regularisers
    ``mean(opacity)`` and ``mean(scale)`` that let Gaussians die."""
    cap_max: int
    start: int = 500
    stop: int = 25000
    every: int = 100
    min_opacity: float = 0.005
    grow_factor: float = 1.05
    noise_lr: float = 5e5
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    seed: int = 0

    def refine_at(self, t: int) -> bool:
        return self.start < t < self.stop and self.every > 0 and t % self.every == 0

    def check(self) -> None:
        if int(self.cap_max) < 1 or self.every < 1 or self.start < 0:
            raise ValueError(f"McmcConfig: cap_max {self.cap_max} < 1, every {self.every} < 1 or a negative start {self.start}")
        if not 0.0 <= float(self.min_opacity) < 1.0 or not 1.0 <= float(self.grow_factor) < float("inf"):
            raise ValueError(f"McmcConfig: min_opacity {self.min_opacity} outside [0, 1) or grow_factor {self.grow_factor} < 1 or not finite")
        for k in ("noise_lr", "opacity_reg", "scale_reg"):
            if not (0.0 <= float(getattr(self, k)) < float("inf")):
                raise ValueError(f"McmcConfig: {k} {getattr(self, k)} is negative or not finite")


def _scene_count(R) -> int:
    return int(R.n) if hasattr(R, "n") else int(R.read_scene()["means"].shape[0])


def _new_density_stats(R) -> Dict[str, torch.Tensor]:
    if hasattr(R, "new_density_stats"):
        return R.new_density_stats()
    n = int(R.read_scene()["means"].shape[0])
    return dict(grad_sum=torch.zeros(n), count=torch.zeros(n, dtype=torch.int32), max_radius=torch.zeros(n))


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


LOSSES = ("dssim",)


def _check_loss(who: str, loss: Optional[str], loss_and_grad: Optional[Callable], lambda_dssim: float) -> None:
    if loss is None:
        return
    if loss not in LOSSES:
        raise ValueError(f"{who}: loss must be None or one of {LOSSES}, got {loss!r}")
    if loss_and_grad is not None:
        raise ValueError(f"{who}: loss={loss!r} and loss_and_grad are two answers to one question: give one")
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise ValueError(f"{who}: lambda_dssim {lambda_dssim} outside [0, 1]")


def _pack_views(who: str, viewmats, Ks, images, masks) -> Tuple[np.ndarray, np.ndarray]:
    """``viewmats [C,4,4]`` and ``Ks [C,3,3]`` (arrays or tensors) as float32 host arrays, once the counts of views, images and masks agree."""
    V = np.asarray(viewmats.detach().cpu() if isinstance(viewmats, torch.Tensor) else viewmats, dtype=np.float32).reshape(-1, 4, 4)
    K = np.asarray(Ks.detach().cpu() if isinstance(Ks, torch.Tensor) else Ks, dtype=np.float32).reshape(-1, 3, 3)
    C = V.shape[0]
    if K.shape[0] != C or len(images) != C or (masks is not None and len(masks) != C):
        raise ValueError(f"{who}: {C} views, {K.shape[0]} Ks, {len(images)} images" + ("" if masks is None else f", {len(masks)} masks"))
    return V, K


def _view_pass(R, V, K, W: int, H: int, bg, cache: Dict[int, tuple], v: int, images, masks, loss: Optional[str], lg: Callable,
               lambda_dssim: float, share: int, out, want):
    """One view of a step, for ``fit_scene`` and ``deform.fit_dynamic_scene``: the frame, the loss against view ``v``'s target and mask
    (moved to the frame's device once, kept in ``cache``) -- ``lg`` and the chain to the raw accumulators in torch, or with ``loss`` the
    renderer's ``photometric_loss`` -- and ``render_backward(out=out, want=want)`` of its gradient divided by ``share`` (the views that share
    a step's weight; 1: as it is).  Returns ``(the loss, the accumulated gradients, the frame)``."""
    frame = R.render(V, K, W, H, bg)
    rgb = frame["rgb"]
    if v not in cache:
        tm = None if masks is None else torch.as_tensor(masks[v]).to(rgb.device)
        cache[v] = (torch.as_tensor(images[v]).to(device=rgb.device, dtype=rgb.dtype).reshape(rgb.shape), tm)
    weigh = (lambda g: g) if share == 1 else (lambda g: g / share)
    if loss is None:
        value, g_rgb = lg(rgb, *cache[v])
        g_acc, g_a, _ = prechain(rgb, frame["alpha"], frame["depth"], bg, weigh(g_rgb), None, None)
    else:
        pl = R.photometric_loss(rgb, cache[v][0], mask=cache[v][1], alpha=frame["alpha"], background=bg, lambda_dssim=lambda_dssim)
        value, g_acc, g_a = pl["loss"], weigh(pl["g_rgb"]), weigh(pl["g_alpha"])
    return value, R.render_backward(V, K, W, H, g_acc, g_a, None, out=out, want=want), frame


def mean_loss(r, viewmats, Ks, W: int, H: int, images, masks=None, background: Sequence[float] = (0.0, 0.0, 0.0),
              loss_and_grad: Optional[Callable] = None, loss: Optional[str] = None, lambda_dssim: float = 0.2) -> float:
    """The loss ``fit_scene`` descends, averaged over ALL the views, for the scene as it stands in ``r`` (or a stand-in)."""
    _check_loss("mean_loss", loss, loss_and_grad, lambda_dssim)
    lg = l1_loss_and_grad if loss_and_grad is None else loss_and_grad
    bg = tuple(float(v) for v in background)
    V, K = _pack_views("mean_loss", viewmats, Ks, images, masks)
    vals = []
    for v in range(V.shape[0]):
        rgb = r.render(V[v], K[v], W, H, bg)["rgb"]
        if loss is not None:
            vals.append(r.photometric_loss(rgb, torch.as_tensor(images[v]), mask=None if masks is None else torch.as_tensor(masks[v]),
                                           lambda_dssim=lambda_dssim, want_grad=False)["loss"].detach().reshape(()))
        else:
            mask = None if masks is None else torch.as_tensor(masks[v]).to(rgb.device)
            vals.append(float(torch.as_tensor(lg(rgb, torch.as_tensor(images[v]).to(device=rgb.device, dtype=rgb.dtype).reshape(rgb.shape), mask)[0])))
    if not vals:
        return 0.0
    return float(torch.stack(vals).mean()) if loss is not None else sum(vals) / len(vals)


def fit_scene(r, viewmats, Ks, W: int, H: int, images, iters: int, what: Sequence[str] = ("colors", "opacities"),
              lrs: Optional[Dict[str, float]] = None, masks=None, views_per_step: int = 1,
              background: Sequence[float] = (0.0, 0.0, 0.0), loss_and_grad: Optional[Callable] = None, renderer=None, seed: int = 0,
              extent: Optional[float] = None, visible_only: bool = True, loss: Optional[str] = None, lambda_dssim: float = 0.2,
              densify: Union[DensifyConfig, McmcConfig, None] = None) -> FitResult:
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
    Moments left by an earlier fit are dropped first where the renderer has ``adam_reset``.

    ``loss="dssim"``: the 3DGS photometric loss ``(1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM)`` instead: the renderer's
    ``photometric_loss`` takes the frame, the target, the mask, the frame's alpha and the background and returns the prechained
    ``g_rgb`` and ``g_alpha``, which go to ``render_backward`` as they are -- no torch op lies between the frame and its backward pass.
    ``history`` then holds that combined loss.  ``loss`` together with ``loss_and_grad`` is refused.

    ``densify``: a ``DensifyConfig`` turns adaptive density control on: ``density_accumulate`` follows every ``render_backward``, and after
    the steps of the config's schedule ``densify`` (then new statistics; the gradient buffers are made anew every step anyway) and
    ``reset_opacity`` are called, with the scene extent the means' rate uses.  ``n_history`` then holds N after every step.  A stand-in
    ``renderer`` needs those three methods too.  ``None``: the loop above, unchanged.

    ``densify=McmcConfig(cap_max, ...)``: MCMC density control instead ("MCMC density control"); no statistics are kept.
    Before ``adam_step``, ``opacity_reg / N`` is added to the accumulated ``opacities`` gradient and ``scale_reg / (3 N)`` to the ``scales``
    gradient, where those groups are in ``what``: the derivatives of ``opacity_reg mean(o)`` and ``scale_reg mean(s)`` with respect to the
    activated arrays, at the current N.  After ``adam_step``, on the config's schedule, ``mcmc_refine(seed=cfg.seed + t)``; then, every
    step, ``mcmc_noise(noise_lr * the means' rate of step t, t, cfg.seed)``.  ``n_history`` holds N after every step; it never exceeds
    ``max(cap_max, the initial N)``; ``refines`` holds ``(step, N, relocated, added)`` of every ``mcmc_refine``.  The regularisers make every gradient non-zero, so ``visible_only`` then skips nothing.
    ``noise_lr > 0`` without ``"means"`` in ``what`` is refused.  The regularisers are not part of ``history``, which stays the image
    loss.  Not provided: gsplat's two-pass order (relocate, then sample again for the growth) and its screen-size rules."""
    R = r if renderer is None else renderer
    _check_loss("fit_scene", loss, loss_and_grad, lambda_dssim)
    what = tuple(what)
    bad = [k for k in what if k not in _WHAT]
    if bad or not what:
        raise ValueError(f"fit_scene: what must name some of {_WHAT}, got {what}")
    rates = dict(DEFAULT_LRS, **(lrs or {}))
    V, K = _pack_views("fit_scene", viewmats, Ks, images, masks)
    C = V.shape[0]
    per = int(views_per_step)
    if not 1 <= per <= C:
        raise ValueError(f"fit_scene: views_per_step {per} out of [1, {C}]")
    if extent is None:
        extent = 1.0
        if "means" in what or densify is not None:
            m = R.read_scene()["means"]
            extent = float((m - m.mean(dim=0)).norm(dim=1).max()) if m.shape[0] else 1.0
    lg = l1_loss_and_grad if loss_and_grad is None else loss_and_grad
    bg = tuple(float(v) for v in background)
    if hasattr(R, "adam_reset"):
        R.adam_reset()
    rng = np.random.default_rng(seed)
    targets: Dict[int, Tuple[torch.Tensor, Optional[torch.Tensor]]] = {}
    losses = []
    stats, n_history, refines, was_reset = None, [], [], False
    mcmc, densify = (densify, None) if isinstance(densify, McmcConfig) else (None, densify)
    n_now = 0
    if mcmc is not None:
        mcmc.check()
        missing = [k for k in ("mcmc_refine", "mcmc_noise") if not hasattr(R, k)]
        if missing:
            raise ValueError(f"fit_scene: densify=McmcConfig needs a renderer with {missing}")
        if mcmc.noise_lr > 0 and "means" not in what:
            raise ValueError("fit_scene: McmcConfig.noise_lr > 0 scales the means' learning rate: put 'means' into what, or set noise_lr=0")
        n_now = _scene_count(R)
    if densify is not None:
        densify.check()
        missing = [k for k in ("density_accumulate", "densify", "reset_opacity") if not hasattr(R, k)]
        if missing:
            raise ValueError(f"fit_scene: densify needs a renderer with {missing}")
        stats = _new_density_stats(R)
    for t in range(1, int(iters) + 1):
        acc = None
        total = None
        for v in rng.choice(C, size=per, replace=False):
            v = int(v)
            value, acc, _ = _view_pass(R, V[v], K[v], W, H, bg, targets, v, images, masks, loss, lg, lambda_dssim, 1, out=acc, want=what)
            if stats is not None:
                R.density_accumulate(W, H, stats)
            value = torch.as_tensor(value).detach().reshape(())
            total = value if total is None else total + value
        if mcmc is not None:   # d/do of opacity_reg mean(o), d/ds of scale_reg mean(s): constants, at the current N
            if "opacities" in what and mcmc.opacity_reg:
                acc["opacities"].add_(float(mcmc.opacity_reg) / n_now)
            if "scales" in what and mcmc.scale_reg:
                acc["scales"].add_(float(mcmc.scale_reg) / (3 * n_now))
        R.adam_step(acc, step_rates(rates, what, extent, t, int(iters)), t, visible_only=visible_only)
        losses.append(total / per)
        if mcmc is not None:
            if mcmc.refine_at(t):
                done = R.mcmc_refine(min_opacity=mcmc.min_opacity, cap_max=int(mcmc.cap_max), grow_factor=mcmc.grow_factor, seed=mcmc.seed + t)
                n_now = int(done["n"])
                refines.append((t, n_now, int(done["relocated"]), int(done["added"])))
            if mcmc.noise_lr > 0:
                R.mcmc_noise(float(mcmc.noise_lr) * step_rates(rates, what, extent, t, int(iters))["means"], t, mcmc.seed)
            n_history.append(n_now)
        if stats is not None:
            if densify.densify_at(t):
                R.densify(stats, grow_grad2d=densify.grow_grad2d, grow_scale3d=densify.grow_scale3d, prune_opacity=densify.prune_opacity,
                          prune_scale3d=densify.prune_scale3d, scene_extent=extent, split_factor=densify.split_factor,
                          max_gaussians=densify.max_gaussians, seed=densify.seed + t, prune_scale_on=was_reset)
                stats = _new_density_stats(R)
            if densify.reset_at(t):
                R.reset_opacity(densify.reset_opacity)
                was_reset = True
            n_history.append(int(stats["count"].shape[0]))
    history = [float(x) for x in torch.stack(losses).cpu()] if losses else []   # (one read-back for the run: no step waits for its loss)
    return FitResult(history=history, steps=len(history), n_history=n_history, refines=refines)


def image_metrics(r, viewmats, Ks, W: int, H: int, images, masks=None, background: Sequence[float] = (0.0, 0.0, 0.0)) -> Dict[str, torch.Tensor]:
    """Per-view ``l1``, ``ssim``, ``mse`` and ``psnr`` (``-10 log10 mse``; images in 0..1) of the scene as it stands in ``r`` against ``images
    [C,H,W,3]`` over ``masks [C,H,W]``: float32 host tensors ``[C]``.  Each view is one frame and one terms-only
    ``Rasterizer.photometric_loss``; the terms of all the views are read back once, at the end."""
    bg = tuple(float(v) for v in background)
    V, K = _pack_views("image_metrics", viewmats, Ks, images, masks)
    rows = []
    for v in range(V.shape[0]):
        rgb = r.render(V[v], K[v], W, H, bg)["rgb"]
        rows.append(r.photometric_loss(rgb, torch.as_tensor(images[v]), mask=None if masks is None else torch.as_tensor(masks[v]),
                                       want_grad=False)["terms"])
    t = torch.stack(rows).cpu() if rows else torch.zeros((0, 4))
    return dict(l1=t[:, 1], ssim=t[:, 2], mse=t[:, 3], psnr=-10.0 * torch.log10(t[:, 3]))


SH_C0 = 0.28209479177387814   # the DC basis function: colour = 0.5 + SH_C0 * coefficient


def init_scene(r, points, colors=None, *, sh_degree: int = 3, init_opacity: float = 0.1, init_scale: float = 1.0, min_dist2: float = 1e-7,
               group_id=None, n_groups: int = 0, knn: Optional[Callable] = None) -> Dict[str, torch.Tensor]:
    """The first scene from a point cloud, the published initialisation (Kerbl et al. 2023; gsplat's trainer), ending in ``r.upload`` of the
    activated arrays, which are returned (float32 tensors on the device the distances live on):

    - ``means`` = ``points [N,3]``;
    - ``scales [N,3]`` = ``init_scale * sqrt(max(m, min_dist2))`` on all three axes, ``m = ((d0 + d1) + d2) / 3`` in float32 the mean squared
      distance to the three nearest other points (gsplat's rule with 3DGS's clamp), from ``r.knn_points(points, 3)`` (a HIP kernel;
      DESIGN.md 3, "Scene from points");
    - ``opacities`` = ``init_opacity``; ``quats`` = the identity ``(1, 0, 0, 0)``;
    - ``colors [N,(sh_degree+1)^2,3]``: the DC row ``(rgb - 0.5) / SH_C0``, the other rows zero.  ``colors [N,3]`` is float in 0..1 or uint8
      (divided by 255 in float32); ``None`` is grey 0.5.

    ``group_id`` / ``n_groups`` go to ``upload`` as they are.  ``knn``: a callable ``(points, k) -> dist2 [N,k]`` used in ``r.knn_points``' place
    (the CPU tests pass the numpy restatement).  ``ValueError`` for fewer than 4 points, a non-finite point, ``colors`` of another length
    or outside 0..1, ``sh_degree < 0``.  Not provided: readers for COLMAP or PLY clouds, random initial rotations."""
    who = "init_scene"
    if int(sh_degree) < 0:
        raise ValueError(f"{who}: sh_degree {sh_degree} must be >= 0")
    if isinstance(points, torch.Tensor):
        p = points.detach().to(torch.float32)
    else:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32)))
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{who}: points must be [N,3], got {list(p.shape)}")
    n = int(p.shape[0])
    if n < 4:
        raise ValueError(f"{who}: {n} points, at least 4 are needed (three neighbours each)")
    if knn is None:
        p = p.to(r.device).contiguous()
        if not bool(torch.isfinite(p).all()):
            raise ValueError(f"{who}: points hold a non-finite coordinate")
        d = r.knn_points(p, 3, indices=False)["dist2"]
    else:
        if not bool(torch.isfinite(p).all()):
            raise ValueError(f"{who}: points hold a non-finite coordinate")
        d = knn(p.cpu().numpy(), 3)
        d = d.detach() if isinstance(d, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(d, dtype=np.float32)))
        d = d.to(device=p.device, dtype=torch.float32)
    if tuple(d.shape) != (n, 3):
        raise ValueError(f"{who}: knn returned {list(d.shape)}, expected [{n}, 3]")
    dev = p.device
    # a divisor as a one-element tensor: torch turns a division by a Python number into a product with its reciprocal, which is not the
    # correctly rounded quotient the formulas (and tests/tools/knn_ref.py) name
    const = lambda v: torch.full((1,), v, dtype=torch.float32, device=dev)
    if colors is None:
        rgb = torch.full((n, 3), 0.5, dtype=torch.float32, device=dev)
    else:
        c = colors.detach() if isinstance(colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(colors)))
        if tuple(c.shape) != (n, 3):
            raise ValueError(f"{who}: colors must be [{n}, 3], got {list(c.shape)}")
        c = c.to(dev)
        rgb = c.to(torch.float32) / const(255.0) if c.dtype == torch.uint8 else c.to(torch.float32)
        if not bool(((rgb >= 0.0) & (rgb <= 1.0)).all()):
            raise ValueError(f"{who}: colors outside 0..1 (float) / not uint8")
    m = ((d[:, 0] + d[:, 1]) + d[:, 2]) / const(3.0)
    s = float(init_scale) * torch.sqrt(torch.clamp(m, min=float(min_dist2)))
    kk = (int(sh_degree) + 1) ** 2
    sh = torch.zeros((n, kk, 3), dtype=torch.float32, device=dev)
    sh[:, 0, :] = (rgb - 0.5) / const(SH_C0)
    quats = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    quats[:, 0] = 1.0
    scene = dict(means=p.contiguous(), opacities=torch.full((n,), float(init_opacity), dtype=torch.float32, device=dev), colors=sh,
                 quats=quats, scales=s.to(torch.float32)[:, None].expand(n, 3).contiguous())
    r.upload(scene["means"], scene["opacities"], scene["colors"], quats=scene["quats"], scales=scene["scales"], sh_degree=int(sh_degree),
             group_id=group_id, n_groups=n_groups)
    return scene
