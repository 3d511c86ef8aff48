"""Frames as differentiable functions of the camera and of the Gaussians ("Backward pass").

``render_differentiable`` is a ``torch.autograd.Function`` around ``Rasterizer.render`` and ``Rasterizer.render_backward``: forward is
the ordinary frame, backward chains the frame's pointwise tail in torch (``prechain``) and hands the gradients of the raw
accumulators to the HIP backward pass.  The scene lives in the rasterizer: ``params`` only NAMES the arrays last uploaded, so that
their gradients have somewhere to go -- after an optimiser step of the caller's own the caller uploads them again
(``Rasterizer.upload``), or the next frame still shows the old scene.  The alternative that needs no upload is
``Rasterizer.adam_step``: a fused Adam step on the resident scene from the gradients ``Rasterizer.render_backward`` returns
(``fit.fit_scene`` is the loop).  The view matrix is an argument of every call and needs no upload.

The poses of the splat groups are a variable too (``group_poses=``, up to 32 groups per frame), and so are the node transforms of a
deformable scene (``node_transforms=``), whose REST arrays ``params`` names with ``rest_params=True``.  Not differentiated: K, meshes (a
scene with meshes is refused), joint angles, and every decision of the renderer (culls, clamps, the alpha and transmittance
thresholds), which are constants of the derivative.  The per-Gaussian sums are float atomics: gradients
vary in their last bits from run to run.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

# params key -> key of Rasterizer.render_backward's result
PARAM_KEYS = ("means", "opacities", "colors", "quats", "scales", "covariances")


def prechain(rgb: torch.Tensor, alpha: torch.Tensor, depth: torch.Tensor, background, g_rgb: Optional[torch.Tensor],
             g_alpha: Optional[torch.Tensor], g_depth: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Gradients of the raw accumulators (``sum c alpha T`` [H,W,3], ``1 - T_final`` [H,W], ``sum z alpha T`` [H,W]) from those of the
    delivered frame ``rgb = clamp(acc + (1 - alpha) bg, 0, 1)``, ``alpha``, ``depth = acc_z / max(alpha, 1e-10)``.  The clamp passes
    where ``rgb < 1``: with non-negative colours and background (SH colours are clamped at 0) the sum never falls below 0, so a pixel
    at 0 sits ON the bound, where torch's clamp passes too."""
    a = alpha.reshape(alpha.shape[0], alpha.shape[1])
    d = depth.reshape(a.shape)
    bg = torch.as_tensor(background, dtype=rgb.dtype, device=rgb.device).reshape(3)
    zero = torch.zeros_like(a)
    g_acc = torch.zeros_like(rgb) if g_rgb is None else torch.where(rgb < 1, g_rgb.reshape(rgb.shape), torch.zeros_like(rgb))
    g_a = (zero if g_alpha is None else g_alpha.reshape(a.shape)) - (g_acc * bg).sum(dim=-1)
    if g_depth is None:
        g_z = zero
    else:
        gd = g_depth.reshape(a.shape)
        g_z = gd / torch.clamp(a, min=1e-10)
        g_a = g_a - torch.where(a > 1e-10, gd * d / torch.clamp(a, min=1e-10), zero)
    return g_acc, g_a, g_z


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, viewmat, K, W, H, background, keys, pose_groups, group_poses, node_transforms, rest_params, *tensors):
        V = np.eye(4, dtype=np.float32)
        V[:viewmat.shape[0]] = viewmat.detach().cpu().numpy().astype(np.float32)
        if group_poses is not None:   # the frame is rendered under these poses, and they stay set
            r.set_group_poses(group_poses.detach().to(torch.float32).cpu().numpy().reshape(-1, 12))
        if node_transforms is not None:   # ... and under this deformation, which stays too
            r.deform(node_transforms.detach().to(device=r.device, dtype=torch.float32).contiguous())
        out = r.render(V, K, W, H, background)
        rgb, alpha, depth = out["rgb"].clone(), out["alpha"].clone(), out["depth"].clone()
        ctx.save_for_backward(rgb, alpha, depth)
        pmeta = None if group_poses is None else (group_poses.device, group_poses.dtype, tuple(group_poses.shape))
        nmeta = None if node_transforms is None else (node_transforms.device, node_transforms.dtype, tuple(node_transforms.shape))
        ctx.call = (r, V, K, W, H, background, keys, tuple(viewmat.shape), viewmat.device, viewmat.dtype,
                    [(t.device, t.dtype, tuple(t.shape)) for t in tensors], pose_groups, pmeta, nmeta, rest_params)
        return rgb, alpha, depth

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_depth):
        rgb, alpha, depth = ctx.saved_tensors
        r, V, K, W, H, background, keys, vshape, vdev, vdt, metas, pose_groups, pmeta, nmeta, rest_params = ctx.call
        g_acc, g_a, g_z = prechain(rgb, alpha, depth, background, g_rgb, g_alpha, g_depth)
        # only what some input needs: the projection's backward neither reads nor writes the rest
        needs = ctx.needs_input_grad[11:]
        need_poses = pmeta is not None and ctx.needs_input_grad[8]
        need_nodes = nmeta is not None and ctx.needs_input_grad[9]
        want = (("viewmat",) if ctx.needs_input_grad[1] else ()) + tuple(k for k, need in zip(keys, needs) if need) + \
            (("group_poses",) if need_poses else ())
        if need_nodes:   # the deformed means and orientations are what the nodes move
            want += tuple(k for k in ("means", "quats" if r.covariance_form == "quats" else "covariances") if k not in want)
        if not want:
            return (None,) * (11 + len(keys))
        res = r.render_backward(V, K, W, H, g_acc, g_a, g_z, want=want, pose_groups=pose_groups if need_poses else None)
        grads = [None]
        if ctx.needs_input_grad[1]:
            gv = torch.zeros(vshape, dtype=torch.float32, device=res["viewmat"].device)
            gv[:3] = res["viewmat"]
            grads = [gv.to(device=vdev, dtype=vdt)]
        gp = None
        if need_poses:   # the rows of pose_groups are filled, the rest are zero
            pdev, pdt, pshape = pmeta
            full = torch.zeros((pshape[0], 12), dtype=torch.float32, device=res["group_poses"].device)
            full[torch.as_tensor(list(pose_groups), dtype=torch.long, device=full.device)] = res["group_poses"].reshape(-1, 12)
            gp = full.reshape(pshape).to(device=pdev, dtype=pdt)
        gn = None
        if need_nodes:
            ndev, ndt, nshape = nmeta
            gn = r.deform_backward(res).reshape(nshape).to(device=ndev, dtype=ndt)
        if rest_params:   # params names the REST arrays: what the deformation moved goes through its adjoint, the others are theirs as they are
            moved = {k: res[k] for k, need in zip(keys, needs) if need and k in ("means", "quats", "covariances")}
            if moved:
                res = dict(res, **r.deform_backward_rest(moved))
        for k, (dev, dt, shape), need in zip(keys, metas, needs):
            grads.append(res[k].reshape(shape).to(device=dev, dtype=dt) if need else None)
        return (None, grads[0], None, None, None, None, None, None, gp, gn, None, *grads[1:])


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, rgb, target, mask, lambda_dssim):
        res = r.photometric_loss(rgb, target, mask=mask, lambda_dssim=lambda_dssim, want_grad=ctx.needs_input_grad[1])
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(res["g_rgb"].reshape(rgb.shape))
        ctx.like = (rgb.device, rgb.dtype)
        return res["loss"].clone()

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        (g_rgb,) = ctx.saved_tensors
        return None, (g_rgb * g.to(g_rgb.device)).to(device=ctx.like[0], dtype=ctx.like[1]), None, None, None


def photometric_loss(r, rgb: torch.Tensor, target, mask=None, lambda_dssim: float = 0.2) -> torch.Tensor:
    """The scalar 3DGS photometric loss ``(1 - lambda) L1 + lambda (1 - SSIM)`` of ``rgb [H,W,3]`` against ``target`` over ``mask``
    (``Rasterizer.photometric_loss`` of rasterizer ``r``, in its plain form), through which a gradient flows to ``rgb`` -- a frame of
    ``render_differentiable``, whose backward does the pre-chain.  No gradient flows to ``target``."""
    return _PhotometricLoss.apply(r, rgb, target, mask, float(lambda_dssim))


def render_differentiable(r, viewmat: torch.Tensor, K, width: int, height: int, params: Optional[Dict[str, torch.Tensor]] = None,
                          background: Optional[Sequence[float]] = None, group_poses: Optional[torch.Tensor] = None,
                          pose_groups: Optional[Sequence[int]] = None, node_transforms: Optional[torch.Tensor] = None,
                          rest_params: bool = False) -> Dict[str, torch.Tensor]:
    """One frame of rasterizer ``r`` -- ``rgb [H,W,3]``, ``alpha [H,W,1]``, ``depth [H,W,1]`` on its device -- through which gradients
    flow to ``viewmat`` (``[4,4]`` or ``[3,4]``, world to camera; its twelve upper entries are independent variables) and to those
    tensors of ``params`` that require grad.  ``params`` maps ``means``, ``opacities``, ``colors``, ``quats``, ``scales`` or
    ``covariances`` (``[N,6]``) to THE ARRAYS LAST UPLOADED to ``r``: the frame is rendered from the uploaded copy, not from these
    tensors, so upload again after changing them.  ``K`` is a constant.

    ``group_poses``: ``[G,3,4]`` or ``[G,12]``, rows ``[R | t]`` of ALL the scene's splat groups.  Unlike ``params`` it is a value: its
    detached float32 copy is set with ``set_group_poses`` before the frame (and stays set), and its gradient comes back in its shape,
    device and dtype, twelve independent entries per group, the rows of ``pose_groups`` filled and the rest zero.  ``pose_groups``
    defaults to all groups when there are at most 32 of them; with more it is required (32 ids at the most per frame).

    ``node_transforms``: ``[m,3,4]``, rows ``[R | t]`` of the nodes of the skin bound to ``r`` (``Rasterizer.bind_skin``).  A value like
    ``group_poses``: its detached float32 copy goes through ``r.deform`` before the frame (and stays set), and its gradient comes back
    in its shape, device and dtype, twelve independent entries per node (``Rasterizer.deform_backward``).  It combines with
    ``viewmat``, ``group_poses`` and ``params`` in one call; under a skin the gradients of ``params`` are those of the DEFORMED arrays.

    ``rest_params=True``: ``params`` names the REST arrays of the skinned scene, and the ``means`` / ``quats`` / ``covariances``
    gradients go through the deformation's adjoint (``Rasterizer.deform_backward_rest``) -- the frame is a function of the Gaussians
    that are stored; ``opacities``, ``colors`` and ``scales`` are untouched by a deformation.  It needs a skin and a deformation
    (``node_transforms=``, or ``r.deform`` before the call)."""
    bg = (0.0, 0.0, 0.0) if background is None else tuple(float(v) for v in background)
    params = params or {}
    unknown = [k for k in params if k not in PARAM_KEYS]
    if unknown:
        raise ValueError(f"render_differentiable: unknown params {unknown}; expected some of {PARAM_KEYS}")
    keys = tuple(k for k in PARAM_KEYS if k in params)
    Kc = np.ascontiguousarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K), dtype=np.float32)
    sel = None
    if group_poses is not None:
        n_groups = int(group_poses.shape[0])
        if group_poses.numel() != 12 * n_groups or group_poses.dim() not in (2, 3):
            raise ValueError(f"render_differentiable: group_poses must be [G,3,4] or [G,12], got {tuple(group_poses.shape)}")
        if pose_groups is None:
            if n_groups > 32:
                raise ValueError(f"render_differentiable: {n_groups} groups: name up to 32 of them in pose_groups")
            pose_groups = range(n_groups)
        sel = tuple(int(g) for g in pose_groups)
    elif pose_groups is not None:
        raise ValueError("render_differentiable: pose_groups without group_poses")
    if node_transforms is not None and (node_transforms.dim() != 3 or tuple(node_transforms.shape[1:]) != (3, 4)):
        raise ValueError(f"render_differentiable: node_transforms must be [m,3,4], got {tuple(node_transforms.shape)}")
    if rest_params and not r.has_skin:
        raise ValueError("render_differentiable: rest_params=True needs a skin bound to the rasterizer (bind_skin / set_skin)")
    rgb, alpha, depth = _Render.apply(r, viewmat, Kc, int(width), int(height), bg, keys, sel, group_poses, node_transforms, bool(rest_params),
                                      *[params[k] for k in keys])
    return dict(rgb=rgb, alpha=alpha, depth=depth)
