"""What the loops that fit poses to pictures share (``register.refine_camera_pose``, ``register.refine_group_poses``,
``deform.fit_node_transforms``, ``deform.fit_dynamic_scene``): the Adam rule on se(3) twists, one level of the image pyramid, and the
pass over the views that sums the squared colour difference and its gradients.  What a loop does with a step twist -- about which pivot,
on which side -- stays with the loop."""
from __future__ import annotations

from typing import Tuple

import numpy as np


def adam_scalars(it: int, per: int) -> Tuple[float, float, float]:
    """``(decay, c1, c2)`` of 0-based step ``it`` of ``per``: the step's fall to a twentieth over the level, and Adam's two bias
    corrections.  ``twist_adam`` and the device optimiser (``deform.NodeOptimizer.step``) both take them from here."""
    decay = 0.05 ** (it / max(1, per - 1))
    return decay, 1 - 0.9**(it + 1), 1 - 0.999**(it + 1)


def twist_adam(tw, m1, m2, it: int, per: int, step):
    """One Adam step on ``n`` twists: ``tw [n,6]`` the gradients ``(omega, v)``, ``m1``, ``m2 [n,6]`` the moments, ``step`` the rates in
    radians and scene units at the start of a level.  Returns ``(xi [n,6], m1, m2)``: the twists to step by, and the new moments.
    Float64, elementwise: a row does not depend on how many rows go with it."""
    decay, c1, c2 = adam_scalars(it, per)
    m1 = 0.9 * m1 + 0.1 * tw
    m2 = 0.999 * m2 + 0.001 * tw * tw
    hat = (m1 / c1) / (np.sqrt(m2 / c2) + 1e-12)
    return -np.concatenate([step[0] * decay * hat[:, :3], step[1] * decay * hat[:, 3:]], axis=1), m1, m2


def pyramid_level(imgs, ms, K0s, W: int, H: int, f: int):
    """One level of the pyramid: ``(w, h, targets [C,h,w,3], tms [C,h,w], Kcs [C,3,3])`` of ``imgs [C,H,W,3]``, their 0/1 masks ``ms
    [C,H,W]`` (host tensors) and intrinsics ``K0s [C,3,3]`` at a ``1 / f`` of the size: the area average of the masked images renormalised
    by the mask's coverage, the pixels covered by more than half as the mask, and the first two rows of K rescaled."""
    import torch
    import torch.nn.functional as Fn
    w, h = max(1, W // f), max(1, H // f)
    if f == 1:
        targets, tms = imgs, ms
    else:
        cover = Fn.interpolate(ms[:, None], size=(h, w), mode="area")[:, 0]
        targets = Fn.interpolate((imgs * ms[..., None]).permute(0, 3, 1, 2), size=(h, w), mode="area").permute(0, 2, 3, 1) / torch.clamp(cover, min=1e-6)[..., None]
        tms = (cover > 0.5).to(torch.float32)
    Kcs = K0s.copy()
    Kcs[:, 0] *= w / W
    Kcs[:, 1] *= h / H
    return w, h, targets, tms, Kcs


def device_level(imgs, ms, Vs, K0s, W: int, H: int, f: int, device):
    """The ``pyramid_level`` as ``squared_colour_pass`` takes it, formed once: ``(cams, w, h, targets, tms, scales)`` -- the views' float32
    ``(V, K)``, the targets and masks on ``device``, and every view's ``1 / (3 max(sum(mask), 1) C)`` from the host mask (nothing waits)."""
    import torch
    w, h, targets, tms, Kcs = pyramid_level(imgs, ms, K0s, W, H, f)
    C = len(Vs)
    scales = [1.0 / (3.0 * float(torch.clamp(tms[v].sum(), min=1.0)) * C) for v in range(C)]
    cams = [(Vs[v].astype(np.float32), Kcs[v].astype(np.float32)) for v in range(C)]
    return cams, w, h, targets.to(device), tms.to(device), scales


def squared_colour_pass(r, cams, w: int, h: int, targets, tms, scales, background, out, **backward):
    """The views' frames and backward passes of the mean squared colour difference over the masks, averaged over the views: every view's
    gradients are summed into the dict ``out`` (zeroed first; ``backward``: ``want`` and ``pose_groups`` of ``Rasterizer.render_backward``).
    Returns the loss as a float64 device scalar: the pass only enqueues."""
    import torch
    from .autograd import prechain
    for a in out.values():
        a.zero_()
    total = None
    for (V32, K32), target, tm, scale in zip(cams, targets, tms, scales):
        frame = r.render(V32, K32, w, h, background)
        rgb, alpha, depth = frame["rgb"].clone(), frame["alpha"].clone(), frame["depth"].clone()
        err = rgb - target
        diff = tm[..., None] * err
        value = (diff * err).sum().to(torch.float64) * scale
        total = value if total is None else total + value
        g_acc, g_a, g_z = prechain(rgb, alpha, depth, background, 2.0 * scale * diff, None, None)
        out.update(r.render_backward(V32, K32, w, h, g_acc, g_a, g_z, out=out, **backward))
    return total
