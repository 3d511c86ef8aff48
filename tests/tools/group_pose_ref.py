"""The yardstick of the group-pose gradient (sas_render_backward_poses; DESIGN.md 3, "Backward pass"): tests/tools/grad_ref.py takes the
group poses as constants, so this helper poses the scene ITSELF in torch -- leaf ``G [n_groups,3,4]``, means' = Rg m + t,
Sigma' = Rg Sigma Rg^T handed over as cov6 tensors (for a scene of quaternions and scales Sigma' = M M^T, M = Rg R(q) diag(s)) -- and
hands the posed arrays to ``grad_ref.project(..., group_id=None)`` and ``grad_ref.render`` unchanged.  float64 is the reference, float32
measures what float32 arithmetic alone costs."""
import numpy as np
import torch

import grad_ref


def pose(P, G, gid):
    """The leaves ``P`` of grad_ref.leaves posed by ``G [n_groups,3,4]``: a dict grad_ref.project reads (means, op, colors, cov6)."""
    Gg = G[torch.as_tensor(np.asarray(gid).astype(np.int64))]
    Rg, t = Gg[:, :, :3], Gg[:, :, 3]
    means = torch.einsum("nij,nj->ni", Rg, P["means"]) + t
    if P.get("quats") is not None:
        M = (Rg @ grad_ref.quat_to_rotmat(P["quats"])) * P["scales"].reshape(-1, 1, 3)
        cov = M @ M.transpose(1, 2)
    else:
        c6 = P["cov6"]
        S = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], dim=1).reshape(-1, 3, 3)
        cov = Rg @ S @ Rg.transpose(1, 2)
    cov6 = torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], dim=1)
    return dict(means=means, op=P["op"], colors=P["colors"], cov6=cov6)


def forward(sc, cam, dtype=torch.float64, Rt=None, G=None, straight_through=False):
    """(leaves P, pose leaf G [n_groups,3,4], viewmat leaf [3,4], intermediates, raw frame)."""
    V, K, W, H = cam
    P = grad_ref.leaves(sc, dtype)
    if G is None:
        G = torch.tensor(np.asarray(sc["Rt"] if Rt is None else Rt, np.float64).reshape(-1, 3, 4), dtype=dtype, requires_grad=True)
    vm = torch.tensor(np.asarray(V, np.float64).reshape(4, 4)[:3], dtype=dtype, requires_grad=True)
    I = grad_ref.project(pose(P, G, sc["gid"]), vm, K, W, H, sc["sh"], None, None, straight_through)
    F = grad_ref.render(I, I["valid"], I["radii"], W, H)
    return P, G, vm, I, F


def _full(P, G, vm):
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()
    full = dict(means=z(P["means"]), opacities=z(P["op"]), colors=z(P["colors"]), viewmat=z(vm))
    if "quats" in P:
        full.update(quats=z(P["quats"]), scales=z(P["scales"]))
    else:
        full.update(covariances=z(P["cov6"]))
    full["group_poses"] = z(G)
    return full


def gradients(sc, cam, g_rgb=None, g_alpha=None, g_depth=None, dtype=torch.float64, Rt=None, mask_near=True, straight_through=False):
    """grad_ref.gradients with the poses as a variable: {"full": means, opacities, colors, viewmat, quats + scales | covariances,
    group_poses [n_groups,3,4]; "near"; "valid"; "margin"; "loss"}.  ``straight_through``: grad_ref.project's mutant."""
    P, G, vm, I, F = forward(sc, cam, dtype, Rt, straight_through=straight_through)
    keep = (~F["near"]).to(dtype) if mask_near else torch.ones_like(F["alpha"])
    loss = torch.zeros((), dtype=dtype)
    for g, f in ((g_rgb, F["acc_rgb"]), (g_alpha, F["alpha"]), (g_depth, F["acc_z"])):
        if g is not None:
            gt = torch.as_tensor(np.asarray(g, np.float64), dtype=dtype).reshape(f.shape)
            loss = loss + (gt * (keep[..., None] if f.dim() == 3 else keep) * f).sum()
    loss.backward()
    return dict(full=_full(P, G, vm), near=F["near"].numpy(), valid=I["valid"].numpy(), margin=I["margin"].numpy(), loss=float(loss.detach()))


def loss_at(sc, cam, Rt, g, keep):
    """The float64 loss ``sum keep (g_rgb acc_rgb + g_alpha alpha + g_depth acc_z)`` under the poses ``Rt``, ``keep [H,W]`` held fixed:
    what central differences of the poses are taken of."""
    with torch.no_grad():
        _, _, _, _, F = forward(sc, cam, torch.float64, Rt)
        k = torch.as_tensor(np.asarray(keep, np.float64))
        loss = 0.0
        for gi, f in zip(g, (F["acc_rgb"], F["alpha"], F["acc_z"])):
            gt = torch.as_tensor(np.asarray(gi, np.float64)).reshape(f.shape)
            loss = loss + float((gt * (k[..., None] if f.dim() == 3 else k) * f).sum())
    return loss


def mse_loss_and_grad(sc, groups, background=(0.0, 0.0, 0.0)):
    """``loss_and_grad`` of register.refine_group_poses on this reference, float64: the mean squared colour difference of the delivered
    frame over the mask, and its gradient with respect to the rows of ``groups``."""
    def fn(poses, V, K, w, h, target, mask):
        G = torch.tensor(np.asarray(poses, np.float64).reshape(-1, 3, 4), requires_grad=True)
        _, _, _, _, F = forward(sc, (V, K, w, h), torch.float64, G=G)
        rgb = grad_ref.finish(F, background)["rgb"]
        t = torch.as_tensor(np.asarray(target, np.float64)).reshape(h, w, 3)
        m = torch.as_tensor(np.asarray(mask, np.float64)).reshape(h, w)
        loss = (m[..., None] * (rgb - t) ** 2).sum() / (3.0 * torch.clamp(m.sum(), min=1.0))
        loss.backward()
        return float(loss.detach()), G.grad.numpy()[list(groups)]
    return fn


def frame(sc, cam, Rt=None, background=(0.0, 0.0, 0.0)):
    """The delivered rgb [H,W,3] of the reference, float64."""
    with torch.no_grad():
        _, _, _, _, F = forward(sc, cam, torch.float64, Rt)
        return grad_ref.finish(F, background)["rgb"].numpy()
