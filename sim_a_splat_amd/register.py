"""Register the robot to the splat: the ICP step of the reference (match_splat.py:94-223) without open3d.

The reference samples 20 000 points from the posed URDF meshes, crops the Gaussian centres to a polygon volume, guesses a transform
from the two centroids and runs open3d's ``registration_icp`` with ``TransformationEstimationPointToPoint(with_scaling=True)`` and a
correspondence distance of 0.2.  Here the sampling is ``mesh_io.sample_surface``, the crop ``segment.polygon_volume_mask``, the
nearest-neighbour search of every iteration ``Rasterizer.match_points`` (a HIP kernel; DESIGN.md 3, "Point matching") and the
similarity fit ``umeyama`` on the 18 moments that call returns.  Everything but the matcher is NumPy float64.

    python -m sim_a_splat_amd.register --splat SCENE --urdf ROBOT.urdf --joint-config joint_config.npy \\
        --robot-description-dir DIR --package-name NAME --polygon polygon_bounds.npy --axis-min -0.3 --axis-max 0.1 \\
        [--rotation-xyz 0,0,0 --scale 1 --offset 0,0,0 --threshold 0.2 --points 20000 --seed 0] --out MASKS_DIR [--masks]

writes ``icp_transformation.npy``, ``trans_init.npy``, ``polygon_bounds.npy`` and ``joint_config.npy``; with ``--masks`` it goes on
through ``segment.segment_robot`` and writes ``link_masks_global_dict.npz`` too: the whole directory ``SplatHandler`` reads.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from .rasterizer import _host

N_MOMENTS = 18   # n, sum p' (3), sum q (3), sum q p'^T (9, row-major), sum |p'|^2, sum d2 (sas_match_points)


@dataclass
class RegistrationResult:
    transformation: np.ndarray          # 4x4 float64, source -> target
    fitness: float                      # held matches / source points
    inlier_rmse: float                  # sqrt(sum d2 / held matches)
    iterations: int                     # updates applied
    history: List[Tuple[float, float]] = field(default_factory=list)   # (fitness, inlier_rmse) of every evaluation, the first included


def umeyama(moments, with_scaling: bool = True) -> np.ndarray:
    """The least-squares similarity ``q ~ c R p' + t`` of the held matches, 4x4 float64, from the moments of ``match_points``: the
    closed form of Umeyama (1991) as Eigen's ``umeyama`` evaluates it, which open3d's point-to-point estimation calls.  Centred
    cross-covariance ``Sigma = sum q p'^T / n - mu_q mu_p^T = U D V^T``; ``S = diag(1, 1, -1)`` when ``det U det V < 0`` (a reflection
    would fit better: the proper rotation is taken); ``R = U S V^T``, ``c = tr(D S) / sigma_p^2`` (1 without scaling),
    ``t = mu_q - c R mu_p``.  ValueError below 3 matches or when the matched source points coincide (``sigma_p^2 = 0``)."""
    m = np.asarray(moments, np.float64).reshape(-1)
    if m.shape[0] != N_MOMENTS:
        raise ValueError(f"moments must hold {N_MOMENTS} values, got {m.shape[0]}")
    n = m[0]
    if not n >= 3:
        raise ValueError(f"umeyama needs at least 3 matches, got {n:g}")
    mu_p, mu_q = m[1:4] / n, m[4:7] / n
    sigma = m[7:16].reshape(3, 3) / n - np.outer(mu_q, mu_p)
    var_p = m[16] / n - float(mu_p @ mu_p)
    if not var_p > 0.0 or not np.isfinite(sigma).all():
        raise ValueError("umeyama: the matched source points are degenerate (zero variance)")
    U, D, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = (U * S) @ Vt
    c = float((D * S).sum() / var_p) if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mu_q - c * (R @ mu_p)
    return T


def rotation_from_xyz(rotation_xyz) -> np.ndarray:
    """``Rx(a) Ry(b) Rz(c)``: open3d's ``get_rotation_matrix_from_xyz``."""
    a, b, c = (float(x) for x in rotation_xyz)
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]], np.float64)
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]], np.float64)
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]], np.float64)
    return Rx @ Ry @ Rz


def initial_guess(source, target, rotation_xyz=(0.0, 0.0, 0.0), scale: float = 1.0, offset=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The reference's first guess (match_splat.py:178-196), 4x4: ``scale * R(rotation_xyz) | centre(target) - centre(source) +
    offset``.  As there, the UNROTATED, unscaled source centre is subtracted: with a rotation or a scale the guess does not bring the
    centres together, and ``offset`` is how the reference's user makes up for it."""
    T = np.eye(4)
    T[:3, :3] = float(scale) * rotation_from_xyz(rotation_xyz)
    T[:3, 3] = (np.asarray(_host(target), np.float64).reshape(-1, 3).mean(axis=0) - np.asarray(_host(source), np.float64).reshape(-1, 3).mean(axis=0)
                + np.asarray(offset, np.float64).reshape(3))
    return T


def register_similarity(source, target, init=None, max_correspondence_distance: float = 0.2, max_iteration: int = 30,
                        relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, with_scaling: bool = True, rasterizer=None,
                        matcher: Optional[Callable] = None) -> RegistrationResult:
    """Point-to-point ICP with a similarity (or, ``with_scaling=False``, rigid) update: ``source [S,3]`` onto ``target [T,3]`` from the
    4x4 ``init``.  The loop is that of open3d's ``registration_icp`` as its public documentation and source describe it: evaluate
    (match every moved source point to its nearest target within ``max_correspondence_distance``; ``fitness = n / S``,
    ``inlier_rmse = sqrt(sum d2 / n)``); then per iteration ``T <- umeyama(matches) . T`` and evaluate again; stop when the absolute
    changes of fitness and of inlier_rmse are both below their limits, or after ``max_iteration`` updates.

    One deviation from open3d: it moves its source cloud by every update and so accumulates float64 roundings in the points; here
    each iteration rounds the accumulated ``T`` to float32 once and the matcher applies it to the ORIGINAL source -- nothing is
    re-transformed, and both clouds stay where they are (on the device, with a ``Rasterizer``) for the whole loop.

    ``matcher``: any callable with ``Rasterizer.match_points``' signature and result (the seam for CPU tests); None uses
    ``rasterizer.match_points``, and without a rasterizer either one is made on device 0 for the call.  ValueError when fewer than 3
    points match (``umeyama``)."""
    T = np.eye(4) if init is None else np.array(np.asarray(_host(init), np.float64).reshape(4, 4))
    own = None
    if matcher is None:
        import torch
        if rasterizer is None:
            from .rasterizer import Rasterizer
            rasterizer = own = Rasterizer(0)
        dev = lambda a: (a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float32))
                         ).to(device=rasterizer.device, dtype=torch.float32).reshape(-1, 3).contiguous()
        source, target = dev(source), dev(target)     # uploaded once
        matcher = rasterizer.match_points
    else:
        source = np.ascontiguousarray(np.asarray(_host(source), np.float32).reshape(-1, 3))
        target = np.ascontiguousarray(np.asarray(_host(target), np.float32).reshape(-1, 3))
    n_source = int(source.shape[0])

    def evaluate(T):
        m = np.asarray(matcher(source, target, transform=T, max_distance=float(max_correspondence_distance))["moments"], np.float64)
        n = float(m[0])
        return m, (n / n_source if n_source else 0.0), (float(np.sqrt(m[17] / n)) if n > 0 else 0.0)

    try:
        m, fitness, rmse = evaluate(T)
        history = [(fitness, rmse)]
        iterations = 0
        for _ in range(int(max_iteration)):
            T = umeyama(m, with_scaling) @ T
            iterations += 1
            before = (fitness, rmse)
            m, fitness, rmse = evaluate(T)
            history.append((fitness, rmse))
            if abs(before[0] - fitness) < relative_fitness and abs(before[1] - rmse) < relative_rmse:
                break
    finally:
        if own is not None:
            own.close()
    return RegistrationResult(T, fitness, rmse, iterations, history)


def robot_surface_points(urdf, joint_config, robot_description_dir: str, package_name: str, n_links: int = 7, n_points: int = 20000,
                         seed: int = 0) -> np.ndarray:
    """``n_points`` points ``[n,3]`` float64 on the robot's first ``n_links`` visual meshes posed at ``joint_config``, combined into
    one surface as the reference does (match_splat.py:64-105): ``segment.robot_link_meshes`` with an identity ICP, then
    ``mesh_io.sample_surface`` (whose note on open3d's Poisson-disk sampler applies)."""
    from . import mesh_io, segment
    meshes, transforms = segment.robot_link_meshes(urdf, joint_config, np.eye(4), robot_description_dir, package_name, n_links)
    vs, fs, base = [], [], 0
    for (v, f), T in zip(meshes, transforms):
        vs.append(segment.transform_vertices(v, T))
        fs.append(np.asarray(f, np.int64).reshape(-1, 3) + base)
        base += len(v)
    return mesh_io.sample_surface(np.concatenate(vs), np.concatenate(fs), n_points, seed)


def register_robot(means, urdf, joint_config, robot_description_dir: str, package_name: str, *, polygon=None, axis_min: float = -np.inf,
                   axis_max: float = np.inf, axis: str = "Z", rotation_xyz=(0.0, 0.0, 0.0), scale: float = 1.0, offset=(0.0, 0.0, 0.0),
                   threshold: float = 0.2, n_links: int = 7, n_points: int = 20000, seed: int = 0, max_iteration: int = 30,
                   rasterizer=None, matcher=None) -> Tuple[RegistrationResult, np.ndarray]:
    """Steps 1-4 of the reference's match_splat.py for a splat's centres ``means [N,3]``: crop them to the polygon volume (None: no
    crop), sample the posed robot, guess from the two centres, register.  Returns ``(result, trans_init)``;
    ``result.transformation`` is what ``icp_transformation.npy`` holds."""
    from . import segment
    pts = np.asarray(_host(means), np.float32).reshape(-1, 3)
    if polygon is not None:
        pts = pts[segment.polygon_volume_mask(pts, polygon, axis_min, axis_max, axis)]
    if len(pts) < 3:
        raise ValueError(f"{len(pts)} Gaussian centres in the crop volume: nothing to register to")
    robot = robot_surface_points(urdf, joint_config, robot_description_dir, package_name, n_links, n_points, seed)
    trans_init = initial_guess(robot, pts, rotation_xyz, scale, offset)
    result = register_similarity(robot, pts, trans_init, max_correspondence_distance=threshold, max_iteration=max_iteration,
                                 rasterizer=rasterizer, matcher=matcher)
    return result, trans_init


# ---- camera pose from a picture: render and compare ("Backward pass") -----------------------------------------------------
@dataclass
class PoseRefinement:
    viewmat: np.ndarray                 # 4x4 float64, world -> camera (OpenCV axes)
    loss: float                         # mean squared colour difference of the last evaluation, at full size
    history: List[Tuple[int, float]] = field(default_factory=list)   # (downsampling factor, loss) of every evaluation


def se3_exp(xi) -> np.ndarray:
    """4x4 rigid motion of the twist ``xi = (omega, v)``: rotation by Rodrigues' formula, translation ``V(omega) v``."""
    xi = np.asarray(xi, np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        A, B, C = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        A, B, C = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th), (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * Wx + B * (Wx @ Wx)
    T[:3, 3] = (np.eye(3) + B * Wx + C * (Wx @ Wx)) @ v
    return T


def twist_gradient(d_viewmat, viewmat) -> np.ndarray:
    """Gradient with respect to a camera-frame twist ``xi`` at 0 of a loss whose gradient with respect to the rows ``[R | t]`` of
    ``viewmat`` is ``d_viewmat [3,4]``, for ``viewmat(xi) = se3_exp(xi) viewmat``."""
    G = np.asarray(d_viewmat, np.float64).reshape(-1, 4)[:3]
    A = np.asarray(viewmat, np.float64).reshape(4, 4)[:3]
    g = np.zeros(6)
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1.0
        Ek = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
        g[k] = float(np.sum(G * (Ek @ A)))
    g[3:] = G[:, 3]
    return g


def refine_camera_pose(r, image, V0, K, W: int, H: int, iters: int = 300, mask=None, *, factors: Sequence[int] = (4, 2, 1),
                       step: Tuple[float, float] = (0.01, 0.01), background=(0.0, 0.0, 0.0),
                       pivot_depth: Optional[float] = None, loss_and_grad: Optional[Callable] = None) -> PoseRefinement:
    """Refine the camera pose ``V0`` (4x4 world -> camera) so that rasterizer ``r``'s frame looks like ``image [H,W,3]`` (float, 0..1):
    Adam on an se(3) increment of the camera (a twist about the point ``pivot_depth`` in front of the camera -- None: the median depth
    of the first frame's covered pixels -- re-centred on the current pose after every step: turning about the scene instead of about the
    camera keeps rotation and translation from trading against each other), minimising
    the mean squared colour difference over the pixels where ``mask [H,W]`` is non-zero, coarse to fine: the iterations are split
    evenly over ``factors``, each rendering at ``K / factor`` against the area-averaged image.  ``step``: Adam's step in radians and in
    scene units at the start of a level; it falls to a twentieth over the level.  Gradients come from
    ``autograd.render_differentiable``; ``loss_and_grad(V, K, W, H, target, mask) -> (loss, d_viewmat [3,4])`` replaces the renderer
    (tests run the same optimiser on a CPU reference).  What the renderer does not differentiate -- K, decisions -- stays fixed."""
    import torch
    from ._picture_fit import pyramid_level, twist_adam
    dev = getattr(r, "device", "cpu")
    img = torch.as_tensor(np.asarray(_host(image), np.float32)).reshape(H, W, 3)
    m = torch.ones((H, W), dtype=torch.float32) if mask is None else (torch.as_tensor(np.asarray(_host(mask))) != 0).to(torch.float32).reshape(H, W)
    K0 = np.asarray(_host(K), np.float64).reshape(3, 3)
    V = np.asarray(_host(V0), np.float64).reshape(4, 4).copy()

    def evaluate(Vc, Kc, w, h, target, tm):
        if loss_and_grad is not None:
            return loss_and_grad(Vc, Kc, w, h, target, tm)
        from .autograd import render_differentiable
        vm = torch.tensor(Vc, dtype=torch.float32, device=dev, requires_grad=True)
        out = render_differentiable(r, vm, Kc.astype(np.float32), w, h, background=background)
        t, k = target.to(out["rgb"].device), tm.to(out["rgb"].device)
        loss = (k[..., None] * (out["rgb"] - t) ** 2).sum() / (3.0 * torch.clamp(k.sum(), min=1.0))
        loss.backward()
        return float(loss.detach()), vm.grad[:3].double().cpu().numpy()

    if pivot_depth is None and loss_and_grad is None:
        first = r.render(V.astype(np.float32), K0.astype(np.float32), W, H, background)
        seen = first["depth"][first["alpha"] > 0.5]
        pivot_depth = float(seen.median()) if seen.numel() else 1.0
    Tp = np.eye(4)
    Tp[2, 3] = 1.0 if pivot_depth is None else float(pivot_depth)
    Tpi = np.linalg.inv(Tp)
    res = PoseRefinement(V, float("nan"))
    per = max(1, int(iters) // max(1, len(factors)))
    for f in factors:
        w, h, targets, tms, Kcs = pyramid_level(img[None], m[None], K0[None], W, H, f)
        m1, m2 = np.zeros((1, 6)), np.zeros((1, 6))
        for it in range(per):
            loss, dV = evaluate(V, Kcs[0], w, h, targets[0], tms[0])
            res.history.append((int(f), loss))
            g = twist_gradient(dV, V)
            g[:3] += np.cross(g[3:], Tp[:3, 3])   # the same twist about the pivot
            xi, m1, m2 = twist_adam(g[None], m1, m2, it, per, step)
            V = Tp @ se3_exp(xi[0]) @ Tpi @ V
    res.viewmat = V
    res.loss = evaluate(V, K0, W, H, img, m)[0]
    res.history.append((1, res.loss))
    return res


# ---- group poses from pictures: where is the T-block, where are the links ("Backward pass") -------------------------------------
@dataclass
class GroupPoseRefinement:
    poses: np.ndarray                   # [G,3,4] float64, rows [R | t] of every group (the groups that were not refined as they were)
    loss: float                         # mean squared colour difference of the last evaluation, at full size, averaged over the views
    history: List[Tuple[int, float]] = field(default_factory=list)   # (downsampling factor, loss) of every evaluation


def refine_group_poses(r, images, viewmats, Ks, W: int, H: int, groups: Sequence[int], iters: int = 200, masks=None, pivots=None,
                       step: Tuple[float, float] = (0.01, 0.01), factors: Sequence[int] = (2, 1), background=(0.0, 0.0, 0.0),
                       loss_and_grad: Optional[Callable] = None) -> GroupPoseRefinement:
    """Refine the poses of the splat groups ``groups`` (up to 32 ids) of rasterizer ``r`` so that its frames look like ``images
    [C,H,W,3]`` (float, 0..1) seen from ``viewmats [C,4,4]`` (world -> camera) with ``Ks [C,3,3]``: all views observe ONE set of poses.
    ``refine_camera_pose``'s scheme per group: Adam on an se(3) twist that left-multiplies the group's pose about its pivot
    (``pivots [n_sel,3]``, world coordinates; None: the pose's translation, where the canonical origin lands), minimising the mean
    squared colour difference over ``masks [C,H,W]`` averaged over the views, coarse to fine over ``factors`` with the step falling to
    a twentieth over each level.  Every step renders every view and accumulates the pose gradient of ``Rasterizer.render_backward``
    through ``out=``.  The start is ``r.get_group_poses()``; the poses are written to ``r`` with ``set_group_poses`` every step and are
    left at the result.  ``loss_and_grad(poses [G,3,4], V, K, w, h, target, mask) -> (loss, d_poses [n_sel,3,4])`` replaces the
    renderer for one view (tests run the same optimiser on a CPU reference)."""
    import torch
    from ._picture_fit import device_level, pyramid_level, squared_colour_pass, twist_adam
    sel = [int(g) for g in groups]
    n_sel = len(sel)
    Vs = np.asarray(_host(viewmats), np.float64).reshape(-1, 4, 4)
    C = Vs.shape[0]
    K0s = np.asarray(_host(Ks), np.float64).reshape(-1, 3, 3)
    if K0s.shape[0] == 1 and C > 1:
        K0s = np.repeat(K0s, C, axis=0)
    imgs = torch.as_tensor(np.asarray(_host(images), np.float32)).reshape(C, H, W, 3)
    ms = torch.ones((C, H, W), dtype=torch.float32) if masks is None else (torch.as_tensor(np.asarray(_host(masks))) != 0).to(torch.float32).reshape(C, H, W)
    poses = np.asarray(r.get_group_poses(), np.float64).reshape(-1, 3, 4).copy()
    if n_sel < 1 or len(set(sel)) != n_sel or min(sel) < 0 or max(sel) >= poses.shape[0]:
        raise ValueError(f"refine_group_poses: groups must name distinct ids below {poses.shape[0]}, got {tuple(groups)}")
    piv = poses[sel, :, 3].copy() if pivots is None else np.asarray(_host(pivots), np.float64).reshape(n_sel, 3).copy()
    acc = {}   # the pose gradients of the views, summed: made by the first pass, reused by the others
    level = (lambda f: pyramid_level(imgs, ms, K0s, W, H, f)) if loss_and_grad is not None else (lambda f: device_level(imgs, ms, Vs, K0s, W, H, f, r.device))

    def evaluate(G, lv):
        """(loss, d_poses [n_sel,3,4]) averaged over the views, at one ``level``."""
        if loss_and_grad is not None:
            w, h, targets, tms, Kcs = lv
            parts = [loss_and_grad(G, Vs[v], Kcs[v], w, h, targets[v], tms[v]) for v in range(C)]
            return sum(p[0] for p in parts) / C, sum(np.asarray(p[1], np.float64).reshape(n_sel, 3, 4) for p in parts) / C
        total = squared_colour_pass(r, *lv, background, acc, want=("group_poses",), pose_groups=sel)
        return float(total), acc["group_poses"].double().cpu().numpy()   # (the evaluation waits here, once)

    res = GroupPoseRefinement(poses, float("nan"))
    per = max(1, int(iters) // max(1, len(factors)))
    for f in factors:
        lv = level(f)
        m1, m2 = np.zeros((n_sel, 6)), np.zeros((n_sel, 6))
        for it in range(per):
            r.set_group_poses(poses.reshape(-1, 12).astype(np.float32))
            loss, dG = evaluate(poses, lv)
            res.history.append((int(f), loss))
            G4 = np.tile(np.eye(4), (n_sel, 1, 1))
            G4[:, :3] = poses[sel]
            tw = np.stack([twist_gradient(dG[q], G4[q]) for q in range(n_sel)])
            tw[:, :3] += np.cross(tw[:, 3:], piv)   # the same twists about the pivots
            xi, m1, m2 = twist_adam(tw, m1, m2, it, per, step)
            for q, g in enumerate(sel):
                Tp = np.eye(4)
                Tp[:3, 3] = piv[q]
                Tpi = np.eye(4)
                Tpi[:3, 3] = -piv[q]
                M = Tp @ se3_exp(xi[q]) @ Tpi
                poses[g] = (M @ G4[q])[:3]
                piv[q] = (M @ np.append(piv[q], 1.0))[:3]   # the pivot is a point of the group: it moves with it
    r.set_group_poses(poses.reshape(-1, 12).astype(np.float32))
    res.poses = poses
    res.loss = evaluate(poses, level(1))[0]
    res.history.append((1, res.loss))
    return res


def main(argv: Optional[Sequence[str]] = None, matcher=None) -> int:
    import argparse
    from . import io, poses, segment
    vec3 = lambda s: [float(x) for x in s.split(",")]
    ap = argparse.ArgumentParser(prog="python -m sim_a_splat_amd.register", description=__doc__.split("\n\n")[0])
    ap.add_argument("--splat", required=True, help="scene: .npy of centres, .npz / .json scene, splatfacto config.yml, run directory or .ckpt")
    ap.add_argument("--urdf", required=True)
    ap.add_argument("--joint-config", required=True, help=".npy, or comma-separated joint positions")
    ap.add_argument("--robot-description-dir", required=True, help="what package://NAME in the URDF's mesh filenames stands for")
    ap.add_argument("--package-name", required=True)
    ap.add_argument("--polygon", required=True, help="polygon_bounds.npy of the crop volume")
    ap.add_argument("--axis-min", type=float, required=True)
    ap.add_argument("--axis-max", type=float, required=True)
    ap.add_argument("--axis", default="Z")
    ap.add_argument("--rotation-xyz", type=vec3, default=[0.0, 0.0, 0.0], help="initial rotation, radians about x, y, z (comma-separated)")
    ap.add_argument("--scale", type=float, default=1.0, help="initial scale")
    ap.add_argument("--offset", type=vec3, default=[0.0, 0.0, 0.0], help="added to the initial translation (comma-separated)")
    ap.add_argument("--threshold", type=float, default=0.2, help="largest correspondence distance")
    ap.add_argument("--points", type=int, default=20000, help="points sampled from the robot's meshes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--links", type=int, default=7)
    ap.add_argument("--distance", type=float, default=0.015, help="--masks: the mask rule's distance")
    ap.add_argument("--out", required=True, help="masks directory to write")
    ap.add_argument("--masks", action="store_true", help="go on through segment.segment_robot and write the link masks too")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    means = segment.load_means(a.splat)
    jc = io.load_joint_config(a.joint_config) if Path(a.joint_config).exists() else np.array([float(x) for x in a.joint_config.split(",")])
    polygon = np.load(a.polygon, allow_pickle=False)
    r = None
    if matcher is None or a.masks:
        from .rasterizer import Rasterizer
        r = Rasterizer(a.device)
    try:
        result, trans_init = register_robot(means, a.urdf, jc, a.robot_description_dir, a.package_name, polygon=polygon, axis_min=a.axis_min,
                                            axis_max=a.axis_max, axis=a.axis, rotation_xyz=a.rotation_xyz, scale=a.scale, offset=a.offset,
                                            threshold=a.threshold, n_links=a.links, n_points=a.points, seed=a.seed, rasterizer=r,
                                            matcher=matcher)
        icp = result.transformation
        s, _, _ = poses.decompose_icp(icp)      # what SplatHandler will ask of the file: raises before anything is written
        d = Path(a.out)
        d.mkdir(parents=True, exist_ok=True)
        if a.masks:
            crop = segment.polygon_volume_mask(means, polygon, a.axis_min, a.axis_max, a.axis)
            masks = segment.segment_robot(means, a.urdf, jc, icp, a.robot_description_dir, a.package_name, a.links, distance=a.distance,
                                          crop=crop, rasterizer=r)
            segment.write_masks_dir(d, masks, jc, icp)
            for k, m in masks.items():
                print(f"{k}: {int(m.sum())} of {len(m)} Gaussians")
    finally:
        if r is not None:
            r.close()
    np.save(d / "icp_transformation.npy", icp)
    np.save(d / "trans_init.npy", trans_init)
    np.save(d / "polygon_bounds.npy", np.asarray(polygon, np.float64))
    np.save(d / "joint_config.npy", np.asarray(jc, np.float64).reshape(-1))
    print(f"fitness {result.fitness:.4f}, inlier rmse {result.inlier_rmse:.6f}, {result.iterations} iterations, scale {s:.6f}")
    print(f"-> {d}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
