"""The yardstick of the backward pass ("Backward pass"): oracle/np_twin.py's ``project`` and ``render`` restated in torch
and differentiated by torch autograd -- float64 for the reference, float32 to measure what float32 arithmetic alone costs.

Decisions (culls, the radius' ceil, the Jacobian's clamp, alpha against 1/255 and 0.999, T (1 - alpha) against 1e-4) are taken on
detached values and are constants of the derivative.  ``render`` also reports every pixel at which some decision of a live
(pixel, entry) pair lies within a relative ``MARGIN`` of its threshold: the tests zero the upstream gradients there, so that an
implementation that takes such a decision the other way contributes, like the reference, exactly nothing.

The intermediates of the projection (means2d, conics, colors, depths, opacities) keep their gradients, so the compositing's backward
is held to the reference apart from the projection's."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

TILE = 16
NEAR, FAR, EPS2D = 0.01, 1e10, 0.3
ALPHA_THRESHOLD = 1.0 / 255.0
MAX_ALPHA, T_STOP = 0.999, 1e-4
MARGIN = 1e-3
SCREEN = ("means2d", "conics", "opacities", "colors", "depths")


def quat_to_rotmat(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def sh_basis(dirs, degree):
    d = dirs / dirs.norm(dim=-1, keepdim=True)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    B = [torch.full_like(x, 0.2820947917738781)]
    if degree >= 1:
        B += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
    if degree >= 2:
        z2 = z * z
        fC1 = x * x - y * y
        fS1 = 2 * x * y
        B += [0.5462742152960395 * fS1, -1.092548430592079 * z * y, 0.9461746957575601 * z2 - 0.3153915652525201,
              -1.092548430592079 * z * x, 0.5462742152960395 * fC1]
    if degree >= 3:
        fTmp0C = -2.285228997322329 * z2 + 0.4570457994644658
        fTmp1B = 1.445305721320277 * z
        fC2 = x * fC1 - y * fS1
        fS2 = x * fS1 + y * fC1
        B += [-0.5900435899266435 * fS2, fTmp1B * fS1, fTmp0C * y, z * (1.865881662950577 * z2 - 1.119528997770346),
              fTmp0C * x, fTmp1B * fC1, -0.5900435899266435 * fC2]
    return torch.stack(B, dim=1)


def _near(v, thr):
    """|v - thr| within MARGIN of thr's size (elementwise, detached)."""
    return (v - thr).abs() <= MARGIN * abs(thr)


def project(P, viewmat, K, W, H, sh_degree, group_id=None, group_Rt=None, straight_through=False):
    """np_twin.project on tensors: ``P`` holds means, op, colors and quats + scales or cov6; ``viewmat [3,4]``.  Returns the
    intermediates, ``valid`` / ``radii`` (detached), ``margin``: per Gaussian, whether a projection-level decision is within MARGIN,
    and what the Jacobian's clamp saw: ``ratios [N,2]`` (x/z, y/z, detached) and ``limits`` (x_pos, x_neg, y_pos, y_neg).
    ``straight_through`` is a MUTANT the tests measure their cases' sensitivity with: the same forward, but the clamp's gradient
    passes to x and y as if it never bound."""
    means, op = P["means"], P["op"]
    dt = means.dtype
    n = means.shape[0]
    Kc = torch.as_tensor(np.asarray(K, np.float64).reshape(3, 3), dtype=dt)
    fx, fy, cx, cy = Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]
    Rg = None
    if group_id is not None and group_Rt is not None:
        G = torch.as_tensor(np.asarray(group_Rt, np.float64).reshape(-1, 3, 4), dtype=dt)[torch.as_tensor(np.asarray(group_id).astype(np.int64))]
        Rg = G[:, :, :3]
        means = torch.einsum("nij,nj->ni", Rg, means) + G[:, :, 3]
    if P.get("quats") is not None:
        R = quat_to_rotmat(P["quats"])
        if Rg is not None:
            R = Rg @ R
        M = R * P["scales"].reshape(-1, 1, 3)
        cov = M @ M.transpose(1, 2)
    else:
        c6 = P["cov6"]
        cov = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], dim=1).reshape(-1, 3, 3)
        if Rg is not None:
            cov = Rg @ cov @ Rg.transpose(1, 2)
    Rw, tw = viewmat[:3, :3], viewmat[:3, 3]
    pc = means @ Rw.T + tw
    covc = Rw @ cov @ Rw.T
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    zd = z.detach()
    valid = (zd >= NEAR) & (zd <= FAR)
    margin = _near(zd, NEAR) | _near(zd, FAR)
    zs = torch.where(valid, z, torch.ones_like(z))
    tan_fovx, tan_fovy = 0.5 * W / fx, 0.5 * H / fy
    lim_x_pos = (W - cx) / fx + 0.3 * tan_fovx
    lim_x_neg = cx / fx + 0.3 * tan_fovx
    lim_y_pos = (H - cy) / fy + 0.3 * tan_fovy
    lim_y_neg = cy / fy + 0.3 * tan_fovy
    rz = 1.0 / zs
    ux, uy = x * rz, y * rz
    for u, lo, hi in ((ux.detach(), -lim_x_neg, lim_x_pos), (uy.detach(), -lim_y_neg, lim_y_pos)):
        margin = margin | (valid & (_near(u, float(lo)) | _near(u, float(hi))))
    tx = zs * torch.minimum(lim_x_pos, torch.maximum(-lim_x_neg, ux))
    ty = zs * torch.minimum(lim_y_pos, torch.maximum(-lim_y_neg, uy))
    if straight_through:
        tx, ty = x + (tx - x).detach(), y + (ty - y).detach()
    zero = torch.zeros_like(rz)
    J = torch.stack([fx * rz, zero, -fx * tx * rz * rz, zero, fy * rz, -fy * ty * rz * rz], dim=1).reshape(-1, 2, 3)
    c2 = J @ covc @ J.transpose(1, 2)
    c00 = c2[:, 0, 0] + EPS2D
    c01 = c2[:, 0, 1]
    c11 = c2[:, 1, 1] + EPS2D
    det = c00 * c11 - c01 * c01
    valid = valid & (det.detach() > 0)
    dets = torch.where(valid, det, torch.ones_like(det))
    conic = torch.stack([c11 / dets, -c01 / dets, c00 / dets], dim=1)
    mx = fx * x * rz + cx
    my = fy * y * rz + cy
    opd = op.detach()
    thr32 = float(np.float32(ALPHA_THRESHOLD))
    valid = valid & (opd >= thr32)
    margin = margin | (_near(opd, thr32))
    with torch.no_grad():
        extent = torch.clamp(torch.sqrt(2.0 * torch.log(torch.clamp(opd, min=1e-30) / ALPHA_THRESHOLD)), max=3.33)
        extent = torch.where(valid, torch.nan_to_num(extent, nan=0.0), torch.zeros_like(extent))
        b = 0.5 * (c00 + c11)
        v1 = b + torch.sqrt(torch.clamp(b * b - det, min=0.01))
        r1 = extent * torch.sqrt(torch.clamp(v1, min=0))
        px_ = torch.minimum(extent * torch.sqrt(torch.clamp(c00, min=0)), r1)
        py_ = torch.minimum(extent * torch.sqrt(torch.clamp(c11, min=0)), r1)
        rx, ry = torch.ceil(px_), torch.ceil(py_)
        for pre in (px_, py_):   # the ceil: a radius within MARGIN of an integer
            margin = margin | (valid & ((pre - torch.round(pre)).abs() <= MARGIN * torch.clamp(pre, min=1.0)))
        valid = valid & (~((rx <= 0) & (ry <= 0)))
        mxd, myd = mx.detach(), my.detach()
        for v, thr in ((mxd + rx, 0.0), (mxd - rx, float(W)), (myd + ry, 0.0), (myd - ry, float(H))):   # the rectangle against the image
            margin = margin | (valid & ((v - thr).abs() <= MARGIN * max(1.0, abs(thr))))
        valid = valid & (~((mxd + rx <= 0) | (mxd - rx >= W) | (myd + ry <= 0) | (myd - ry >= H)))
        valid = valid & ((rx > 0) & (ry > 0))
        radii = torch.stack([torch.where(valid, rx, torch.zeros_like(rx)), torch.where(valid, ry, torch.zeros_like(ry))], dim=1)
    campos = -Rw.T @ tw
    if sh_degree >= 0:
        kk = (sh_degree + 1) ** 2
        B = sh_basis(means - campos, sh_degree)
        rgb = torch.clamp(torch.einsum("nk,nkc->nc", B, P["colors"].reshape(n, kk, 3)) + 0.5, min=0.0)
    else:
        rgb = P["colors"].reshape(n, 3) * 1.0
    return dict(valid=valid, radii=radii, margin=margin, means2d=torch.stack([mx, my], dim=1), depths=z * 1.0, conics=conic,
                colors=rgb, opacities=op * 1.0, ratios=torch.stack([ux, uy], dim=1).detach(),
                limits=tuple(float(v) for v in (lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg)))


def render(I, valid, radii, W, H):
    """np_twin.render's compositing on the intermediates ``I``: the raw accumulators ``acc_rgb [H,W,3]``, ``alpha [H,W]`` (1 - T_final),
    ``acc_z [H,W]``, and ``near [H,W]``: pixels with a decision of a live pair within MARGIN of its threshold."""
    m2, con, col, dep, opa = I["means2d"], I["conics"], I["colors"], I["depths"], I["opacities"]
    dt = m2.dtype
    tw, th = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    m2d, rad = m2.detach().double().numpy(), radii.double().numpy()
    x0 = np.clip(np.floor((m2d[:, 0] - rad[:, 0]) / TILE), 0, tw).astype(int)
    x1 = np.clip(np.ceil((m2d[:, 0] + rad[:, 0]) / TILE), 0, tw).astype(int)
    y0 = np.clip(np.floor((m2d[:, 1] - rad[:, 1]) / TILE), 0, th).astype(int)
    y1 = np.clip(np.ceil((m2d[:, 1] + rad[:, 1]) / TILE), 0, th).astype(int)
    vis = np.nonzero(valid.numpy())[0]
    dkey = dep.detach().numpy().astype(np.float32)
    order = vis[np.lexsort((vis, dkey[vis]))]
    py, px = torch.meshgrid(torch.arange(H, dtype=dt) + 0.5, torch.arange(W, dtype=dt) + 0.5, indexing="ij")
    T = torch.ones((H, W), dtype=dt)
    acc = torch.zeros((H, W, 3), dtype=dt)
    accz = torch.zeros((H, W), dtype=dt)
    done = torch.zeros((H, W), dtype=torch.bool)
    near = torch.zeros((H, W), dtype=torch.bool)
    for g in order:
        ys, ye, xs, xe = y0[g] * TILE, min(y1[g] * TILE, H), x0[g] * TILE, min(x1[g] * TILE, W)
        if ys >= ye or xs >= xe:
            continue
        sl = (slice(ys, ye), slice(xs, xe))
        dx, dy = m2[g, 0] - px[sl], m2[g, 1] - py[sl]
        a, b, c = con[g, 0], con[g, 1], con[g, 2]
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        oE = opa[g] * torch.exp(-sigma)
        al = torch.clamp(oE, max=MAX_ALPHA)
        Ts, ds = T[sl], done[sl]
        ald, oEd = al.detach(), oE.detach()
        use = (~ds) & (sigma.detach() >= 0) & (ald >= ALPHA_THRESHOLD)
        nT = Ts * (1 - al)
        nTd = nT.detach()
        stop = use & (nTd <= T_STOP)
        nr = (~ds) & (_near(ald, ALPHA_THRESHOLD) | _near(oEd, MAX_ALPHA) | (use & _near(nTd, T_STOP)))
        use = use & ~stop
        w = torch.where(use, al * Ts, torch.zeros_like(al))
        pad = (xs, W - xe, ys, H - ye)
        wf = torch.nn.functional.pad(w, pad)
        acc = acc + wf[..., None] * col[g]
        accz = accz + wf * dep[g]
        T = T - torch.nn.functional.pad(torch.where(use, Ts - nT, torch.zeros_like(al)), pad)
        done = done | torch.nn.functional.pad(stop, pad)
        near = near | torch.nn.functional.pad(nr, pad)
    return dict(acc_rgb=acc, alpha=1 - T, acc_z=accz, near=near)


def leaves(sc, dtype=torch.float64):
    """The scene dict of tests/tools/scene_cases.py as leaf tensors that require grad."""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=True)
    n = np.asarray(sc["means"]).shape[0]
    kk = (sc["sh"] + 1) ** 2 if sc["sh"] >= 0 else 1
    P = dict(means=t(sc["means"]), op=t(sc["op"]), colors=t(np.asarray(sc["colors"], np.float64).reshape(n, kk, 3)))
    if sc.get("quats") is not None and sc.get("cov6") is None:
        P.update(quats=t(sc["quats"]), scales=t(sc["scales"]))
    else:
        P.update(cov6=t(sc["cov6"]))
    return P


def forward(sc, cam, dtype=torch.float64, Rt=None, viewmat=None, P=None, straight_through=False):
    """(leaves P, viewmat leaf [3,4], intermediates, raw frame) of scene ``sc`` seen by ``cam = (V, K, W, H)``."""
    V, K, W, H = cam
    P = leaves(sc, dtype) if P is None else P
    if viewmat is None:
        viewmat = torch.tensor(np.asarray(V, np.float64).reshape(4, 4)[:3], dtype=dtype, requires_grad=True)
    gid = sc.get("gid")
    rt = (sc.get("Rt") if Rt is None else Rt) if gid is not None else None
    I = project(P, viewmat, K, W, H, sc["sh"], gid, rt, straight_through)
    for k in SCREEN:
        if I[k].requires_grad:
            I[k].retain_grad()
    F = render(I, I["valid"], I["radii"], W, H)
    return P, viewmat, I, F


def finish(F, background=(0.0, 0.0, 0.0)):
    """The frame sas_render delivers from the raw accumulators (np_twin.render's last lines)."""
    a = F["alpha"]
    bg = torch.as_tensor(np.asarray(background, np.float64), dtype=a.dtype)
    return dict(rgb=torch.clamp(F["acc_rgb"] + (1 - a)[..., None] * bg, 0, 1), alpha=a, depth=F["acc_z"] / torch.clamp(a, min=1e-10))


def gradients(sc, cam, g_rgb=None, g_alpha=None, g_depth=None, dtype=torch.float64, Rt=None, mask_near=True, straight_through=False):
    """Gradients of ``sum g_rgb acc_rgb + sum g_alpha alpha + sum g_depth acc_z``: {"screen": means2d, conics, opacities, colors, depths;
    "full": means, opacities, colors, quats + scales | covariances, viewmat; "near": the masked pixels [H,W]; "valid"; "margin"}.
    ``mask_near``: the upstream gradients are zeroed at the ``near`` pixels first (the caller zeroes the same pixels for the GPU)."""
    P, vm, I, F = forward(sc, cam, dtype, Rt, straight_through=straight_through)
    keep = (~F["near"]).to(dtype) if mask_near else torch.ones_like(F["alpha"])
    loss = torch.zeros((), dtype=dtype)
    for g, f in ((g_rgb, F["acc_rgb"]), (g_alpha, F["alpha"]), (g_depth, F["acc_z"])):
        if g is not None:
            gt = torch.as_tensor(np.asarray(g, np.float64), dtype=dtype).reshape(f.shape)
            loss = loss + (gt * (keep[..., None] if f.dim() == 3 else keep) * f).sum()
    loss.backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()
    screen = {k: z(I[k]) for k in SCREEN}
    full = dict(means=z(P["means"]), opacities=z(P["op"]), colors=z(P["colors"]), viewmat=z(vm))
    if "quats" in P:
        full.update(quats=z(P["quats"]), scales=z(P["scales"]))
    else:
        full.update(covariances=z(P["cov6"]))
    return dict(screen=screen, full=full, near=F["near"].numpy(), valid=I["valid"].numpy(), margin=I["margin"].numpy(),
                frame={k: v.detach().double().numpy() for k, v in F.items() if k != "near"})


def rel_err(g, ref):
    """max |g - ref| / max |ref| (0 when both vanish): the measure of DESIGN.md 3, "Backward pass"."""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max() if ref.size else 0.0
    d = np.abs(g.reshape(ref.shape) - ref).max() if ref.size else 0.0
    return 0.0 if d == 0.0 else d / top if top > 0 else np.inf
