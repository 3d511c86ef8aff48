"""The cases of the group-pose gradient tests (tests/test_group_pose_cpu.py, tests/test_gpu_x_group_pose_grad.py): grouped scenes, their
cameras and upstream gradients, the float64 reference of tests/tools/group_pose_ref.py per case (computed once and shared), and the
float32 reference's own error, which sets the GPU bound.  The shapes are the smallest at which the kernel can go wrong: several
workgroups, several groups per wave, a group absent from most waves, a group that is culled whole, a group whose Gaussians lie beyond
the limits of the Jacobian's clamp under an off-axis camera.  As in grad_cases.py a case masks at most
MAX_MASKED of its pixels and holds no Gaussian with a marginal projection decision; test_group_pose_cpu.py asserts both.

    python tests/tools/group_pose_cases.py      prints the F32_ERR table of tests/test_gpu_x_group_pose_grad.py"""
import functools

import numpy as np

import grad_cases as gc
import grad_ref
import group_pose_ref as gpr
import lift_ref as lr
import scene_cases as sc_kit

MAX_MASKED = gc.MAX_MASKED
SH2_SEED = 5      # chosen on the CPU: 0 marginal Gaussians after _clean, masked pixels under the cap (test_group_pose_cpu.py)
RARE_GROUP, RARE_COUNT = 4, 3
BEHIND_GROUP = 2


def _gp600():
    return gc._clean(lr.blob_scene(600, 22, 0.08, n_groups=5), sc_kit.ring(48, 32, f=0.45 * 48))


def _gp_sh2():
    sc = sc_kit.synthetic(150, SH2_SEED, 0.12)
    n = np.asarray(sc["means"]).shape[0]
    sc = dict(sc, colors=np.ascontiguousarray(np.asarray(sc["colors"])[:, :9]), sh=2, gid=(np.arange(n) % 3).astype(np.uint8), G=3,
              Rt=sc_kit.random_group_poses(3, SH2_SEED + 1))
    return gc._clean(sc, sc_kit.ring(40, 24, f=22.0, yaw=20.0, elev=0.3))


def _gp_rare():
    """gp600 with group RARE_GROUP left on its first RARE_COUNT Gaussians only: most waves skip the slot."""
    sc, cam = _gp600()
    gid = np.array(sc["gid"])
    mine = np.nonzero(gid == RARE_GROUP)[0][RARE_COUNT:]
    gid[mine] = (mine % RARE_GROUP).astype(np.uint8)
    return gc._clean(dict(sc, gid=gid), cam)


def _gp_behind():
    """gp600 with group BEHIND_GROUP posed behind the camera: two and a half times the camera's distance from the origin, on the camera's
    side (the scene's box has half width 1, the camera looks at the origin): all its Gaussians are culled."""
    sc, cam = _gp600()
    V = np.asarray(cam[0], np.float64).reshape(4, 4)
    campos = -V[:3, :3].T @ V[:3, 3]
    Rt = np.array(sc["Rt"], np.float32).reshape(-1, 12).copy()
    Rt[BEHIND_GROUP, 3::4] = (2.5 * campos).astype(np.float32)
    return gc._clean(dict(sc, Rt=Rt), cam)


BUILDERS = {
    "gp600": _gp600,
    "gp600_cov6": lambda: (gc._cov6(_gp600()[0]), _gp600()[1]),
    "gp_sh2": _gp_sh2,
    "gp_rare": _gp_rare,
    "gp_behind": _gp_behind,
    "gp_clamp": lambda: gc.BUILDERS["clamp_groups"](),   # five Gaussians of group gc.CLAMP_GROUP beyond the limits of the Jacobian's clamp
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, camera, upstream gradients g_rgb [H,W,3], g_alpha [H,W], g_depth [H,W]), drawn as grad_cases.case draws them."""
    sc, cam = BUILDERS[name]()
    W, H = cam[2], cam[3]
    rng = np.random.default_rng(2000 + NAMES.index(name.replace("_cov6", "")))   # (the two forms of one scene share their draw)
    g = (rng.normal(size=(H, W, 3)).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32),
         (0.3 * rng.normal(size=(H, W))).astype(np.float32))
    return sc, cam, g


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name="float64"):
    """group_pose_ref.gradients of the case (shared: callers do not write into it)."""
    import torch
    sc, cam, g = case(name)
    return gpr.gradients(sc, cam, *g, dtype=getattr(torch, dtype_name))


def masked_upstream(name):
    """The upstream gradients as the GPU gets them: zero at the reference's near-threshold pixels."""
    sc, cam, g = case(name)
    keep = ~reference(name)["near"]
    return [(gi * (keep[..., None] if gi.ndim == 3 else keep)).astype(np.float32) for gi in g]


@functools.lru_cache(maxsize=None)
def mutant_reference(name):
    """The full gradients from grad_ref.project's straight-through mutant (the clamp's gradient passed to x and y), same upstream gradients."""
    sc, cam, _ = case(name)
    return gpr.gradients(sc, cam, *masked_upstream(name), mask_near=False, straight_through=True)["full"]


def float32_errors(name):
    r64, r32 = reference(name)["full"], reference(name, "float32")["full"]
    return {k: grad_ref.rel_err(r32[k], r64[k]) for k in r64}


# ---- two views of one grouped scene -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_view_case():
    sc, cam = _gp600()
    return gc._clean(sc, gc.second_camera())[0], (cam, gc.second_camera())


@functools.lru_cache(maxsize=None)
def two_view_reference(dtype_name="float64"):
    """(sum of the two views' pose gradients [n_groups,3,4], [near masks], [upstream gradients])."""
    import torch
    sc, cams = two_view_case()
    gs, refs = [], []
    for v, cam in enumerate(cams):
        rng = np.random.default_rng(2077 + v)
        W, H = cam[2], cam[3]
        g = (rng.normal(size=(H, W, 3)).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32), (0.3 * rng.normal(size=(H, W))).astype(np.float32))
        gs.append(g)
        refs.append(gpr.gradients(sc, cam, *g, dtype=getattr(torch, dtype_name)))
    return dict(group_poses=refs[0]["full"]["group_poses"] + refs[1]["full"]["group_poses"]), [r["near"] for r in refs], gs


# ---- a plain L2 loss on the delivered frame, as grad_cases.l2_reference, with the poses as a variable ----------------------------------------
L2_CASE = "gp600"


@functools.lru_cache(maxsize=None)
def l2_reference(dtype_name="float64"):
    """Gradients of sum keep ((rgb - t_rgb)^2 + (alpha - t_a)^2 + 0.1 (depth - t_d)^2) over gc.L2_BACKGROUND: (group_poses and viewmat, keep, targets)."""
    import torch
    dt = getattr(torch, dtype_name)
    sc, cam, _ = case(L2_CASE)
    W, H = cam[2], cam[3]
    rng = np.random.default_rng(5)
    targets = (rng.uniform(0, 1, (H, W, 3)).astype(np.float32), rng.uniform(0, 1, (H, W)).astype(np.float32), rng.uniform(2, 4, (H, W)).astype(np.float32))
    P, G, vm, I, F = gpr.forward(sc, cam, dt)
    out = grad_ref.finish(F, gc.L2_BACKGROUND)
    keep = (~F["near"]).to(dt)
    t_rgb, t_a, t_d = [torch.as_tensor(t.astype(np.float64), dtype=dt) for t in targets]
    loss = (keep[..., None] * (out["rgb"] - t_rgb) ** 2).sum() + (keep * (out["alpha"] - t_a) ** 2).sum() + 0.1 * (keep * (out["depth"] - t_d) ** 2).sum()
    loss.backward()
    return dict(group_poses=G.grad.double().numpy(), viewmat=vm.grad.double().numpy()), keep.double().numpy(), targets


# ---- the recovery case: one group of a three-group scene displaced about its centroid, two views ----------------------------------------
RECOVER_GROUP = 1
RECOVER_TWIST = np.array([0.04, -0.035, 0.03, 0.02, -0.015, 0.018])   # 3.50 degrees, 0.031 units
RECOVER_ITERS = 64   # chosen on the CPU reference: 0.064 degrees and 6.4e-4 at the end (0.24 degrees after 40: the decaying Adam step needs its tail)
RECOVER_REF_END = (0.0635, 6.42e-4)   # (degrees, units) where the float64 reference run ends: test_group_pose_cpu.py holds this to the run


def recovery_case():
    """(scene, [cameras], true poses [3,3,4] float64, displaced poses, pivot [1,3]): group RECOVER_GROUP turned and shifted about its
    posed centroid by RECOVER_TWIST."""
    from sim_a_splat_amd.register import se3_exp
    sc = lr.blob_scene(240, 31, 0.10, n_groups=3)
    cams = [sc_kit.ring(40, 24, f=0.45 * 40, yaw=0.0, elev=0.2), sc_kit.ring(40, 24, f=0.45 * 40, yaw=75.0, elev=0.3)]
    true = np.asarray(sc["Rt"], np.float64).reshape(-1, 3, 4)
    m = np.asarray(sc["means"], np.float64)[np.asarray(sc["gid"]) == RECOVER_GROUP]
    pivot = (true[RECOVER_GROUP, :, :3] @ m.T).T.mean(axis=0) + true[RECOVER_GROUP, :, 3]
    Tp = np.eye(4)
    Tp[:3, 3] = pivot
    G4 = np.eye(4)
    G4[:3] = true[RECOVER_GROUP]
    start = true.copy()
    start[RECOVER_GROUP] = (Tp @ se3_exp(RECOVER_TWIST) @ np.linalg.inv(Tp) @ G4)[:3]
    return sc, cams, true, start, pivot.reshape(1, 3)


def pose_error(G_est, G_true, pivot):
    """(angle in degrees, distance between the images of ``pivot``'s canonical point) between two poses [3,4] of one group."""
    A, B = np.asarray(G_est, np.float64).reshape(3, 4), np.asarray(G_true, np.float64).reshape(3, 4)
    D = A[:, :3] @ B[:, :3].T
    p0 = B[:, :3].T @ (np.asarray(pivot, np.float64).reshape(3) - B[:, 3])   # the canonical point the true pose sends to the pivot
    ang = float(np.degrees(np.arccos(np.clip((np.trace(D) - 1.0) / 2.0, -1.0, 1.0))))
    return ang, float(np.linalg.norm(A[:, :3] @ p0 + A[:, 3] - np.asarray(pivot, np.float64).reshape(3)))


if __name__ == "__main__":   # the table of tests/test_gpu_x_group_pose_grad.py
    for name in NAMES:
        print(f'    "{name}": dict(' + ", ".join(f"{k}={v:.2e}" for k, v in float32_errors(name).items()) + "),")
    a, b = reference("gp_rare")["full"]["group_poses"][RARE_GROUP], reference("gp_rare", "float32")["full"]["group_poses"][RARE_GROUP]
    print(f'    "gp_rare_row": dict(group_poses={grad_ref.rel_err(b, a):.2e}),')
    a, b = two_view_reference()[0], two_view_reference("float32")[0]
    print('    "two_views": dict(' + ", ".join(f"{k}={grad_ref.rel_err(b[k], a[k]):.2e}" for k in a) + "),")
    a, b = l2_reference()[0], l2_reference("float32")[0]
    print('    "l2": dict(' + ", ".join(f"{k}={grad_ref.rel_err(b[k], a[k]):.2e}" for k in a) + "),")
