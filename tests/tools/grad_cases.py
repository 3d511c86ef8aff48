"""The cases of the backward-pass tests (tests/test_grad_cpu.py, tests/test_gpu_t_backward.py): scene, camera and upstream gradients per
name.  Seeds and scene parameters were chosen on the CPU (tests/tools/grad_ref.py) so that at most 2 % of a case's pixels are masked, and a
drawn Gaussian whose projection-level decision (near / far and opacity culls, the radius' ceil, the rectangle against the image, the
Jacobian's clamp) lies within grad_ref.MARGIN of its threshold is rejected from the draw (``_clean``: such a decision depends on the
Gaussian and the camera alone); test_grad_cpu.py asserts both conditions for every case as the tests use it.  Most cases stand under
scene_cases.ring (fx = fy, centred principal point, no roll); "offaxis" and the "clamp*" cases stand under scene_cases.general."""
import functools

import numpy as np

import grad_ref
import lift_ref as lr
import scene_cases as sc_kit

MAX_MASKED = 0.02


def _cov6(sc):
    """The scene's covariances in the world frame, in place of its quaternions and scales."""
    q = np.asarray(sc["quats"], np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * np.asarray(sc["scales"], np.float64)[:, None, :]
    C = M @ M.transpose(0, 2, 1)
    out = dict(sc)
    out.update(quats=None, scales=None, cov6=np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1).astype(np.float32))
    return out


def _clean(sc, cam):
    """The scene without the Gaussians whose projection-level decisions are marginal for this camera."""
    import torch
    with torch.no_grad():
        P = grad_ref.leaves(sc)
        vm = torch.tensor(np.asarray(cam[0], np.float64).reshape(4, 4)[:3])
        gid = sc.get("gid")
        keep = ~grad_ref.project(P, vm, cam[1], cam[2], cam[3], sc["sh"], gid, sc.get("Rt") if gid is not None else None)["margin"].numpy()
    pick = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[keep])
    return dict(sc, **{k: pick(sc[k]) for k in ("means", "op", "colors", "quats", "scales", "cov6", "gid")}), cam


def _blob(W, H, seed=11, n_groups=0):
    return _clean(lr.blob_scene(64, seed, 0.12, n_groups=n_groups), sc_kit.ring(W, H, f=0.45 * max(W, H)))


def _sh(degree, seed=5):
    sc = sc_kit.synthetic(150, seed, 0.12)
    if degree < sc["sh"]:
        kk = (degree + 1) ** 2
        sc = dict(sc, colors=np.ascontiguousarray(np.asarray(sc["colors"])[:, :kk]), sh=degree)
    return _clean(sc, sc_kit.ring(40, 24, f=22.0, yaw=20.0, elev=0.3))


CLAMP_PIXEL = (16, 16)   # (x, y) of the pixel the clamped Gaussian of "special" is centred on
CLAMP_DEPTH = 1.0        # its camera depth: in front of every Gaussian of the blob (those lie 3 - sqrt(3) = 1.27 or more from the camera)


def _special(seed=11):
    """The blob scene plus: one Gaussian behind the camera, one below the opacity cull, and one of opacity 1 centred on the pixel
    CLAMP_PIXEL in front of everything (o e^-sigma = 1 > 0.999 there: its alpha is clamped at that pixel).  Its world position is the
    pixel's centre unprojected at CLAMP_DEPTH through the inverse of the case's own view matrix."""
    sc, cam = _blob(32, 32, seed)
    V, K = np.asarray(cam[0], np.float64).reshape(4, 4), np.asarray(cam[1], np.float64).reshape(3, 3)
    R, t = V[:3, :3], V[:3, 3]
    to_world = lambda pc: R.T @ (np.asarray(pc, np.float64) - t)
    centre = np.array([(CLAMP_PIXEL[0] + 0.5 - K[0, 2]) / K[0, 0], (CLAMP_PIXEL[1] + 0.5 - K[1, 2]) / K[1, 1], 1.0]) * CLAMP_DEPTH
    extra = np.stack([to_world([0.3, 0.1, -2.0]), to_world([0.1, -0.2, 2.8]), to_world(centre)]).astype(np.float32)
    cat = lambda a, b: np.concatenate([np.asarray(a), np.asarray(b, np.float32)], 0)
    sc = dict(sc, means=cat(sc["means"], extra), op=cat(sc["op"], [0.9, 0.002, 1.0]),
              colors=cat(sc["colors"], [[0.2, 0.4, 0.6]] * 3), quats=cat(sc["quats"], [[1, 0, 0, 0]] * 3),
              scales=cat(sc["scales"], [[0.1, 0.1, 0.1]] * 3))
    return sc, cam


def _dense(seed=8):
    """About 2 000 Gaussians at 48x48: every tile's list spans several staged batches of 256, and half the pixels stop at T <= 1e-4."""
    return _clean(lr.blob_scene(2000, seed, 0.08, spread=1.0, z_spread=0.5, op=(0.7, 0.99)), sc_kit.ring(48, 48, f=54.0, yaw=0.0, elev=0.0))


# ---- an off-axis camera, and Gaussians beyond the limits of the Jacobian's clamp -----------------------------------------------------------
OFFAXIS = dict(W=40, H=28, fx=20.0, fy=15.0, cx=14.0, cy=17.0, eye=(0.6, 0.5, 2.6), target=(0.1, -0.1, 0.0), roll_deg=25.0)
CLAMP_Z, CLAMP_OVER, CLAMP_OPACITY = 0.9, 1.04, 0.8   # the extras: camera depth, x/z or y/z over the limit, opacity ...
CLAMP_SCALE = (0.16, 0.13, 0.17)                     # ... and scales: not quite round, so that their quaternions receive too (chosen on the
#                                                      CPU among a few triples: no marginal Gaussian in any of the three cases)
CLAMP = dict(x_pos=-5, x_neg=-4, y_pos=-3, y_neg=-2, corner=-1)         # indices of the extra Gaussians of the "clamp*" cases
CLAMP_NAMES = ("clamp", "clamp_cov6", "clamp_groups")
CLAMP_GROUP = 1                                                          # the (posed) group the extras of "clamp_groups" belong to


def clamp_limits(cam):
    """(x_pos, x_neg, y_pos, y_neg): the bounds on x/z and y/z beyond which the Jacobian's tx / ty are clamped (oracle/np_twin.py)."""
    _, K, W, H = cam
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return ((W - cx) / fx + 0.15 * W / fx, cx / fx + 0.15 * W / fx, (H - cy) / fy + 0.15 * H / fy, cy / fy + 0.15 * H / fy)


def _offaxis(n_groups=0):
    """The blob under a camera with fx != fy, an off-centre principal point and roll; no Gaussian reaches a clamp limit."""
    return _clean(lr.blob_scene(64, 11, 0.12, n_groups=n_groups), sc_kit.general(**OFFAXIS))


def _clamp(n_groups=0):
    """"offaxis" plus five Gaussians close to the lens, each at a camera-frame point (u_x z, u_y z, z) unprojected through the inverse of
    the case's own view matrix: one beyond each of the four limits by the factor CLAMP_OVER, the fifth beyond two at once (CLAMP names
    them).  With groups the five belong to group CLAMP_GROUP and are placed through the inverse of its pose as well: they land there
    AFTER posing."""
    sc, cam = _offaxis(n_groups)
    V = np.asarray(cam[0], np.float64).reshape(4, 4)
    xp, xn, yp, yn = clamp_limits(cam)
    f, z = CLAMP_OVER, CLAMP_Z
    ratios = [(f * xp, 0.15), (-f * xn, -0.1), (0.2, f * yp), (-0.15, -f * yn), (f * xp, -f * yn)]
    world = np.array([V[:3, :3].T @ (np.array([ux * z, uy * z, z]) - V[:3, 3]) for ux, uy in ratios])
    cat = lambda a, b: np.concatenate([np.asarray(a), np.asarray(b, np.asarray(a).dtype)], 0)
    if n_groups:
        G = np.asarray(sc["Rt"], np.float64).reshape(-1, 3, 4)[CLAMP_GROUP]
        world = (world - G[:, 3]) @ G[:, :3]   # the canonical point m with Rg m + t = world
        sc = dict(sc, gid=cat(sc["gid"], [CLAMP_GROUP] * 5))
    sc = dict(sc, means=cat(sc["means"], world), op=cat(sc["op"], [CLAMP_OPACITY] * 5),
              colors=cat(sc["colors"], [[0.9, 0.3, 0.2], [0.2, 0.8, 0.3], [0.3, 0.4, 0.9], [0.8, 0.8, 0.2], [0.6, 0.2, 0.7]]),
              quats=cat(sc["quats"], [[1, 0, 0, 0]] * 5), scales=cat(sc["scales"], [CLAMP_SCALE] * 5))
    return sc, cam


BUILDERS = {
    "blob_32x32": lambda: _blob(32, 32),
    "blob_40x24": lambda: _blob(40, 24),
    "blob_17x33": lambda: _blob(17, 33),
    "dense_48x48": _dense,
    "sh0": lambda: _sh(0),
    "sh2": lambda: _sh(2),
    "sh3": lambda: _sh(3),
    "cov6": lambda: (_cov6(_blob(40, 24)[0]), _blob(40, 24)[1]),
    "groups3": lambda: _blob(40, 24, n_groups=3),
    "special": _special,
}
BUILDERS["two_views"] = lambda: _two_views()   # (not a case of its own: the scene of two_view_reference)
BUILDERS.update({                              # (behind it: a case's upstream gradients are drawn from its place in this table)
    "offaxis": _offaxis,
    "clamp": _clamp,
    "clamp_cov6": lambda: (_cov6(_clamp()[0]), _clamp()[1]),
    "clamp_groups": lambda: _clamp(n_groups=3),
})
NAMES = tuple(n for n in BUILDERS if n != "two_views")
SPECIAL = dict(behind=-3, transparent=-2, clamped=-1)   # indices of the extra Gaussians of "special"


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, camera, upstream gradients g_rgb [H,W,3], g_alpha [H,W], g_depth [H,W])."""
    sc, cam = BUILDERS[name]()
    W, H = cam[2], cam[3]
    rng = np.random.default_rng(1000 + list(BUILDERS).index(name))
    g = (rng.normal(size=(H, W, 3)).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32),
         (0.3 * rng.normal(size=(H, W))).astype(np.float32))
    return sc, cam, g


@functools.lru_cache(maxsize=None)
def reference(name, which=(True, True, True), dtype_name="float64"):
    """grad_ref.gradients of the case (computed once per session and shared: callers do not write into it)."""
    import torch
    sc, cam, g = case(name)
    pick = [gi if w else None for gi, w in zip(g, which)]
    return grad_ref.gradients(sc, cam, *pick, dtype=getattr(torch, dtype_name))


def masked_upstream(name, which=(True, True, True)):
    """The upstream gradients as the GPU gets them: zero at the reference's near-threshold pixels."""
    sc, cam, g = case(name)
    keep = ~reference(name, which)["near"]
    return [None if not w else (gi * (keep[..., None] if gi.ndim == 3 else keep)).astype(np.float32) for gi, w in zip(g, which)]


# ---- what the new cases are measured with: mutants of the reference, and the clamped Gaussians held alone ----------------------------------
MUTANTS = ("straight_through", "swap_f", "centred")


@functools.lru_cache(maxsize=None)
def mutant_reference(name, kind):
    """The full gradients of the case, same masked upstream gradients, from a reference that is wrong in one way: ``straight_through``
    (grad_ref.project's mutant: the clamp's gradient goes to x and y), ``swap_f`` (fx and fy exchanged in K), ``centred`` (the principal
    point at the image's centre).  A case counts only if these are far from the reference (test_grad_cpu.py)."""
    sc, (V, K, W, H), _ = case(name)
    K = np.array(K, np.float64).reshape(3, 3)
    if kind == "swap_f":
        K[0, 0], K[1, 1] = K[1, 1], K[0, 0]
    if kind == "centred":
        K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    return grad_ref.gradients(sc, (V, K, W, H), *masked_upstream(name), mask_near=False, straight_through=kind == "straight_through")["full"]


EXTRA_ROWS = ("means", "quats", "scales")


@functools.lru_cache(maxsize=None)
def extras_upstream():
    """The masked upstream gradients of "clamp", zeroed outside the five extras' rectangles (means2d +- radii of the reference): what the
    extras' rows receive is then no smaller than anything else in the arrays."""
    import torch
    sc, cam, _ = case("clamp")
    W, H = cam[2], cam[3]
    with torch.no_grad():
        I = grad_ref.forward(sc, cam)[2]
    m2, rad = I["means2d"].numpy(), I["radii"].numpy()
    px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    inside = np.zeros((H, W), bool)
    for i in CLAMP.values():
        inside |= (np.abs(px - m2[i, 0]) <= rad[i, 0]) & (np.abs(py - m2[i, 1]) <= rad[i, 1])
    return tuple((gi * (inside[..., None] if gi.ndim == 3 else inside)).astype(np.float32) for gi in masked_upstream("clamp")), inside


@functools.lru_cache(maxsize=None)
def extras_reference(dtype_name="float64"):
    """The extras' rows (in CLAMP's order) of EXTRA_ROWS of the full gradients of "clamp" under extras_upstream."""
    import torch
    sc, cam, _ = case("clamp")
    full = grad_ref.gradients(sc, cam, *extras_upstream()[0], dtype=getattr(torch, dtype_name), mask_near=False)["full"]
    return {k: full[k][list(CLAMP.values())] for k in EXTRA_ROWS}


# ---- two views of one scene, and a plain L2 loss on the delivered frame ---------------------------------------------------------------
def second_camera():
    return sc_kit.ring(32, 32, f=0.45 * 32, yaw=70.0, elev=0.4)


def _two_views():
    sc, cam = _blob(32, 32)
    return _clean(sc, second_camera())[0], cam


@functools.lru_cache(maxsize=None)
def two_view_reference(dtype_name="float64"):
    """(sum of the two views' full gradients, [near mask of view 0, of view 1]); each view has its own upstream gradients."""
    import torch
    sc, cam, g = case("two_views")
    rng = np.random.default_rng(77)
    g2 = (rng.normal(size=g[0].shape).astype(np.float32), rng.normal(size=g[1].shape).astype(np.float32), (0.3 * rng.normal(size=g[2].shape)).astype(np.float32))
    a = grad_ref.gradients(sc, cam, *g, dtype=getattr(torch, dtype_name))
    b = grad_ref.gradients(sc, second_camera(), *g2, dtype=getattr(torch, dtype_name))
    return {k: a["full"][k] + b["full"][k] for k in a["full"] if k != "viewmat"}, [a["near"], b["near"]], [g, g2]


L2_BACKGROUND = (0.1, 0.3, 0.2)
L2_KEYS = {"l2": "blob_40x24", "l2:clamp": "clamp"}   # the rows of the float32 table and their cases


@functools.lru_cache(maxsize=None)
def l2_target(name):
    sc, cam, g = case(name)
    rng = np.random.default_rng(5)
    W, H = cam[2], cam[3]
    return rng.uniform(0, 1, (H, W, 3)).astype(np.float32), rng.uniform(0, 1, (H, W)).astype(np.float32), rng.uniform(2, 4, (H, W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def l2_reference(name, dtype_name="float64"):
    """Full gradients of sum keep ((rgb - t_rgb)^2 + (alpha - t_a)^2 + 0.1 (depth - t_d)^2) on the DELIVERED frame over L2_BACKGROUND;
    ``keep`` zeroes the near-threshold pixels.  Returns (gradients, keep [H,W])."""
    import torch
    dt = getattr(torch, dtype_name)
    sc, cam, _ = case(name)
    P, vm, I, F = grad_ref.forward(sc, cam, dt)
    out = grad_ref.finish(F, L2_BACKGROUND)
    keep = (~F["near"]).to(dt)
    t_rgb, t_a, t_d = [torch.as_tensor(t.astype(np.float64), dtype=dt) for t in l2_target(name)]
    loss = (keep[..., None] * (out["rgb"] - t_rgb) ** 2).sum() + (keep * (out["alpha"] - t_a) ** 2).sum() + 0.1 * (keep * (out["depth"] - t_d) ** 2).sum()
    loss.backward()
    res = dict(means=P["means"].grad, opacities=P["op"].grad, colors=P["colors"].grad, viewmat=vm.grad, quats=P["quats"].grad, scales=P["scales"].grad)
    return {k: v.double().numpy() for k, v in res.items()}, keep.double().numpy()


MODES = {"all": (True, True, True), "rgb": (True, False, False), "alpha": (False, True, False), "depth": (False, False, True)}
RUNS = tuple((n, "all") for n in NAMES) + tuple(("blob_32x32", m) for m in ("rgb", "alpha", "depth"))


def float32_errors(name, mode="all"):
    """grad_ref.rel_err of the reference evaluated in torch float32 against float64, per output array: {"screen": {..}, "full": {..}}."""
    r64, r32 = reference(name, MODES[mode]), reference(name, MODES[mode], "float32")
    return {part: {k: grad_ref.rel_err(r32[part][k], r64[part][k]) for k in r64[part]} for part in ("screen", "full")}


# ---- the pose-refinement case: a perturbed camera of a 2 000-Gaussian scene at 64x64 --------------------------------------------------------
POSE_ANGLE_DEG, POSE_SHIFT = 3.0, 0.03


def pose_case():
    """(scene, camera, twist xi): the camera se3_exp(xi) V is 3 degrees and 3 cm (of its centre: |v| = 0.03 about the camera) off V."""
    sc = lr.blob_scene(2000, 21, 0.06, spread=1.0, z_spread=0.5, op=(0.5, 0.95))
    cam = sc_kit.ring(64, 64, f=72.0, yaw=10.0, elev=0.2)
    xi = np.array([0.6, -0.7, 0.4, 0.5, -0.4, 0.77])
    xi[:3] *= np.deg2rad(POSE_ANGLE_DEG) / np.linalg.norm(xi[:3])
    xi[3:] *= POSE_SHIFT / np.linalg.norm(xi[3:])
    return sc, cam, xi


def pose_case_offaxis():
    """pose_case's scene and twist under a camera at the same place with fx != fy, its principal point a fifth of the image off the
    centre in x and in y (12.8 of 64 pixels each) and 15 degrees of roll, aimed so that the scene's centre still falls on the image's
    centre.  Chosen on the CPU: the loss falls monotonically along the twist at all three pyramid levels (test_grad_cpu.py)."""
    sc, _, xi = pose_case()
    yaw = np.deg2rad(10.0)
    cam = sc_kit.general(64, 64, 72.0, 60.0, 44.8, 19.2, (3.0 * np.sin(yaw), 0.2, 3.0 * np.cos(yaw)), (0.34, 0.75, -0.1), 15.0)
    return sc, cam, xi


def pose_error(V_est, V_true):
    """(angle in degrees, distance between the camera centres) between two world -> camera matrices."""
    A, B = np.asarray(V_est, np.float64).reshape(4, 4), np.asarray(V_true, np.float64).reshape(4, 4)
    D = A @ np.linalg.inv(B)
    centre = lambda M: -M[:3, :3].T @ M[:3, 3]
    return float(np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))), float(np.linalg.norm(centre(A) - centre(B)))


if __name__ == "__main__":   # the table of profiles/render_backward.txt and of tests/test_gpu_t_backward.py
    for name, mode in RUNS:
        e = float32_errors(name, mode)
        print(f'    "{name}:{mode}": dict(screen=dict(' + ", ".join(f"{k}={v:.2e}" for k, v in e["screen"].items()) + "),")
        print("        full=dict(" + ", ".join(f"{k}={v:.2e}" for k, v in e["full"].items()) + ")),")
    a, b = two_view_reference()[0], two_view_reference("float32")[0]
    print('    "two_views": dict(' + ", ".join(f"{k}={grad_ref.rel_err(b[k], a[k]):.2e}" for k in a) + "),")
    for key, name in L2_KEYS.items():
        a, b = l2_reference(name)[0], l2_reference(name, "float32")[0]
        print(f'    "{key}": dict(' + ", ".join(f"{k}={grad_ref.rel_err(b[k], a[k]):.2e}" for k in a) + "),")
    a, b = extras_reference(), extras_reference("float32")
    print('    "clamp:extras": dict(' + ", ".join(f"{k}={grad_ref.rel_err(b[k], a[k]):.2e}" for k in a) + "),")
