"""The cases of the optimiser-step tests (tests/test_fit_cpu.py, tests/test_gpu_u_fit.py): small scenes, drawn gradients, the float32
restatement's error against float64, and the fit case with its CPU stand-in renderer.

    python tests/tools/fit_cases.py        prints F32_ERR as it stands today

Every scene has N = 200 Gaussians (no multiple of 64: n_pad > n) with drawn means (the storage order is no identity).  The gradients of
a case are drawn per step: magnitudes log-uniform in [1e-4, 1], random signs, float32."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(Path(__file__).resolve().parent)):
    if p not in sys.path:
        sys.path.insert(0, p)
import fit_ref  # noqa: E402
import grad_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

N = 200
STEPS = 20
LRS = dict(means=1.6e-3, opacities=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4, quats=1e-3, scales=5e-3)
# name -> (sh_degree, groups, covariance form): the colour block is 3, 12, 27 and 48 floats (the plane tail), 12 with groups / cov6
CASES = {"rgb": (-1, 0, "quats"), "sh1": (1, 0, "quats"), "sh2": (2, 0, "quats"), "sh3": (3, 0, "quats"), "groups3": (1, 3, "quats"),
         "cov6": (1, 0, "cov6")}
NAMES = tuple(CASES)
CAMERA = dict(W=48, H=40, f=45.0, yaw=20.0, elev=0.25)   # (H ragged: 2.5 tiles)
BACKGROUND = (0.1, 0.2, 0.3)

# max |x32 - x64| / max |x64| after STEPS steps, per case and variable group: fit_ref in float32 against float64 (float32_errors below;
# tests/test_fit_cpu.py holds the table to it).  The GPU test's bounds are four times these.
F32_ERR = {
    "rgb": dict(means=2.96e-07, opacities=8.30e-08, colors=2.57e-07, quats=2.87e-07, scales=7.08e-07),
    "sh1": dict(means=2.09e-07, opacities=9.34e-08, colors=2.94e-07, quats=1.97e-07, scales=1.11e-06),
    "sh2": dict(means=2.37e-07, opacities=9.56e-08, colors=2.71e-07, quats=2.02e-07, scales=7.70e-07),
    "sh3": dict(means=1.77e-07, opacities=7.88e-08, colors=3.24e-07, quats=2.85e-07, scales=8.79e-07),
    "groups3": dict(means=1.45e-07, opacities=9.47e-08, colors=3.32e-07, quats=2.13e-07, scales=7.49e-07),
    "cov6": dict(means=2.40e-07, opacities=8.90e-08, colors=2.34e-07),
}


def _seed(name):
    return 100 + NAMES.index(name)


def scene(name):
    """The case's scene in scene_cases' dict form."""
    deg, G, form = CASES[name]
    rng = np.random.default_rng(_seed(name))
    kk = (deg + 1) ** 2 if deg >= 0 else 1
    means = rng.normal(0.0, 0.45, (N, 3)).astype(np.float32)
    quats = rng.normal(size=(N, 4)).astype(np.float32)
    scales = rng.uniform(0.03, 0.12, (N, 3)).astype(np.float32)
    op = rng.uniform(0.05, 0.95, N).astype(np.float32)
    colors = rng.normal(0.0, 0.3, (N, kk, 3)).astype(np.float32)
    colors[:, 0] += 0.5 if deg < 0 else 0.4
    sc = dict(means=means, op=op, colors=colors if deg >= 0 else colors.reshape(N, 3), sh=deg, quats=quats, scales=scales, cov6=None, gid=None, G=0, Rt=None)
    if G:
        sc.update(gid=rng.integers(0, G, N).astype(np.uint8), G=G, Rt=sc_kit.random_group_poses(G, _seed(name)))
    if form == "cov6":
        R = grad_ref.quat_to_rotmat(torch.tensor(quats.astype(np.float64))).numpy()
        M = R * scales.astype(np.float64)[:, None, :]
        S = M @ M.transpose(0, 2, 1)
        sc.update(cov6=np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32), quats=None, scales=None)
    return sc


def ref_scene(sc):
    """scene_cases' dict as fit_ref.new_state takes it."""
    n = np.asarray(sc["means"]).shape[0]
    return dict(means=sc["means"], opacities=sc["op"], colors=np.asarray(sc["colors"]).reshape(n, -1, 3), quats=sc["quats"], scales=sc["scales"])


def groups_of(name):
    return ("means", "opacities", "colors") + (("quats", "scales") if CASES[name][2] == "quats" else ())


def draw_gradients(name, steps=STEPS, seed_offset=0, n=N):
    """[steps] dicts of float32 gradients under render_backward's keys, in the shapes it returns."""
    rng = np.random.default_rng(1000 + _seed(name) + seed_offset)
    deg = CASES[name][0]
    kk = (deg + 1) ** 2 if deg >= 0 else 1
    shapes = dict(means=(n, 3), opacities=(n,), colors=(n, kk, 3), quats=(n, 4), scales=(n, 3))
    out = []
    for _ in range(steps):
        out.append({k: (10.0 ** rng.uniform(-4.0, 0.0, shapes[k]) * rng.choice([-1.0, 1.0], shapes[k])).astype(np.float32) for k in groups_of(name)})
    return out


_RUNS = {}


def reference(name, dtype=np.float64):
    """fit_ref's state after STEPS steps of the case (computed once per dtype, never changed)."""
    key = (name, np.dtype(dtype).name)
    if key not in _RUNS:
        _RUNS[key] = fit_ref.run(ref_scene(scene(name)), draw_gradients(name), LRS, dtype)
    return _RUNS[key]


def float32_errors(name):
    a, b = reference(name)["x"], reference(name, np.float32)["x"]
    return {k: fit_ref.rel_err(b[k], a[k]) for k in groups_of(name)}


def camera():
    c = CAMERA
    return sc_kit.ring(c["W"], c["H"], f=c["f"], yaw=c["yaw"], elev=c["elev"])


# ---- the fit case: a scene whose colours were tinted and opacities scaled, recovered from frames of the true scene ---------------------
FIT = dict(n=150, W=48, H=40, views=4, iters=40, views_per_step=2, what=("colors", "opacities"),
           lrs=dict(sh_dc=3e-2, sh_rest=3e-3, opacities=5e-2))
FIT_BACKGROUND = (0.0, 0.0, 0.0)


def fit_case():
    """(true scene, perturbed scene, viewmats [C,4,4], Ks [C,3,3], W, H)."""
    rng = np.random.default_rng(77)
    n = FIT["n"]
    means = rng.normal(0.0, 0.4, (n, 3)).astype(np.float32)
    colors = rng.normal(0.0, 0.08, (n, 4, 3)).astype(np.float32)
    colors[:, 0] = rng.uniform(-0.8, 1.2, (n, 3))
    true = dict(means=means, op=rng.uniform(0.4, 0.9, n).astype(np.float32), colors=colors, sh=1, quats=rng.normal(size=(n, 4)).astype(np.float32),
                scales=rng.uniform(0.05, 0.12, (n, 3)).astype(np.float32), cov6=None, gid=None, G=0, Rt=None)
    tint = np.array([0.5, -0.4, 0.3], np.float32)
    start = dict(true, colors=(colors * np.float32(0.6) + np.concatenate([tint[None, None], np.zeros((1, 3, 3), np.float32)], axis=1)).astype(np.float32),
                 op=(true["op"] * np.float32(0.6)).astype(np.float32))
    cams = [sc_kit.ring(FIT["W"], FIT["H"], f=42.0, yaw=90.0 * k + 10.0, elev=0.2 + 0.1 * k) for k in range(FIT["views"])]
    return true, start, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), FIT["W"], FIT["H"]


class RefRenderer:
    """The three methods fit_scene uses, on the float64 references: grad_ref renders and differentiates, fit_ref steps."""

    def __init__(self, sc):
        self.sc = dict(sc)
        self.S = fit_ref.new_state(ref_scene(sc), np.float64)
        self._last = None

    def _scene(self):
        x = self.S["x"]
        return dict(self.sc, means=x["means"], op=x["opacities"], colors=x["colors"], quats=x["quats"], scales=x["scales"])

    def render(self, V, K, W, H, background=(0.0, 0.0, 0.0), **kw):
        P, vm, I, F = grad_ref.forward(self._scene(), (V, K, W, H))
        self._last = (np.asarray(V).tobytes(), P, F)
        out = grad_ref.finish({k: v.detach() for k, v in F.items() if k != "near"}, background)
        return dict(rgb=out["rgb"], alpha=out["alpha"][..., None], depth=out["depth"][..., None])

    def render_backward(self, V, K, W, H, g_rgb=None, g_alpha=None, g_depth=None, *, out=None, want=None, **kw):
        if self._last is None or self._last[0] != np.asarray(V).tobytes():
            self.render(V, K, W, H)
        _, P, F = self._last
        self._last = None
        loss = sum((g.double().reshape(f.shape) * f).sum() for g, f in ((g_rgb, F["acc_rgb"]), (g_alpha, F["alpha"]), (g_depth, F["acc_z"])) if g is not None)
        loss.backward()
        names = dict(means="means", opacities="op", colors="colors", quats="quats", scales="scales")
        res = dict(out or {})
        for k in (want or names):
            g = P[names[k]].grad
            g = torch.zeros_like(P[names[k]]) if g is None else g
            res[k] = g.detach().clone() if res.get(k) is None else res[k] + g.detach()
        return res

    def adam_step(self, grads, lrs, step, betas=(0.9, 0.999), eps=1e-15, visible_only=False):
        fit_ref.step(self.S, {k: v.numpy() for k, v in grads.items()}, lrs, step, betas, eps, visible_only)

    def read_scene(self):
        return {k: torch.tensor(v) for k, v in self.S["x"].items()}


def fit_targets(true, V, K, W, H):
    """Frames [C,H,W,3] float32 of the true scene from the float64 reference."""
    R = RefRenderer(true)
    with torch.no_grad():
        return np.stack([R.render(V[c], K[c], W, H, FIT_BACKGROUND)["rgb"].numpy() for c in range(len(V))]).astype(np.float32)


if __name__ == "__main__":
    print("F32_ERR = {")
    for name in NAMES:
        print(f'    "{name}": dict(' + ", ".join(f"{k}={v:.2e}" for k, v in float32_errors(name).items()) + "),")
    print("}")
