"""GPU: the backward pass (sas_render_backward_screen / sas_render_backward, Rasterizer.render_backward, autograd.render_differentiable;
DESIGN.md 3, "Backward pass") against tests/tools/grad_ref.py, the float64 torch restatement of oracle/np_twin.py under autograd.

Measure per output array: max |g - g_ref| / max |g_ref| (grad_ref.rel_err).  Bound: FOUR times the same measure of the reference
evaluated in torch float32 on the CPU against float64, on the same case -- F32_ERR below, the table of profiles/render_backward.txt
(python tests/tools/grad_cases.py prints it).  Where the float32 reference is exact (an array that receives nothing) the bound is 0.
Upstream gradients are zero at the pixels the reference reports as near a decision threshold (grad_cases.masked_upstream)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, autograd
from sim_a_splat_amd.rasterizer import SasError

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import grad_cases as gc  # noqa: E402
import grad_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

# profiles/render_backward.txt, column "float32 reference"; tests/test_grad_cpu.py holds the table to what grad_cases computes today
F32_ERR = {
    "blob_32x32:all": dict(screen=dict(means2d=5.55e-07, conics=1.08e-06, opacities=7.51e-07, colors=5.54e-07, depths=4.07e-07),
        full=dict(means=5.80e-07, opacities=7.51e-07, colors=5.54e-07, viewmat=2.99e-07, quats=1.21e-06, scales=6.98e-07)),
    "blob_40x24:all": dict(screen=dict(means2d=6.38e-07, conics=1.08e-06, opacities=1.51e-06, colors=8.93e-07, depths=6.59e-07),
        full=dict(means=5.12e-07, opacities=1.51e-06, colors=8.93e-07, viewmat=4.61e-07, quats=7.68e-07, scales=6.72e-07)),
    "blob_17x33:all": dict(screen=dict(means2d=4.80e-07, conics=9.05e-07, opacities=2.55e-07, colors=7.01e-07, depths=7.19e-07),
        full=dict(means=4.66e-07, opacities=2.55e-07, colors=7.01e-07, viewmat=4.05e-07, quats=5.90e-07, scales=1.29e-06)),
    "dense_48x48:all": dict(screen=dict(means2d=1.55e-06, conics=6.48e-07, opacities=8.69e-07, colors=7.60e-07, depths=6.44e-07),
        full=dict(means=1.52e-06, opacities=8.69e-07, colors=7.60e-07, viewmat=2.65e-07, quats=1.24e-06, scales=6.69e-07)),
    "sh0:all": dict(screen=dict(means2d=1.56e-06, conics=9.69e-07, opacities=3.43e-07, colors=9.81e-07, depths=4.50e-07),
        full=dict(means=9.26e-07, opacities=3.43e-07, colors=9.72e-07, viewmat=8.40e-07, quats=2.21e-06, scales=1.11e-06)),
    "sh2:all": dict(screen=dict(means2d=5.55e-07, conics=5.66e-07, opacities=5.38e-07, colors=4.68e-07, depths=5.17e-07),
        full=dict(means=7.35e-07, opacities=5.38e-07, colors=3.47e-07, viewmat=4.29e-07, quats=1.44e-06, scales=2.07e-06)),
    "sh3:all": dict(screen=dict(means2d=1.06e-06, conics=7.64e-07, opacities=8.44e-07, colors=1.21e-06, depths=5.95e-07),
        full=dict(means=1.30e-06, opacities=8.44e-07, colors=1.59e-06, viewmat=7.27e-07, quats=1.34e-06, scales=8.18e-07)),
    "cov6:all": dict(screen=dict(means2d=1.06e-06, conics=1.08e-06, opacities=4.93e-07, colors=5.35e-07, depths=1.14e-06),
        full=dict(means=1.03e-06, opacities=4.93e-07, colors=5.35e-07, viewmat=6.57e-07, covariances=1.09e-06)),
    "groups3:all": dict(screen=dict(means2d=1.18e-06, conics=1.32e-06, opacities=5.82e-07, colors=4.64e-07, depths=7.79e-07),
        full=dict(means=1.16e-06, opacities=5.82e-07, colors=4.64e-07, viewmat=1.45e-06, quats=6.66e-07, scales=7.25e-07)),
    "special:all": dict(screen=dict(means2d=1.27e-06, conics=7.40e-07, opacities=4.19e-07, colors=7.07e-07, depths=3.95e-07),
        full=dict(means=1.14e-06, opacities=4.19e-07, colors=7.07e-07, viewmat=1.12e-06, quats=7.45e-07, scales=8.21e-07)),
    "offaxis:all": dict(screen=dict(means2d=2.39e-06, conics=1.97e-06, opacities=8.42e-07, colors=1.35e-06, depths=2.78e-07),
        full=dict(means=1.64e-06, opacities=8.42e-07, colors=1.35e-06, viewmat=2.05e-06, quats=9.27e-07, scales=1.48e-06)),
    "clamp:all": dict(screen=dict(means2d=1.96e-06, conics=2.33e-07, opacities=7.60e-07, colors=9.40e-07, depths=6.27e-07),
        full=dict(means=2.28e-06, opacities=7.60e-07, colors=9.40e-07, viewmat=1.13e-06, quats=1.01e-06, scales=8.90e-07)),
    "clamp_cov6:all": dict(screen=dict(means2d=1.57e-06, conics=6.78e-07, opacities=6.65e-07, colors=1.20e-06, depths=8.37e-07),
        full=dict(means=1.60e-06, opacities=6.65e-07, colors=1.20e-06, viewmat=1.32e-06, covariances=2.18e-06)),
    "clamp_groups:all": dict(screen=dict(means2d=1.05e-06, conics=2.04e-07, opacities=4.42e-07, colors=5.69e-07, depths=6.09e-07),
        full=dict(means=6.56e-07, opacities=4.42e-07, colors=5.69e-07, viewmat=9.46e-07, quats=4.38e-07, scales=5.70e-07)),
    "blob_32x32:rgb": dict(screen=dict(means2d=5.91e-07, conics=7.05e-07, opacities=9.71e-07, colors=5.54e-07, depths=0.00e+00),
        full=dict(means=6.51e-07, opacities=9.71e-07, colors=5.54e-07, viewmat=8.56e-07, quats=9.15e-07, scales=8.36e-07)),
    "blob_32x32:alpha": dict(screen=dict(means2d=9.26e-07, conics=7.54e-07, opacities=4.60e-07, colors=0.00e+00, depths=0.00e+00),
        full=dict(means=1.04e-06, opacities=4.60e-07, colors=0.00e+00, viewmat=3.85e-07, quats=1.41e-06, scales=5.82e-07)),
    "blob_32x32:depth": dict(screen=dict(means2d=1.29e-06, conics=1.67e-06, opacities=4.97e-07, colors=0.00e+00, depths=4.07e-07),
        full=dict(means=8.81e-07, opacities=4.97e-07, colors=0.00e+00, viewmat=1.01e-06, quats=1.44e-06, scales=8.73e-07)),
    "two_views": dict(means=1.15e-06, opacities=6.57e-07, colors=1.13e-06, quats=1.16e-06, scales=7.79e-07),
    "l2": dict(means=6.79e-06, opacities=1.80e-06, colors=2.18e-07, viewmat=1.39e-06, quats=7.43e-06, scales=9.99e-06),
    "l2:clamp": dict(means=1.09e-06, opacities=1.75e-06, colors=8.65e-07, viewmat=5.84e-07, quats=1.88e-06, scales=5.02e-06),
    "clamp:extras": dict(means=6.73e-07, quats=1.01e-06, scales=8.90e-07),
}
FACTOR = 4.0


def _hold(what, got, ref, f32_err):
    """Print every figure, then hold each array to FACTOR times the float32 reference's error."""
    rows = [(k, grad_ref.rel_err(got[k], ref[k]), FACTOR * f32_err[k]) for k in ref]
    for k, e, b in rows:
        print(f"BACKWARD {what:28s} {k:12s} hip {e:.3e}  float32 ref {f32_err[k]:.3e}  bound {b:.3e}  {'ok' if e <= b else 'MISS'}")
    bad = [(k, e, b) for k, e, b in rows if not e <= b]
    assert not bad, (what, bad)


def _run(r, name, mode):
    """(screen-space result, full result) of the case on the GPU, as float64 arrays."""
    sc, cam, _ = gc.case(name)
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    g = gc.masked_upstream(name, gc.MODES[mode])
    screen = r.render_backward(V, K, W, H, *g, screen_space=True)
    full = r.render_backward(V, K, W, H, *g)
    to = lambda d: {k: v.double().cpu().numpy() for k, v in d.items()}
    return to(screen), to(full)


@pytest.mark.parametrize("name,mode", gc.RUNS, ids=[f"{n}-{m}" for n, m in gc.RUNS])
def test_case_against_reference(rasterizer, name, mode):
    ref = gc.reference(name, gc.MODES[mode])
    screen, full = _run(rasterizer, name, mode)
    key = f"{name}:{mode}"
    _hold(key + " screen", screen, ref["screen"], F32_ERR[key]["screen"])
    _hold(key + " full", full, ref["full"], F32_ERR[key]["full"])
    # a Gaussian that receives nothing in the reference (culled, or hidden behind pixels that stopped) receives exact zeros
    dead = np.all([np.all(ref["screen"][k].reshape(len(ref["valid"]), -1) == 0, axis=1) for k in grad_ref.SCREEN], axis=0)
    for part, res in (("screen", screen), ("full", full)):
        for k, v in res.items():
            if k != "viewmat":
                assert np.all(v.reshape(len(dead), -1)[dead] == 0), (part, k)
    if name == "special":
        assert dead[gc.SPECIAL["behind"]] and dead[gc.SPECIAL["transparent"]] and not dead[gc.SPECIAL["clamped"]]
    if name == "dense_48x48":
        assert (ref["valid"] & dead).sum() > 0   # entries behind pixels that stopped at T <= 1e-4


def test_clamped_alpha_passes_nothing_to_opacity_or_sigma(rasterizer):
    """Upstream gradients at ONE pixel, the one the opacity-1 Gaussian of "special" is centred on (o e^-sigma = 1 > 0.999 there, asserted
    from the reference in test_grad_cpu.py): through its clamped alpha nothing reaches its opacity, conic or mean -- exact zeros -- while its
    colour and depth take w g."""
    r = rasterizer
    sc, cam, g = gc.case("special")
    V, K, W, H = cam
    x, y = gc.CLAMP_PIXEL
    only = np.zeros((H, W), bool)
    only[y, x] = True
    gm = [(gi * (only[..., None] if gi.ndim == 3 else only)).astype(np.float32) for gi in g]
    ref = grad_ref.gradients(sc, cam, *gm, mask_near=False)
    assert not ref["near"][y, x]
    sc_kit.upload(r, sc)
    screen = {k: v.double().cpu().numpy() for k, v in r.render_backward(V, K, W, H, *gm, screen_space=True).items()}
    i = gc.SPECIAL["clamped"]
    for k in ("opacities", "means2d", "conics"):
        assert np.all(ref["screen"][k][i] == 0) and np.all(screen[k][i] == 0), (k, screen[k][i])
    assert np.all(screen["colors"][i] != 0) and screen["depths"][i] != 0
    np.testing.assert_allclose(screen["colors"][i], 0.999 * gm[0][y, x].astype(np.float64), rtol=1e-6)   # w = alpha T = 0.999 in front of everything: two float32 roundings, 1.2e-7
    behind = np.nonzero(np.any(ref["screen"]["opacities"].reshape(len(ref["valid"]), -1) != 0, axis=1))[0]
    assert len(behind) > 0 and i not in behind   # others at that pixel do receive through their (unclamped) alphas


def test_clamped_gaussians_alone(rasterizer):
    """The five Gaussians of "clamp" beyond the limits of the Jacobian's clamp, held apart from the blob: upstream gradients only inside
    their rectangles, and the measure taken over THEIR rows of means, quats and scales alone, against four times the float32 reference's
    figure on those rows -- the blob's larger gradients cannot hide a wrong branch."""
    r = rasterizer
    sc, (V, K, W, H), _ = gc.case("clamp")
    g, _ = gc.extras_upstream()
    sc_kit.upload(r, sc)
    full = r.render_backward(V, K, W, H, *g, want=gc.EXTRA_ROWS)
    rows = list(gc.CLAMP.values())
    _hold("clamp:extras", {k: full[k].double().cpu().numpy()[rows] for k in gc.EXTRA_ROWS}, gc.extras_reference(), F32_ERR["clamp:extras"])


def test_want_selects_the_outputs(rasterizer):
    """``want`` leaves the other outputs NULL to the C call: only the named keys come back, held to the reference as in the full call."""
    r = rasterizer
    name = "blob_32x32"
    sc, (V, K, W, H), _ = gc.case(name)
    ref = gc.reference(name)
    sc_kit.upload(r, sc)
    g = gc.masked_upstream(name)
    for want in (("viewmat",), ("means", "scales"), ("colors",)):
        got = r.render_backward(V, K, W, H, *g, want=want)
        assert set(got) == set(want)
        _hold(f"want={'+'.join(want)}", {k: v.double().cpu().numpy() for k, v in got.items()}, {k: ref["full"][k] for k in want},
              F32_ERR[f"{name}:all"]["full"])
    got = r.render_backward(V, K, W, H, *g, screen_space=True, want=("conics",))
    assert set(got) == {"conics"}
    _hold("want=conics", {"conics": got["conics"].double().cpu().numpy()}, {"conics": ref["screen"]["conics"]}, F32_ERR[f"{name}:all"]["screen"])
    with pytest.raises(ValueError, match="want must name"):
        r.render_backward(V, K, W, H, *g, want=("conics",))


def test_two_views_sum(rasterizer):
    r = rasterizer
    ref, nears, gs = gc.two_view_reference()
    sc, cam, _ = gc.case("two_views")
    sc_kit.upload(r, sc)
    out = None
    for (V, K, W, H), near, g in zip((cam, gc.second_camera()), nears, gs):
        keep = ~near
        gm = [(gi * (keep[..., None] if gi.ndim == 3 else keep)).astype(np.float32) for gi in g]
        out = r.render_backward(V, K, W, H, *gm, out=out)
    got = {k: v.double().cpu().numpy() for k, v in out.items() if k != "viewmat"}
    _hold("two_views", got, ref, F32_ERR["two_views"])


@pytest.mark.parametrize("key", list(gc.L2_KEYS), ids=list(gc.L2_KEYS.values()))
def test_autograd_l2_loss(rasterizer, key):
    r = rasterizer
    name = gc.L2_KEYS[key]
    sc, cam, _ = gc.case(name)
    V, K, W, H = cam
    ref, keep = gc.l2_reference(name)
    sc_kit.upload(r, sc)
    dev = r.device
    names = dict(means="means", opacities="op", colors="colors", quats="quats", scales="scales")
    params = {k: torch.tensor(np.asarray(sc[s], np.float32), device=dev, requires_grad=True) for k, s in names.items()}
    vm = torch.tensor(np.asarray(V, np.float32), device=dev, requires_grad=True)
    out = autograd.render_differentiable(r, vm, K, W, H, params=params, background=gc.L2_BACKGROUND)
    t_rgb, t_a, t_d = [torch.tensor(t, device=dev) for t in gc.l2_target(name)]
    kp = torch.tensor(keep.astype(np.float32), device=dev)
    loss = (kp[..., None] * (out["rgb"] - t_rgb) ** 2).sum() + (kp * (out["alpha"][..., 0] - t_a) ** 2).sum() + \
        0.1 * (kp * (out["depth"][..., 0] - t_d) ** 2).sum()
    keys = list(params)
    grads = torch.autograd.grad(loss, [vm] + [params[k] for k in keys])
    got = dict(viewmat=grads[0][:3].double().cpu().numpy(), **{k: g.double().cpu().numpy() for k, g in zip(keys, grads[1:])})
    _hold(key, got, ref, F32_ERR[key])


def test_refine_camera_pose_recovers(rasterizer):
    """A camera 3 degrees and 3 cm off is brought back to under a tenth of both in a fixed 300 iterations.  (That the loss falls
    monotonically from the start to the truth, with no other minimum between, is checked on the CPU reference: test_grad_cpu.py.)"""
    from sim_a_splat_amd.register import refine_camera_pose, se3_exp
    r = rasterizer
    sc, (V, K, W, H), xi = gc.pose_case()
    sc_kit.upload(r, sc)
    target = r.render(V, K, W, H)["rgb"].clone()
    V0 = se3_exp(xi) @ np.asarray(V, np.float64)
    a0, d0 = gc.pose_error(V0, V)
    res = refine_camera_pose(r, target, V0, K, W, H, iters=300)
    a1, d1 = gc.pose_error(res.viewmat, V)
    print(f"BACKWARD refine_camera_pose: {a0:.3f} deg, {d0 * 1e3:.2f} mm -> {a1:.4f} deg, {d1 * 1e3:.3f} mm; loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    assert a0 > 2.9 and d0 > 0.02
    assert a1 < 0.1 * gc.POSE_ANGLE_DEG and d1 < 0.1 * gc.POSE_SHIFT


def test_refine_camera_pose_recovers_off_axis(rasterizer):
    """The same scene, perturbation, iterations and acceptance under a camera with fx != fy, its principal point a fifth of the image off
    the centre and roll (grad_cases.pose_case_offaxis): the pyramid's rescaled K and the pose gradient hold off-axis.  (The CPU reference's
    loss falls monotonically along the twist at all three levels: test_grad_cpu.py.)"""
    from sim_a_splat_amd.register import refine_camera_pose, se3_exp
    r = rasterizer
    sc, (V, K, W, H), xi = gc.pose_case_offaxis()
    sc_kit.upload(r, sc)
    target = r.render(V, K, W, H)["rgb"].clone()
    V0 = se3_exp(xi) @ np.asarray(V, np.float64)
    a0, d0 = gc.pose_error(V0, V)
    res = refine_camera_pose(r, target, V0, K, W, H, iters=300)
    a1, d1 = gc.pose_error(res.viewmat, V)
    print(f"BACKWARD refine_camera_pose off-axis: {a0:.3f} deg, {d0 * 1e3:.2f} mm -> {a1:.4f} deg, {d1 * 1e3:.3f} mm; loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    assert a0 > 2.9 and d0 > 0.02
    assert a1 < 0.1 * gc.POSE_ANGLE_DEG and d1 < 0.1 * gc.POSE_SHIFT


def test_door_a_refine_pose():
    """GaussianSplat.refine_pose is refine_camera_pose on the model's rasterizer with camera 0's intrinsics, OpenGL poses in and out."""
    from sim_a_splat_amd.gaussian_splat import GaussianSplat, PinholeCamera, SplatModel, viewmat_from_c2w_opengl
    from sim_a_splat_amd.register import refine_camera_pose, se3_exp
    from sim_a_splat_amd.synthetic import c2w_opengl_from_viewmat
    rng = np.random.default_rng(2)
    n, W, H = 600, 48, 32
    model = SplatModel(rng.normal(0, 0.4, (n, 3)), np.log(rng.uniform(0.05, 0.12, (n, 3))), rng.normal(size=(n, 4)), rng.normal(size=(n, 3)),
                       rng.normal(0, 0.1, (n, 15, 3)), rng.normal(0.5, 1.5, (n, 1)))
    V, K, _, _ = sc_kit.ring(W, H, f=40.0, yaw=30.0, elev=0.1)
    pose = c2w_opengl_from_viewmat(V)
    gs = GaussianSplat.from_model(model, PinholeCamera(torch.from_numpy(pose[:3]), 40.0, 40.0, W / 2, H / 2, W, H))
    r = model._rasterizer()
    try:
        image = gs.render(pose)["rgb"].clone()
        xi = np.array([0.01, -0.012, 0.008, 0.006, -0.004, 0.005])
        V0 = se3_exp(xi) @ np.asarray(V, np.float64)
        start = c2w_opengl_from_viewmat(V0)
        got = gs.refine_pose(start, image, iters=240)
        want = refine_camera_pose(r, image, viewmat_from_c2w_opengl(start[:3]), K, W, H, 240, background=tuple(float(v) for v in model.background_color))
        assert got.shape == (4, 4)
        a0, d0 = gc.pose_error(V0, V)
        a1, d1 = gc.pose_error(viewmat_from_c2w_opengl(got[:3]), V)
        a2, d2 = gc.pose_error(want.viewmat, V)
        print(f"BACKWARD door A refine_pose: {a0:.3f} deg, {d0 * 1e3:.2f} mm -> {a1:.4f} deg, {d1 * 1e3:.3f} mm (refine_camera_pose: {a2:.4f} deg, {d2 * 1e3:.3f} mm)")
        assert a1 < 0.5 * a0 and d1 < 0.5 * d0                    # it moves towards the truth ...
        assert abs(a1 - a2) < 0.05 * a0 and abs(d1 - d2) < 0.05 * d0   # ... as the function underneath does (float atomics: not bit for bit)
    finally:
        r.close()


def test_error_paths(rasterizer):
    from sim_a_splat_amd.rasterizer import Rasterizer
    r = rasterizer
    sc, cam, g = gc.case("blob_32x32")
    V, K, W, H = cam
    fresh = Rasterizer(0)
    try:
        with pytest.raises(SasError, match="before sas_scene_upload"):
            fresh.render_backward(V, K, W, H, g[0])
    finally:
        fresh.close()
    sc_kit.upload(r, sc)
    with pytest.raises(ValueError, match="all None"):
        r.render_backward(V, K, W, H)
    with pytest.raises(ValueError, match="g_rgb must be"):
        r.render_backward(V, K, W, H, g[0][:-1])
    L = _capi.lib()
    Vp, Kp = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(K, np.float32)
    gt = torch.zeros((H, W), device=r.device)
    d_first = torch.zeros((r.n, 3), device=r.device)
    for fn, n_out in ((L.sas_render_backward_screen, 5), (L.sas_render_backward, 7)):
        rc = fn(r._ctx, Vp.ctypes.data, Kp.ctypes.data, W, H, 0, None, gt.data_ptr(), None, *([None] * n_out), None)
        assert rc != 0 and b"output is NULL" in L.sas_last_error(r._ctx)
        rc = fn(r._ctx, Vp.ctypes.data, Kp.ctypes.data, W, H, 0, None, None, None, d_first.data_ptr(), *([None] * (n_out - 1)), None)
        assert rc != 0 and b"are all NULL" in L.sas_last_error(r._ctx)
        rc = fn(r._ctx, Vp.ctypes.data, Kp.ctypes.data, -1, H, 0, None, gt.data_ptr(), None, d_first.data_ptr(), *([None] * (n_out - 1)), None)
        assert rc != 0 and b"bad image size" in L.sas_last_error(r._ctx)
        rc = fn(r._ctx, Vp.ctypes.data, Kp.ctypes.data, W, H, _capi.SAS_ASYNC, None, gt.data_ptr(), None, d_first.data_ptr(), *([None] * (n_out - 1)), None)
        assert rc != 0 and b"not accepted" in L.sas_last_error(r._ctx)
    d_cov6 = torch.zeros((r.n, 6), device=r.device)
    rc = L.sas_render_backward(r._ctx, Vp.ctypes.data, Kp.ctypes.data, W, H, 0, None, gt.data_ptr(), None, None, None, None, None, None,
                               d_cov6.data_ptr(), None, None)
    assert rc != 0 and b"quaternions and scales" in L.sas_last_error(r._ctx)
    r.upload_meshes(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]]), np.array([0.5, 0.5, 0.5], np.float32))
    try:
        with pytest.raises(SasError, match="meshes"):
            r.render_backward(V, K, W, H, g[0])
    finally:
        r.clear_meshes()
    assert r.render_backward(V, K, W, H, g[0])["means"].abs().sum() > 0   # the context stays usable
