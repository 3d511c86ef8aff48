"""GPU: the adjoint of the deformation (sas_scene_deform_backward; Rasterizer.deform_backward, autograd.render_differentiable(node_transforms=),
deform.fit_node_transforms, SplatScene.fit_deformation; DESIGN.md 3, "Deformation") against tests/tools/skin_grad_ref.py, the torch restatement
of skin_ref.deform_ref under autograd.  Every case is held to the float64 restatement within four times the float32 restatement's own error
(F32_ERR below: the largest over four shuffled orders of the Gaussians, since the device sums in an arbitrary order; the measured ratios are
printed); what the contract makes exact -- rows of unnamed nodes, zero upstream -- is compared for equality.  Scenes have 777 Gaussians in 2
groups, as quaternions and as covariances; frames are 64x48."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import SasError

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import scene_cases as sc_kit  # noqa: E402
import skin_grad_child  # noqa: E402
import skin_grad_ref as sg  # noqa: E402
import skin_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
BG = (0.1, 0.2, 0.3)

# python tests/tools/skin_grad_ref.py
F32_ERR = {   # (case, form): (dR, dt), float32 restatement against float64, the largest of 4 shuffled orders
    ("m1", "quats"): (7.87e-07, 1.68e-06),
    ("m1", "covariances"): (6.84e-07, 3.69e-07),
    ("m5_k3", "quats"): (2.40e-07, 2.56e-07),
    ("m5_k3", "covariances"): (3.00e-07, 8.37e-07),
    ("m70_k4", "quats"): (2.37e-07, 1.22e-07),
    ("m70_k4", "covariances"): (2.61e-07, 5.05e-07),
    ("m257_k8", "quats"): (2.06e-07, 8.26e-08),
    ("m257_k8", "covariances"): (1.77e-07, 1.37e-07),
    ("m2048_k4", "quats"): (1.14e-07, 6.25e-08),
    ("m2048_k4", "covariances"): (6.24e-08, 8.57e-08),
    ("m2049_k4", "quats"): (1.46e-07, 7.79e-08),
    ("m2049_k4", "covariances"): (1.37e-07, 7.61e-08),
    ("m70_far", "quats"): (1.47e-07, 1.39e-07),
    ("m70_far", "covariances"): (1.89e-07, 1.50e-07),
    ("m70_group", "quats"): (1.32e-07, 2.27e-07),
    ("m70_group", "covariances"): (1.45e-07, 2.23e-07),
    ("m70_dead", "quats"): (1.98e-07, 1.79e-07),
    ("m70_dead", "covariances"): (1.36e-07, 1.49e-07),
}
F32_ERR_MEANS_ONLY = {
    ("m70_k4", "quats"): (2.22e-07, 1.22e-07),
    ("m70_k4", "covariances"): (2.34e-07, 5.05e-07),
}
ALL = [(name, form) for name in sg.CASES for form in sg.FORMS]


def _cam(yaw=25.0):
    return sc_kit.ring(W, H, f=55.0, yaw=yaw, elev=0.3)[:2]


def _held(got, ref, f32, what):
    """The four-times rule on both outputs; prints the ratios."""
    e = sg.split_err(got, ref)
    print(f"  {what}: dR device {e[0]:.3e} = {e[0] / f32[0]:.2f} x float32 restatement, dt device {e[1]:.3e} = {e[1] / f32[1]:.2f} x")
    assert e[0] <= 4.0 * f32[0] and e[1] <= 4.0 * f32[1], (what, e, f32)


def _bind(r, c):
    """The case's scene and skin on ``r``; returns the binding the device holds (the kit's, or what ``bind_skin`` made of the kit's arguments)."""
    r.upload(**c["scene"])
    if c["dead"] or set(c["bind"]) == {"k"}:
        r.set_skin(c["indices"], c["weights"])
        return c["indices"], c["weights"]
    r.bind_skin(c["nodes"], **c["bind"])
    back = r.read_skin()
    idx, w = back["indices"].cpu().numpy(), back["weights"].cpu().numpy()
    assert np.array_equal(idx, c["indices"])   # (the weights are the device's exp: the reference takes them as they are)
    return idx, w


def _grads(r, c, means=True, orient=True):
    g = {}
    if means:
        g["means"] = torch.from_numpy(c["d_means"]).to(r.device)
    if orient:
        g[c["form"]] = torch.from_numpy(c["d_orient"]).to(r.device)
    return g


# ---- every case against the float64 restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", ALL)
def test_every_case_is_the_restatement(rasterizer, name, form):
    r = rasterizer
    c = sg.case(name, form)
    idx, w = _bind(r, c)
    r.deform(c["transforms"])
    got = r.deform_backward(_grads(r, c))
    assert got.device == r.device and got.dtype == torch.float32 and tuple(got.shape) == (c["m"], 3, 4)
    got = got.cpu().numpy()
    ref = sg.grad64(name, form) if w is c["weights"] else sg.node_grad_ref(c["rest"], idx, w, c["transforms"], c["d_means"], c["d_orient"])
    _held(got, ref, F32_ERR[(name, form)], f"{name} {form}")
    # rows of nodes no live entry names are exactly zero
    named = np.zeros(c["m"], bool)
    live = (idx >= 0) & (idx < c["m"]) & (w > 0)
    named[idx[live]] = True
    assert (got[~named] == 0.0).all() and np.isfinite(got).all()
    if name in ("m257_k8", "m2048_k4", "m2049_k4", "m70_far"):
        assert (~named).any()
    if name in ("m70_far", "m70_group", "m70_dead"):
        assert (~live.any(axis=1)).any()   # Gaussians without a live entry occur


@pytest.mark.parametrize("form", sg.FORMS)
def test_exact_zeros_means_alone_and_dead_entries(rasterizer, form):
    r = rasterizer
    c = sg.case("m70_k4", form)
    _bind(r, c)
    r.deform(c["transforms"])
    zero = {k: torch.zeros_like(v) for k, v in _grads(r, c).items()}
    assert (r.deform_backward(zero).cpu().numpy() == 0.0).all()
    # means alone: the mean path, no quaternion term -- the reference with a zero orientation gradient
    got = r.deform_backward(_grads(r, c, orient=False)).cpu().numpy()
    ref = sg.grad64("m70_k4", form, True, False)
    assert np.array_equal(ref, sg.node_grad_ref(c["rest"], c["indices"], c["weights"], c["transforms"], c["d_means"], np.zeros_like(c["d_orient"])))
    _held(got, ref, F32_ERR_MEANS_ONLY[("m70_k4", form)], f"means alone {form}")
    # ... and the orientation alone adds up with it to the whole (the adjoint is linear)
    rot = r.deform_backward(_grads(r, c, means=False)).cpu().numpy()
    _held(got.astype(np.float64) + rot, sg.grad64("m70_k4", form), F32_ERR[("m70_k4", form)], f"means + orientation {form}")
    # dead entries (index -1, index >= m, weight 0, weight negative) change nothing: the same figures as the entries written as (-1, 0)
    d = sg.case("m70_dead", form)
    live = (d["indices"] >= 0) & (d["indices"] < d["m"]) & (d["weights"] > 0)
    clean_i, clean_w = np.where(live, d["indices"], -1).astype(np.int32), np.where(live, d["weights"], 0.0).astype(np.float32)
    assert (clean_i != d["indices"]).any() and (clean_w != d["weights"]).any()
    ref = sg.grad64("m70_dead", form)
    assert np.array_equal(ref, sg.node_grad_ref(d["rest"], clean_i, clean_w, d["transforms"], d["d_means"], d["d_orient"]))
    r.upload(**d["scene"])
    for what, (i, w) in (("dead", (d["indices"], d["weights"])), ("clean", (clean_i, clean_w))):
        r.set_skin(i, w)
        r.deform(d["transforms"])
        _held(r.deform_backward(_grads(r, d)).cpu().numpy(), ref, F32_ERR[("m70_dead", form)], f"{what} entries {form}")


# ---- the paths ------------------------------------------------------------------------------------------------------------------------------
def test_lds_and_global_paths_and_both_forms_agree(rasterizer, tmp_path):
    """SAS_SKIN_GRAD_LDS=0 (every sum in global memory) and both forms of the adds, in a fresh child process: each agrees with this process'
    defaults within the bound, and is itself held to the float64 restatement.  (The limit and limit + 1 are cases of the test above.)"""
    out = tmp_path / "skin_grad_child.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("SAS_SKIN_GRAD_LDS", "SAS_SKIN_GRAD_STAGED")}
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "tools" / "skin_grad_child.py"), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "skin grad child ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
    with np.load(out) as z:
        for name, form in skin_grad_child.CASES:
            mine = skin_grad_child.node_grad(rasterizer, sg.case(name, form))
            for setting in skin_grad_child.SETTINGS:
                other = z[f"{setting}_{name}_{form}"]
                _held(other, sg.grad64(name, form), F32_ERR[(name, form)], f"{setting} {name} {form}")
                _held(other, mine, F32_ERR[(name, form)], f"{setting} against the default, {name} {form}")


# ---- linearity, and the chain on real gradients ---------------------------------------------------------------------------------------------
def _f32_err_of(c, d_means, d_orient, ref):
    worst = [0.0, 0.0]
    for s in range(sg.ORDERS):
        order = np.random.default_rng(7000 + s).permutation(c["rest"]["means"].shape[0])
        e = sg.split_err(sg.node_grad_ref(c["rest"], c["indices"], c["weights"], c["transforms"], d_means, d_orient, torch.float32, order), ref)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    return worst


@pytest.mark.parametrize("form", sg.FORMS)
def test_chain_on_real_gradients_linearity_and_autograd(rasterizer, form):
    """render_backward on two frames of the deformed scene, then deform_backward.  The reference chains the SAME device gradients through the float64
    restatement, so only the new kernel is under test; the bound is four times the float32 restatement's error on those gradients."""
    from sim_a_splat_amd.autograd import render_differentiable
    r = rasterizer
    c = sg.case("m70_k4", form)
    _bind(r, c)
    r.deform(c["transforms"])
    want = ("means", form)
    rng = np.random.default_rng(31)
    views = [(_cam(25.0), rng.normal(size=(H, W, 3)).astype(np.float32)), (_cam(140.0), rng.normal(size=(H, W, 3)).astype(np.float32))]
    acc, parts, singles = {}, [], []
    for (V, K), g in views:
        r.render(V, K, W, H, BG)
        one = r.render_backward(V, K, W, H, g_rgb=g, want=want)
        assert set(one) == set(want) and float(one["means"].abs().max()) > 0.0
        parts.append({k: v.clone() for k, v in one.items()})
        singles.append(r.deform_backward(one).cpu().numpy().astype(np.float64))
        for k, v in one.items():   # the sum of the views, as out= would hold it
            acc[k] = v.clone() if k not in acc else acc[k] + v
    got = r.deform_backward(acc).cpu().numpy()
    dm, do = acc["means"].cpu().numpy(), acc[form].cpu().numpy()
    ref = sg.node_grad_ref(c["rest"], c["indices"], c["weights"], c["transforms"], dm, do)
    f32 = _f32_err_of(c, dm, do, ref)
    _held(got, ref, f32, f"two views, one call {form}")
    _held(singles[0] + singles[1], got, f32, f"two calls against one {form}")
    # through out=: the accumulation render_backward does itself
    acc2 = {}
    for (V, K), g in views:
        r.render(V, K, W, H, BG)
        acc2 = r.render_backward(V, K, W, H, g_rgb=g, want=want, out=acc2)
    _held(r.deform_backward(acc2).cpu().numpy(), ref, f32, f"out= accumulation {form}")
    # render_differentiable(node_transforms=T): one view, T a float64 host tensor -- its gradient comes back as such
    (V, K), g = views[0]
    ref1 = sg.node_grad_ref(c["rest"], c["indices"], c["weights"], c["transforms"], parts[0]["means"].cpu().numpy(), parts[0][form].cpu().numpy())
    f32_1 = _f32_err_of(c, parts[0]["means"].cpu().numpy(), parts[0][form].cpu().numpy(), ref1)
    T = torch.from_numpy(c["transforms"].astype(np.float64)).requires_grad_(True)
    Vt = torch.from_numpy(np.asarray(V, np.float32)).requires_grad_(True)
    frame = render_differentiable(r, Vt, K, W, H, background=(0.0, 0.0, 0.0), node_transforms=T)
    # a loss whose gradient with respect to the raw accumulator is g where the frame is below 1 (prechain's clamp), as in the direct call
    (frame["rgb"] * torch.from_numpy(g).to(r.device)).sum().backward()
    assert T.grad is not None and T.grad.shape == T.shape and T.grad.dtype == torch.float64 and T.grad.device == T.device and Vt.grad is not None
    rgb = r.render(V, K, W, H, (0.0, 0.0, 0.0))["rgb"]
    if bool((rgb < 1).all()):   # (no pixel at the clamp: the two upstream gradients are the same image)
        _held(T.grad.numpy(), ref1, f32_1, f"render_differentiable {form}")
    else:
        gm = torch.where(rgb < 1, torch.from_numpy(g).to(r.device), torch.zeros_like(rgb))
        one = r.render_backward(V, K, W, H, g_rgb=gm, g_alpha=torch.zeros((H, W), device=r.device), want=want)
        refc = sg.node_grad_ref(c["rest"], c["indices"], c["weights"], c["transforms"], one["means"].cpu().numpy(), one[form].cpu().numpy())
        _held(T.grad.numpy(), refc, _f32_err_of(c, one["means"].cpu().numpy(), one[form].cpu().numpy(), refc), f"render_differentiable {form}")


# ---- state and refusals ---------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(rasterizer):
    r = rasterizer
    L = _capi.lib()
    c = sg.case("m70_k4", "quats")
    V, K = _cam()
    renders = lambda: float(r.render(V, K, W, H, BG)["alpha"].sum()) > 0.0
    r.upload(**c["scene"])
    g = _grads(r, c)
    out = torch.zeros((c["m"], 3, 4), dtype=torch.float32, device=r.device)
    call = lambda dm=g["means"].data_ptr(), dq=g["quats"].data_ptr(), dc=None, o=out.data_ptr(): L.sas_scene_deform_backward(r._ctx, dm, dq, dc, o, None)
    # no skin
    with pytest.raises(SasError, match="no skin"):
        r.deform_backward(g)
    assert call() == -1 and b"no skin is bound" in L.sas_last_error(r._ctx) and renders()
    # no deform since the bind
    r.set_skin(c["indices"], c["weights"])
    with pytest.raises(SasError, match="no deform"):
        r.deform_backward(g)
    assert call() == -1 and b"no sas_scene_deform since" in L.sas_last_error(r._ctx) and renders()
    r.deform(c["transforms"])
    # a rebind resets it, and so does a clear
    r.set_skin(c["indices"], c["weights"])
    with pytest.raises(SasError, match="no deform"):
        r.deform_backward(g)
    assert call() == -1 and renders()
    r.deform(c["transforms"])
    r.clear_skin()
    with pytest.raises(SasError, match="no skin"):
        r.deform_backward(g)
    assert call() == -1 and renders()
    r.set_skin(c["indices"], c["weights"])
    r.deform(c["transforms"])
    # the C entry's other refusals
    assert call(dm=None, dq=None) == -1 and b"all NULL" in L.sas_last_error(r._ctx)
    assert call(dc=g["means"].data_ptr()) == -1 and b"d_cov6 must be NULL" in L.sas_last_error(r._ctx)
    assert call(o=None) == -1 and b"d_node_Rt is NULL" in L.sas_last_error(r._ctx)
    assert call() == 0 and renders()
    # a wrong-form orientation key, wrong shapes, dtypes and devices
    cov = torch.zeros((sr.N, 6), dtype=torch.float32, device=r.device)
    for bad in ({"means": g["means"], "covariances": cov}, {"covariances": cov}):
        with pytest.raises(ValueError, match="uploaded as quats"):
            r.deform_backward(bad)
    for bad in ({"means": g["means"][:-1].contiguous()}, {"means": g["means"].double()}, {"means": g["means"].cpu()}, {"means": g["means"].T},
                {"quats": g["quats"][:, :3].contiguous()}, {"quats": g["quats"].half()}, {"means": c["d_means"]}):
        with pytest.raises(ValueError, match="contiguous float32"):
            r.deform_backward(bad)
    with pytest.raises(ValueError, match="neither means nor"):
        r.deform_backward({"opacities": torch.zeros(sr.N, device=r.device)})
    with pytest.raises(ValueError, match="dict"):
        r.deform_backward(g["means"])
    assert renders()
    # other keys are ignored; the last deform is the one differentiated; the caller's tensor may change after deform
    ref = sg.grad64("m70_k4", "quats")
    T2 = torch.from_numpy(c["transforms"]).to(r.device)
    r.deform(sr.transforms(c["nodes"], seed=81))
    r.deform(T2)
    T2.zero_()
    got = r.deform_backward(dict(g, opacities=torch.zeros(3, device=r.device), viewmat=None)).cpu().numpy()
    _held(got, ref, F32_ERR[("m70_k4", "quats")], "deform(T1); deform(T2); T2 overwritten")
    # a covariance scene refuses quats
    cc = sg.case("m70_k4", "covariances")
    _bind(r, cc)
    r.deform(cc["transforms"])
    with pytest.raises(ValueError, match="uploaded as covariances"):
        r.deform_backward({"means": g["means"], "quats": g["quats"]})
    assert L.sas_scene_deform_backward(r._ctx, g["means"].data_ptr(), g["quats"].data_ptr(), None, out.data_ptr(), None) == -1
    assert b"d_quats must be NULL" in L.sas_last_error(r._ctx) and renders()
    # upload drops the state with the skin
    r.upload(**c["scene"])
    with pytest.raises(SasError, match="no skin"):
        r.deform_backward(g)


# ---- recovery: how is the sheet bent, from pictures -----------------------------------------------------------------------------------------
def test_fit_node_transforms_recovers_the_bend(rasterizer):
    """The CPU test's recovery case with the same settings, on the device: the run ends where the float64 reference run ends, within 5 % of the
    start error, and below the fraction of the start the kit records (no case of CPU-test size reaches a tenth: skin_grad_ref.RECOVER_FRACTION)."""
    from sim_a_splat_amd import deform
    r = rasterizer
    c = sg.recovery_case()
    r.upload(**c["upload"])
    r.set_skin(c["indices"], c["weights"])
    V, K = np.stack([cam[0] for cam in c["cams"]]), np.stack([cam[1] for cam in c["cams"]])
    res = deform.fit_node_transforms(r, c["images"], V, K, sg.RECOVER_W, sg.RECOVER_H, c["nodes"], iters=sg.RECOVER_ITERS)
    e0, e1 = sg.recovery_error(c, sr.identity_transforms(9)), sg.recovery_error(c, res.transforms)
    print(f"  recovery on the device: mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start (the reference run: {sg.RECOVER_REF_END}); "
          f"loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    assert abs(e1 / e0 - sg.RECOVER_REF_END) < 0.05
    assert e1 < sg.RECOVER_FRACTION * e0
    assert res.transforms.shape == (9, 3, 4) and res.transforms.dtype == np.float64 and len(res.history) == sg.RECOVER_ITERS + 1
    # r is left deformed at the result
    now = r.read_scene()["means"].cpu().numpy()
    want = sr.deform_ref(c["rest"], c["indices"], c["weights"], res.transforms.astype(np.float32))["means"]
    assert np.abs(now - want).max() < 1e-5
    with pytest.raises(ValueError, match="no skin is bound"):
        r.clear_skin()
        deform.fit_node_transforms(r, c["images"], V, K, sg.RECOVER_W, sg.RECOVER_H, c["nodes"], iters=2)


def _look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(wxyz, position) of a camera at ``position`` looking at ``target``: camera-to-world, OpenCV axes (x right, y down, z forward)."""
    from sim_a_splat_amd.poses import matrix_to_quat_wxyz
    p = np.asarray(position, np.float64)
    z = np.asarray(target, np.float64) - p
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return tuple(matrix_to_quat_wxyz(np.stack([x, np.cross(z, x), z], axis=1))), tuple(p)


def test_door_b_fits_its_deformable_group():
    """SplatScene.fit_deformation on a two-group scene whose second group is the kit's sheet: from frames of the truth (get_renders after
    deform(truth)) and a start at rest, the sheet's means end below the same fraction of their start distance, and the next get_render shows it."""
    from sim_a_splat_amd.scene import SplatScene
    c = sg.recovery_case()
    rng = np.random.default_rng(96)
    n0 = 150
    static = ((rng.normal(0.0, 0.08, (n0, 3)) + (0.0, 0.62, 0.0)).astype(np.float32), np.tile(np.eye(3, dtype=np.float32) * 2e-3, (n0, 1, 1)),
              rng.uniform(0, 1, (n0, 3)).astype(np.float32), rng.uniform(0.5, 0.9, n0).astype(np.float32))
    M = sr.quat_to_matrix(c["rest"]["quats"]) * c["scales"].astype(np.float64)[:, None, :]
    cov = (M @ np.swapaxes(M, 1, 2)).astype(np.float32)
    scene = SplatScene(0, background=(0.0, 0.0, 0.0))
    try:
        scene.add_gaussian_splats("static", *static)
        cloth = scene.add_gaussian_splats("cloth", c["rest"]["means"], cov, c["colors"], c["op"], position=(0.0, -0.05, 0.0))
        with pytest.raises(RuntimeError, match="bind_deformable first"):
            scene.fit_deformation(np.zeros((1, H, W, 3), np.uint8), H, W, [_look_at((0.0, 0.0, 1.5))])
        scene.bind_deformable(cloth, c["nodes"], k=4)
        cams = [_look_at((0.0, -0.5, 1.4)), _look_at((1.1, 0.3, 1.0))]
        rows = slice(n0, n0 + sg.RECOVER_N)
        scene.deform(c["truth"].astype(np.float32))
        images = scene.get_renders(H, W, cams, fov=0.9).copy()
        truth = scene._raster.read_scene()["means"].cpu().numpy()[rows]
        scene.deform(sr.identity_transforms(9))
        rest_frame = scene.get_render(H, W, *cams[0], fov=0.9).astype(np.float64)
        rest = scene._raster.read_scene()["means"].cpu().numpy()[rows]
        res = scene.fit_deformation(images, H, W, cams, fov=0.9, iters=sg.RECOVER_ITERS)
        after = scene._raster.read_scene()["means"].cpu().numpy()[rows]
        e0, e1 = np.linalg.norm(rest - truth, axis=1).mean(), np.linalg.norm(after - truth, axis=1).mean()
        f1 = scene.get_render(H, W, *cams[0], fov=0.9).astype(np.float64)
        d0, d1 = np.abs(rest_frame - images[0]).mean(), np.abs(f1 - images[0]).mean()
        print(f"  Door B: mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start; frame difference {d0:.3f} -> {d1:.3f} (of 255); loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
        assert e1 < sg.RECOVER_FRACTION * e0
        assert d1 < 0.5 * d0   # the next get_render shows the result
        assert res.transforms.shape == (9, 3, 4) and scene._raster.has_skin
    finally:
        scene.close()


# ---- last: the bounds-checked build ---------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    import ctypes
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
