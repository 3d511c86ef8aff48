"""GPU: gradients to the group poses (sas_render_backward_poses, Rasterizer.render_backward(pose_groups=), autograd.render_differentiable(
group_poses=), register.refine_group_poses, SplatScene.refine_handle_poses; DESIGN.md 3, "Backward pass") against
tests/tools/group_pose_ref.py, the float64 reference that poses the scene itself in front of tests/tools/grad_ref.py.

Measure and bound are test_gpu_t_backward.py's: per array max |g - g_ref| / max |g_ref| at most FOUR times the same measure of the
reference evaluated in float32 -- F32_ERR below, printed by python tests/tools/group_pose_cases.py -- and 0 where the float32 reference is
exact.  Upstream gradients are zero at the pixels the reference reports as near a decision threshold."""
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
import group_pose_cases as gpc  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

F32_ERR = {
    "gp600": dict(means=1.79e-06, opacities=1.32e-06, colors=9.98e-07, viewmat=1.26e-06, quats=2.40e-06, scales=2.24e-06, group_poses=1.73e-06),
    "gp600_cov6": dict(means=1.75e-06, opacities=1.27e-06, colors=9.84e-07, viewmat=1.28e-06, covariances=1.90e-06, group_poses=1.71e-06),
    "gp_sh2": dict(means=1.86e-06, opacities=3.15e-07, colors=4.90e-07, viewmat=6.03e-07, quats=1.41e-06, scales=4.19e-07, group_poses=5.51e-07),
    "gp_rare": dict(means=1.87e-06, opacities=9.26e-07, colors=5.51e-07, viewmat=1.49e-06, quats=1.63e-06, scales=1.15e-06, group_poses=1.20e-06),
    "gp_behind": dict(means=1.27e-06, opacities=1.54e-06, colors=1.29e-06, viewmat=1.49e-06, quats=9.32e-07, scales=1.18e-06, group_poses=8.65e-07),
    "gp_clamp": dict(means=1.50e-06, opacities=7.00e-07, colors=4.41e-07, viewmat=2.74e-06, quats=4.22e-07, scales=7.02e-07, group_poses=9.50e-07),
    "gp_rare_row": dict(group_poses=2.36e-06),
    "two_views": dict(group_poses=8.65e-07),
    "l2": dict(group_poses=1.81e-06, viewmat=1.04e-06),
}
FACTOR = 4.0


def _hold(what, got, ref, f32_err):
    """Print every figure, then hold each array to FACTOR times the float32 reference's error."""
    rows = [(k, grad_ref.rel_err(got[k], ref[k]), FACTOR * f32_err[k]) for k in ref]
    for k, e, b in rows:
        print(f"GROUP POSE {what:28s} {k:12s} hip {e:.3e}  float32 ref {f32_err[k]:.3e}  bound {b:.3e}  {'ok' if e <= b else 'MISS'}")
    bad = [(k, e, b) for k, e, b in rows if not e <= b]
    assert not bad, (what, bad)


def _np(d):
    return {k: v.double().cpu().numpy() for k, v in d.items()}


def _setup(r, name):
    sc, (V, K, W, H), _ = gpc.case(name)
    sc_kit.upload(r, sc)
    return sc, (V, K, W, H), gpc.masked_upstream(name), gpc.reference(name)["full"]


@pytest.mark.parametrize("name", gpc.NAMES)
def test_case_against_reference(rasterizer, name):
    """Every case, all its groups: ``group_poses`` alone through ``want``, and again in the full call with every other array held too."""
    r = rasterizer
    sc, (V, K, W, H), g, ref = _setup(r, name)
    groups = tuple(range(sc["G"]))
    alone = r.render_backward(V, K, W, H, *g, pose_groups=groups, want=("group_poses",))
    assert set(alone) == {"group_poses"} and tuple(alone["group_poses"].shape) == (len(groups), 3, 4) and alone["group_poses"].dtype == torch.float32
    _hold(name + " alone", _np(alone), {"group_poses": ref["group_poses"]}, F32_ERR[name])
    full = r.render_backward(V, K, W, H, *g, pose_groups=groups)
    assert list(full)[-1] == "group_poses" and list(full)[:-1] == list(r.render_backward(V, K, W, H, *g))   # the other keys and their order are the plain call's
    _hold(name + " full", _np(full), ref, F32_ERR[name])
    if name == "gp_behind":   # a group whose Gaussians are all culled: exact zeros
        assert np.all(ref["group_poses"][gpc.BEHIND_GROUP] == 0)
        for res in (alone, full):
            assert torch.all(res["group_poses"][gpc.BEHIND_GROUP] == 0)
    if name == "gp_rare":     # three Gaussians, absent from most waves: its row alone, held to the float32 reference's error on that row
        row, want = _np(alone)["group_poses"][gpc.RARE_GROUP], ref["group_poses"][gpc.RARE_GROUP]
        _hold("gp_rare row", {"group_poses": row}, {"group_poses": want}, F32_ERR["gp_rare_row"])


def test_selection(rasterizer):
    """The order of ``pose_groups`` is the order of the rows, one group works, and a group that is not named leaves no trace."""
    r = rasterizer
    sc, (V, K, W, H), g, ref = _setup(r, "gp600")
    err = F32_ERR["gp600"]
    got = _np(r.render_backward(V, K, W, H, *g, pose_groups=(3, 0), want=("group_poses",)))["group_poses"]
    assert got.shape == (2, 3, 4)
    _hold("order (3, 0)", {"group_poses": got}, {"group_poses": ref["group_poses"][[3, 0]]}, err)
    one = _np(r.render_backward(V, K, W, H, *g, pose_groups=[2], want=("group_poses",)))["group_poses"]
    assert one.shape == (1, 3, 4)
    _hold("n_sel = 1", {"group_poses": one}, {"group_poses": ref["group_poses"][[2]]}, err)
    # the rare and the culled group through a selection that names only them
    sc, (V, K, W, H), g, ref = _setup(r, "gp_behind")
    got = r.render_backward(V, K, W, H, *g, pose_groups=(gpc.BEHIND_GROUP,), want=("group_poses",))["group_poses"]
    assert torch.all(got == 0)


def test_two_views_sum(rasterizer):
    r = rasterizer
    ref, nears, gs = gpc.two_view_reference()
    sc, cams = gpc.two_view_case()
    sc_kit.upload(r, sc)
    out = None
    for (V, K, W, H), near, g in zip(cams, nears, gs):
        keep = ~near
        gm = [(gi * (keep[..., None] if gi.ndim == 3 else keep)).astype(np.float32) for gi in g]
        out = r.render_backward(V, K, W, H, *gm, out=out, want=("group_poses",), pose_groups=range(sc["G"]))
    _hold("two_views", _np(out), ref, F32_ERR["two_views"])


def test_two_calls_agree(rasterizer):
    """The C ABI runs the projection stage only behind a fresh screen-space pass (float atomics), so the same bits twice cannot be asked of
    two calls: asserted is that two full calls both hold the 4x bound, and, printed, how far apart they are."""
    r = rasterizer
    sc, (V, K, W, H), g, ref = _setup(r, "gp600")
    a = _np(r.render_backward(V, K, W, H, *g, pose_groups=range(5), want=("group_poses",)))
    b = _np(r.render_backward(V, K, W, H, *g, pose_groups=range(5), want=("group_poses",)))
    print(f"GROUP POSE two calls differ by {grad_ref.rel_err(a['group_poses'], b['group_poses']):.3e}")
    for k, res in (("first", a), ("second", b)):
        _hold(k, res, {"group_poses": ref["group_poses"]}, F32_ERR["gp600"])


def test_autograd_l2_loss(rasterizer):
    r = rasterizer
    ref, keep, targets = gpc.l2_reference()
    sc, (V, K, W, H), _ = gpc.case(gpc.L2_CASE)
    sc_kit.upload(r, sc)
    dev = r.device
    G = torch.tensor(np.asarray(sc["Rt"], np.float64).reshape(-1, 3, 4), dtype=torch.float64, requires_grad=True)   # on the host, float64
    vm = torch.tensor(np.asarray(V, np.float32), device=dev, requires_grad=True)
    out = autograd.render_differentiable(r, vm, K, W, H, background=gc.L2_BACKGROUND, group_poses=G)
    t_rgb, t_a, t_d = [torch.tensor(t, device=dev) for t in targets]
    kp = torch.tensor(keep.astype(np.float32), device=dev)
    loss = (kp[..., None] * (out["rgb"] - t_rgb) ** 2).sum() + (kp * (out["alpha"][..., 0] - t_a) ** 2).sum() + \
        0.1 * (kp * (out["depth"][..., 0] - t_d) ** 2).sum()
    gv, gG = torch.autograd.grad(loss, [vm, G])
    assert gG.shape == G.shape and gG.dtype == G.dtype and gG.device == G.device   # in its shape, device and dtype
    _hold("l2", dict(group_poses=gG.numpy(), viewmat=gv[:3].double().cpu().numpy()), ref, F32_ERR["l2"])
    # [G,12], two groups named: their rows are filled, the rest are zero
    G12 = torch.tensor(np.asarray(sc["Rt"], np.float32).reshape(-1, 12), device=dev, requires_grad=True)
    out = autograd.render_differentiable(r, vm.detach(), K, W, H, background=gc.L2_BACKGROUND, group_poses=G12, pose_groups=(4, 1))
    loss = (kp[..., None] * (out["rgb"] - t_rgb) ** 2).sum() + (kp * (out["alpha"][..., 0] - t_a) ** 2).sum() + \
        0.1 * (kp * (out["depth"][..., 0] - t_d) ** 2).sum()
    (g12,) = torch.autograd.grad(loss, [G12])
    assert g12.shape == (5, 12) and g12.device == G12.device and torch.all(g12[[0, 2, 3]] == 0)
    _hold("l2 rows 4, 1", {"group_poses": g12[[4, 1]].double().cpu().numpy().reshape(2, 3, 4)}, {"group_poses": ref["group_poses"][[4, 1]]},
          F32_ERR["l2"])


def test_error_paths(rasterizer):
    r = rasterizer
    sc, (V, K, W, H), g, ref = _setup(r, "gp600")
    alive = lambda: r.render_backward(V, K, W, H, *g, pose_groups=(0,), want=("group_poses",))["group_poses"].abs().sum() > 0
    with pytest.raises(SasError, match="duplicate"):
        r.render_backward(V, K, W, H, *g, pose_groups=(1, 2, 1))
    assert alive()
    with pytest.raises(SasError, match="n_groups"):
        r.render_backward(V, K, W, H, *g, pose_groups=(0, 5))
    assert alive()
    with pytest.raises(SasError, match="n_sel 33"):
        r.render_backward(V, K, W, H, *g, pose_groups=range(33))
    assert alive()
    with pytest.raises(ValueError, match="screen_space"):
        r.render_backward(V, K, W, H, *g, pose_groups=(0,), screen_space=True)
    with pytest.raises(ValueError, match="want must name"):
        r.render_backward(V, K, W, H, *g, want=("group_poses",))
    L = _capi.lib()
    Vp, Kp = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(K, np.float32)
    gt = torch.zeros((H, W), device=r.device)
    d = torch.zeros((1, 12), device=r.device)
    sel = np.zeros(1, np.uint8)
    rc = L.sas_render_backward_poses(r._ctx, Vp.ctypes.data, Kp.ctypes.data, W, H, 0, None, gt.data_ptr(), None, *([None] * 7), 1, None, d.data_ptr(), None)
    assert rc != 0 and b"is NULL" in L.sas_last_error(r._ctx)
    rc = L.sas_render_backward_poses(r._ctx, Vp.ctypes.data, Kp.ctypes.data, W, H, 0, None, gt.data_ptr(), None, *([None] * 7), 1, sel.ctypes.data, None, None)
    assert rc != 0 and b"NULL" in L.sas_last_error(r._ctx)
    rc = L.sas_render_backward_poses(r._ctx, Vp.ctypes.data, Kp.ctypes.data, W, H, 0, None, gt.data_ptr(), None, *([None] * 7), -1, sel.ctypes.data, d.data_ptr(), None)
    assert rc != 0 and b"n_sel -1" in L.sas_last_error(r._ctx)
    assert alive()
    r.upload_meshes(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]]), np.array([0.5, 0.5, 0.5], np.float32))
    try:
        with pytest.raises(SasError, match="meshes"):
            r.render_backward(V, K, W, H, *g, pose_groups=(0,))
    finally:
        r.clear_meshes()
    assert alive()
    plain, cam, gp = gc.case("blob_32x32")   # a scene without groups
    sc_kit.upload(r, plain)
    with pytest.raises(SasError, match="without splat groups"):
        r.render_backward(cam[0], cam[1], cam[2], cam[3], *gp, pose_groups=(0,))
    assert r.render_backward(cam[0], cam[1], cam[2], cam[3], *gp)["means"].abs().sum() > 0   # the context stays usable


def test_refine_group_poses_recovers(rasterizer):
    """The CPU recovery case with the same settings: the displaced group ends below a tenth of its start error, and within 5 % of the
    start error of where the float64 reference run ends (gpc.RECOVER_REF_END, which test_group_pose_cpu.py holds to that run)."""
    from sim_a_splat_amd.register import refine_group_poses
    r = rasterizer
    sc, cams, true, start, pivot = gpc.recovery_case()
    sc_kit.upload(r, sc)
    r.set_group_poses(true.reshape(-1, 12))
    images = np.stack([r.render(V, K, W, H)["rgb"].cpu().numpy() for V, K, W, H in cams])
    r.set_group_poses(start.reshape(-1, 12))
    W, H = cams[0][2], cams[0][3]
    res = refine_group_poses(r, images, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), W, H, [gpc.RECOVER_GROUP],
                             iters=gpc.RECOVER_ITERS, pivots=pivot, factors=(1,))
    g = gpc.RECOVER_GROUP
    (a0, d0), (a1, d1) = gpc.pose_error(start[g], true[g], pivot), gpc.pose_error(res.poses[g], true[g], pivot)
    a2, d2 = gpc.RECOVER_REF_END
    print(f"GROUP POSE refine_group_poses: {a0:.3f} deg, {d0:.4f} -> {a1:.4f} deg, {d1:.5f} (float64 reference: {a2:.4f} deg, {d2:.5f}); loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    assert a1 < 0.1 * a0 and d1 < 0.1 * d0
    assert abs(a1 - a2) < 0.05 * a0 and abs(d1 - d2) < 0.05 * d0
    np.testing.assert_allclose(r.get_group_poses().reshape(-1, 3, 4), res.poses, atol=1e-6)   # the poses are left at the result
    others = [k for k in range(len(true)) if k != g]
    assert np.array_equal(res.poses[others], start[others])


def test_door_b_refine_handle_poses():
    """Two groups through add_gaussian_splats; one handle displaced by 3 degrees and 2 cm is brought back below a tenth of both from two
    views, its wxyz is a unit quaternion, and the next get_render shows the refined pose."""
    from sim_a_splat_amd.poses import matrix_to_quat_wxyz, quat_wxyz_to_matrix
    from sim_a_splat_amd.register import se3_exp
    from sim_a_splat_amd.scene import SplatScene
    from sim_a_splat_amd.synthetic import c2w_opengl_from_viewmat
    rng = np.random.default_rng(3)
    scene = SplatScene(0)
    try:
        hs = []
        for k, centre in enumerate(([-0.35, 0.0, 0.0], [0.4, 0.05, 0.0])):
            n = 150
            c = rng.normal(0, 0.15, (n, 3)) + centre
            A = rng.normal(0, 0.05, (n, 3, 3))
            cov = A @ A.transpose(0, 2, 1) + 0.002 * np.eye(3)
            hs.append(scene.add_gaussian_splats(f"g{k}", c, cov, rng.uniform(0, 1, (n, 3)), rng.uniform(0.5, 0.95, n)))
        H, W, FOV = 48, 64, 0.5   # (vertical field of view in radians: the two groups fill the frame from the ring cameras' distance of 3)
        cams = []
        for yaw, elev in ((0.0, 0.2), (75.0, 0.3)):
            V = np.asarray(sc_kit.ring(W, H, f=60.0, yaw=yaw, elev=elev)[0], np.float64)
            c2w = np.linalg.inv(V)   # OpenCV axes, as the scene's cameras
            cams.append((matrix_to_quat_wxyz(c2w[:3, :3]), c2w[:3, 3].copy()))
        images = scene.get_renders(H, W, cams, fov=FOV)
        h = hs[1]
        xi = np.array([0.03, -0.03, 0.03, 0.012, -0.012, 0.012])
        centroid = np.asarray(scene._groups[1]["centers"], np.float64).mean(axis=0)
        Tp = np.eye(4)
        Tp[:3, 3] = centroid
        M = Tp @ se3_exp(xi) @ np.linalg.inv(Tp)
        h.wxyz, h.position = matrix_to_quat_wxyz(M[:3, :3]), M[:3, 3]
        err = lambda: (float(np.degrees(np.arccos(np.clip((np.trace(quat_wxyz_to_matrix(h.wxyz)) - 1) / 2, -1, 1)))),
                       float(np.linalg.norm(quat_wxyz_to_matrix(h.wxyz) @ centroid + h.position - centroid)))
        a0, d0 = err()
        moved = scene.get_renders(H, W, cams, fov=FOV)
        res = scene.refine_handle_poses([h], images, H, W, cams, fov=FOV, iters=120)
        a1, d1 = err()
        print(f"GROUP POSE door B: {a0:.3f} deg, {d0:.4f} -> {a1:.4f} deg, {d1:.5f}; loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
        assert a0 > 2.5 and d0 > 0.015
        assert a1 < 0.1 * a0 and d1 < 0.1 * d0
        assert abs(np.linalg.norm(h.wxyz) - 1.0) < 1e-12
        assert np.array_equal(hs[0].wxyz, [1, 0, 0, 0]) and np.array_equal(hs[0].position, [0, 0, 0])   # the other handle is as it was
        after = scene.get_renders(H, W, cams, fov=FOV).astype(np.int32)
        d_after, d_moved = np.abs(after - images.astype(np.int32)).mean(), np.abs(moved.astype(np.int32) - images.astype(np.int32)).mean()
        assert d_after < 0.2 * d_moved, (d_after, d_moved)   # the next frames show the refined pose
        np.testing.assert_allclose(scene.group_pose_rows().reshape(-1, 3, 4)[1], res.poses[1], atol=1e-5)
    finally:
        scene.close()
