"""CPU: the yardstick of the backward pass (tests/tools/grad_ref.py) and what the GPU tests assume of their cases (tests/tools/grad_cases.py).

- the reference's forward is oracle/np_twin.py's to 1e-10,
- its gradients are central finite differences of itself in float64 (every output, the view matrix included), also under a camera with
  fx != fy, an off-centre principal point and roll, and with Gaussians beyond the limits of the Jacobian's clamp,
- every GPU case keeps the masking and margin conditions of DESIGN.md 3, "Backward pass",
- the off-axis and clamp cases exercise what they are there for: the clamp binds (or does not), the clamped Gaussians carry weight, and a
  reference that is wrong in the clamp's gradient, in fx against fy or in the principal point is far outside the GPU bound,
- autograd.prechain is torch autograd of the frame's pointwise tail,
- the new entry points are declared, bound and built."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, autograd, build

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import grad_cases as gc  # noqa: E402
import grad_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402
from oracle import np_twin  # noqa: E402


def test_symbols_declared_and_listed():
    header = (Path(build.PKG).parent / "include" / "sim_a_splat_amd.h").read_text()
    for name in ("sas_render_backward_screen", "sas_render_backward"):
        assert name in _capi.EXPORTS and f"int {name}(" in header
    assert build.CSRC / "sas_grad.hip" in build.SOURCES


@pytest.mark.parametrize("name", gc.NAMES)
def test_forward_is_the_twin_and_case_conditions(name):
    sc, cam, _ = gc.case(name)
    V, K, W, H = cam
    ref = gc.reference(name)
    tw = np_twin.render(sc["means"], sc["op"], sc["colors"], V, K, W, H, quats=sc["quats"], scales=sc["scales"], cov6=sc["cov6"],
                        sh_degree=sc["sh"], group_id=sc["gid"], group_Rt=sc["Rt"] if sc["gid"] is not None else None)
    F = {k: torch.as_tensor(v) for k, v in ref["frame"].items()}
    out = grad_ref.finish(F)
    assert np.abs(out["rgb"].numpy() - tw["rgb"]).max() <= 1e-10
    assert np.abs(out["alpha"].numpy() - tw["alpha"][..., 0]).max() <= 1e-10
    assert np.abs(out["depth"].numpy() - tw["depth"][..., 0]).max() <= 1e-10
    assert np.array_equal(ref["valid"], tw["proj"]["valid"])
    # the conditions the GPU comparison rests on, from the reference alone
    assert ref["near"].mean() <= gc.MAX_MASKED, ref["near"].mean()
    assert not ref["margin"].any(), np.nonzero(ref["margin"])[0]
    # ... and the float32 reference takes every decision as the float64 one does
    assert np.array_equal(gc.reference(name, (True, True, True), "float32")["near"], ref["near"])


def test_two_view_scene_conditions():
    _, nears, _ = gc.two_view_reference()
    assert all(n.mean() <= gc.MAX_MASKED for n in nears)
    sc, cam, _ = gc.case("two_views")
    for c in (cam, gc.second_camera()):
        P = grad_ref.leaves(sc)
        with torch.no_grad():
            I = grad_ref.project(P, torch.tensor(np.asarray(c[0], np.float64)[:3]), c[1], c[2], c[3], sc["sh"])
        assert not I["margin"].any()


def test_dense_case_spans_batches_and_stops_pixels():
    sc, cam, _ = gc.case("dense_48x48")
    V, K, W, H = cam
    tw = np_twin.render(sc["means"], sc["op"], sc["colors"], V, K, W, H, quats=sc["quats"], scales=sc["scales"], sh_degree=sc["sh"])
    assert tw["n_isect"] / 9 > 256          # nine tiles: the mean list is longer than one staged batch
    ref = gc.reference("dense_48x48")
    T_final = 1.0 - ref["frame"]["alpha"]
    assert ((T_final < 1.0 / (1.0 - 0.999) * 1e-4) & (T_final > 1e-4)).sum() > 100   # pixels a further entry would have stopped or did stop


def _fd_case():
    """Six Gaussians on 16x16 with SH degree 1, and three more configurations of the same size: cov6, posed groups."""
    sc = sc_kit.synthetic(6, 3, 0.25)
    kk = 4
    sc = dict(sc, colors=np.ascontiguousarray(np.asarray(sc["colors"])[:, :kk]), sh=1, op=np.clip(np.asarray(sc["op"]), 0.3, 0.9).astype(np.float32),
              means=(0.3 * np.asarray(sc["means"])).astype(np.float32))
    return sc, sc_kit.ring(16, 16, f=40.0, yaw=25.0, elev=0.3)


FD_CAMERA = dict(W=16, H=16, fx=40.0, fy=32.0, cx=6.5, cy=9.5, eye=(3.0 * np.sin(np.deg2rad(25.0)), 0.3, 3.0 * np.cos(np.deg2rad(25.0))),
                 target=(-0.04, -0.17, 0.05), roll_deg=20.0)   # _fd_case's place; aimed so that the six Gaussians stay in the middle of the image
FD_CLAMP_Z, FD_CLAMP_OVER, FD_CLAMP_SCALE = 1.2, 1.06, 0.08


def _fd_clamped(sc, cam):
    """``sc`` plus two Gaussians close to the lens: one beyond the positive x limit of the Jacobian's clamp, one beyond the negative y
    limit (chosen on the CPU so that the test's precondition holds: no near pixel, no marginal Gaussian)."""
    V = np.asarray(cam[0], np.float64).reshape(4, 4)
    xp, _, _, yn = gc.clamp_limits(cam)
    z, s = FD_CLAMP_Z, FD_CLAMP_SCALE
    world = np.array([V[:3, :3].T @ (np.array([ux * z, uy * z, z]) - V[:3, 3]) for ux, uy in ((FD_CLAMP_OVER * xp, 0.05), (-0.03, -FD_CLAMP_OVER * yn))])
    cat = lambda a, b: np.concatenate([np.asarray(a), np.asarray(b, np.asarray(a).dtype)], 0)
    rng = np.random.default_rng(17)
    return dict(sc, means=cat(sc["means"], world), op=cat(sc["op"], [0.8, 0.7]),
                colors=cat(sc["colors"], 0.3 * rng.normal(size=(2,) + np.asarray(sc["colors"]).shape[1:])),
                quats=cat(sc["quats"], [[1, 0.1, -0.2, 0.1], [0.9, -0.2, 0.1, 0.3]]),
                scales=cat(sc["scales"], [[s, 0.9 * s, 1.1 * s], [1.1 * s, s, 0.9 * s]]))


def _loss(sc, cam, P, vm, g):
    _, _, I, F = grad_ref.forward(sc, cam, torch.float64, viewmat=vm, P=P)
    return (g[0] * F["acc_rgb"]).sum() + (g[1] * F["alpha"]).sum() + (g[2] * F["acc_z"]).sum(), F, I


@pytest.mark.parametrize("form", ["quats", "cov6", "groups", "general", "general_clamp"])
def test_gradients_are_finite_differences(form):
    sc, cam = _fd_case()
    if form.startswith("general"):
        cam = sc_kit.general(**FD_CAMERA)
    if form == "general_clamp":
        sc = _fd_clamped(sc, cam)
    if form == "cov6":
        sc = gc._cov6(sc)
    if form == "groups":
        sc = dict(sc, gid=(np.arange(6) % 3).astype(np.uint8), G=3, Rt=sc_kit.random_group_poses(3, 4))
    rng = np.random.default_rng(9)
    g = [torch.tensor(rng.normal(size=s)) for s in ((16, 16, 3), (16, 16), (16, 16))]
    P = grad_ref.leaves(sc)
    vm = torch.tensor(np.asarray(cam[0], np.float64)[:3], requires_grad=True)
    loss, F, I = _loss(sc, cam, P, vm, g)
    assert not F["near"].any() and not I["margin"].any() and I["valid"].all()
    assert (F["alpha"] > 0.05).sum() > 50   # the Gaussians show
    if form == "general_clamp":             # the two extras bind the clamp, and nothing else does
        (xp, xn, yp, yn), u = I["limits"], I["ratios"].numpy()
        assert u[-2, 0] > xp * (1 + grad_ref.MARGIN) and u[-1, 1] < -yn * (1 + grad_ref.MARGIN)
        assert np.all((u[:-2, 0] < xp) & (u[:-2, 0] > -xn) & (u[:-2, 1] < yp) & (u[:-2, 1] > -yn))
    loss.backward()
    leaves = dict(P, viewmat=vm)
    for name, t in leaves.items():
        if t is None:
            continue
        an = t.grad.numpy().reshape(-1)
        flat = t.detach().numpy().reshape(-1)
        scale = max(np.abs(an).max(), 1e-12)
        for idx in range(flat.size):
            h = 1e-6 * max(1.0, abs(flat[idx]))
            vals = []
            for s in (+1, -1):
                pert = flat.copy()
                pert[idx] += s * h
                Q = {k: (torch.tensor(pert.reshape(t.shape)) if k == name else (None if v is None else v.detach())) for k, v in P.items()}
                v2 = torch.tensor(pert.reshape(3, 4)) if name == "viewmat" else vm.detach()
                with torch.no_grad():
                    vals.append(float(_loss(sc, cam, Q, v2, g)[0]))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - an[idx]) <= 1e-5 * scale + 1e-9, (form, name, idx, fd, an[idx])


def test_prechain_is_autograd_of_the_pointwise_tail():
    rng = np.random.default_rng(2)
    H, W = 12, 10
    bg = (0.2, 0.0, 0.7)
    acc = torch.tensor(rng.uniform(0, 1.4, (H, W, 3)), requires_grad=True)
    a = torch.tensor(rng.uniform(0, 1, (H, W)), requires_grad=True)
    with torch.no_grad():
        a[0, :3] = 0.0                      # nothing composited: depth's guard
        acc[0, :3] = 0.0
        acc[1, 0] = 0.0                     # a pixel ON the lower bound (bg component 0 in channel 1 stays at 0)
    accz = torch.tensor(rng.uniform(0, 3, (H, W)) * a.detach().numpy(), requires_grad=True)
    rgb = torch.clamp(acc + (1 - a)[..., None] * torch.tensor(bg, dtype=torch.float64), 0, 1)
    depth = accz / torch.clamp(a, min=1e-10)
    g = [torch.tensor(rng.normal(size=s)) for s in ((H, W, 3), (H, W), (H, W))]
    assert (rgb == 1).any() and (rgb == 0).any()
    for which in ((0, 1, 2), (0,), (1,), (2,)):
        gs = [g[k] if k in which else None for k in range(3)]
        exp = torch.autograd.grad(sum((g[k] * (rgb, a, depth)[k]).sum() for k in which), [acc, a, accz], allow_unused=True, retain_graph=True)
        got = autograd.prechain(rgb.detach(), a.detach()[..., None], depth.detach()[..., None], bg, *gs)
        for x, y in zip(got, exp):
            y = torch.zeros_like(x) if y is None else y
            assert torch.allclose(x, y, rtol=1e-12, atol=1e-12)


def test_pose_case_has_no_nearer_minimum():
    """The loss of register.refine_camera_pose, evaluated by the reference at the coarsest level the optimiser starts on, falls
    monotonically along the straight twist from the perturbed camera of grad_cases.pose_case to the true one."""
    from sim_a_splat_amd.register import se3_exp
    sc, (V, K, W, H), xi = gc.pose_case()
    w, h = W // 4, H // 4
    Kc = np.asarray(K, np.float64).copy()
    Kc[0] *= w / W
    Kc[1] *= h / H
    P = {k: (None if v is None else v.detach()) for k, v in grad_ref.leaves(sc).items()}

    def rgb(Vc):
        with torch.no_grad():
            F = grad_ref.forward(sc, (Vc, Kc, w, h), viewmat=torch.tensor(np.asarray(Vc, np.float64)[:3]), P=P)[3]
            return grad_ref.finish(F)["rgb"]
    target = rgb(np.asarray(V, np.float64))
    losses = [float(((rgb(se3_exp((1.0 - t) * xi) @ np.asarray(V, np.float64)) - target) ** 2).mean()) for t in np.linspace(0.0, 1.0, 6)]
    assert all(a > b for a, b in zip(losses, losses[1:])) and losses[-1] == 0.0, losses


@pytest.mark.parametrize("factor", [4, 2, 1])
def test_offaxis_pose_case_has_no_nearer_minimum(factor):
    """test_pose_case_has_no_nearer_minimum for grad_cases.pose_case_offaxis (fx != fy, the principal point a fifth of the image off the
    centre, roll), at each of the three levels of register.refine_camera_pose with K's two rows rescaled as it rescales them."""
    from sim_a_splat_amd.register import se3_exp
    sc, (V, K, W, H), xi = gc.pose_case_offaxis()
    assert K[0, 0] != K[1, 1] and abs(K[0, 2] - W / 2) > 0.1999 * W and abs(K[1, 2] - H / 2) > 0.1999 * H   # (K is float32)
    w, h = W // factor, H // factor
    Kc = np.asarray(K, np.float64).copy()
    Kc[0] *= w / W
    Kc[1] *= h / H
    P = {k: (None if v is None else v.detach()) for k, v in grad_ref.leaves(sc).items()}

    def rgb(Vc):
        with torch.no_grad():
            F = grad_ref.forward(sc, (Vc, Kc, w, h), viewmat=torch.tensor(np.asarray(Vc, np.float64)[:3]), P=P)[3]
            return grad_ref.finish(F)["rgb"]
    target = rgb(np.asarray(V, np.float64))
    losses = [float(((rgb(se3_exp((1.0 - t) * xi) @ np.asarray(V, np.float64)) - target) ** 2).mean()) for t in np.linspace(0.0, 1.0, 6)]
    assert all(a > b for a, b in zip(losses, losses[1:])) and losses[-1] == 0.0, losses


NEW_CASES = ("offaxis",) + gc.CLAMP_NAMES
GPU_FACTOR = 4.0   # tests/test_gpu_t_backward.py's FACTOR: the GPU bound is this times the float32 reference's figure


@pytest.mark.parametrize("name", NEW_CASES)
def test_offaxis_and_clamp_case_conditions(name):
    """From the reference alone.  The camera is off-axis; in the "clamp*" cases each of the four limits of the Jacobian's clamp is
    exceeded by a VALID Gaussian by more than the margin, the published ones among them, and in "offaxis" none is; each published clamp
    Gaussian carries at least 5 % of the case's largest gradient of the means and of the scales (of the covariances in the cov6 form);
    and every figure of the float32 reference is at most 1e-5, as in the cases before these."""
    sc, cam, _ = gc.case(name)
    V, K, W, H = cam
    assert K[0, 0] != K[1, 1] and K[0, 2] != W / 2 and K[1, 2] != H / 2
    assert not np.allclose(np.asarray(V)[0, :3] @ [0.0, 1.0, 0.0], 0.0, atol=0.1)   # roll: the camera's x axis is not level
    ref = gc.reference(name)
    with torch.no_grad():
        I = grad_ref.forward(sc, cam)[2]
    (xp, xn, yp, yn), u, valid = I["limits"], I["ratios"].numpy(), ref["valid"]
    assert np.allclose((xp, xn, yp, yn), gc.clamp_limits(cam), rtol=1e-12) and len({xp, xn, yp, yn}) == 4   # four limits, all apart
    m = 1 + grad_ref.MARGIN
    over = [valid & (u[:, 0] > xp * m), valid & (u[:, 0] < -xn * m), valid & (u[:, 1] > yp * m), valid & (u[:, 1] < -yn * m)]
    inside = (u[:, 0] < xp) & (u[:, 0] > -xn) & (u[:, 1] < yp) & (u[:, 1] > -yn)
    if name == "offaxis":
        assert valid.all() and inside.all()
    else:
        n = len(valid)
        idx = {k: n + i for k, i in gc.CLAMP.items()}
        assert valid[list(idx.values())].all()
        assert over[0][idx["x_pos"]] and over[1][idx["x_neg"]] and over[2][idx["y_pos"]] and over[3][idx["y_neg"]]
        assert over[0][idx["corner"]] and over[3][idx["corner"]]
        assert inside[:n - 5].all()   # the blob is as in "offaxis"
        if name == "clamp_groups":
            gid = np.asarray(sc["gid"])
            G = np.asarray(sc["Rt"], np.float64).reshape(-1, 3, 4)[gc.CLAMP_GROUP]
            assert np.all(gid[-5:] == gc.CLAMP_GROUP) and not np.allclose(G[:, :3], np.eye(3), atol=1e-2) and np.abs(G[:, 3]).max() > 1e-2
        for k in ("means", "covariances" if name == "clamp_cov6" else "scales"):
            a = np.abs(ref["full"][k])
            share = a[list(idx.values())].max(axis=1) / a.max()
            assert share.min() >= 0.05, (k, share)
    e = gc.float32_errors(name)
    worst = max(max(e["screen"].values()), max(e["full"].values()))
    assert worst <= 1e-5, e


@pytest.mark.parametrize("name,kind", [("offaxis", "swap_f"), ("offaxis", "centred")] + [(n, "straight_through") for n in gc.CLAMP_NAMES])
def test_offaxis_and_clamp_cases_are_sensitive(name, kind):
    """A reference that is wrong in one way -- fx and fy exchanged, the principal point centred, the clamp's gradient passed straight
    through to x and y (grad_ref.project's mutant; its forward is the reference's) -- misses the GPU test's bound on ``means`` and on
    ``viewmat`` by more than a factor of 100: an implementation with that error cannot pass."""
    ref, e = gc.reference(name)["full"], gc.float32_errors(name)["full"]
    mut = gc.mutant_reference(name, kind)
    for k in ("means", "viewmat"):
        d = grad_ref.rel_err(mut[k], ref[k])
        print(f"BACKWARD mutant {kind} on {name}: {k} off by {d:.3e}, GPU bound {GPU_FACTOR * e[k]:.3e}")
        assert d > 100 * GPU_FACTOR * e[k], (k, d, e[k])
    if kind == "straight_through":
        sc, cam, _ = gc.case(name)
        with torch.no_grad():
            a, b = grad_ref.forward(sc, cam)[3], grad_ref.forward(sc, cam, straight_through=True)[3]
        assert all(torch.equal(a[k], b[k]) for k in a)   # the same frame: only the derivative differs


def test_extras_upstream_covers_the_clamped_gaussians():
    """The GPU test that holds the five extras' rows of "clamp" alone: its upstream gradients are zero outside their rectangles and at the
    masked pixels, every extra's rows of means, quats and scales receive, and on EACH extra's row of ``means`` the straight-through mutant
    is off by more than 100 times that test's bound, four times the float32 figure, in that test's measure (over the five rows)."""
    g, inside = gc.extras_upstream()
    near = gc.reference("clamp")["near"]
    assert 0 < inside.sum() and all(np.all(gi[~inside | near] == 0) for gi in g)
    rows, r32 = gc.extras_reference(), gc.extras_reference("float32")
    for k in gc.EXTRA_ROWS:
        assert rows[k].shape[0] == 5 and np.all(np.abs(rows[k]).max(axis=1) > 0), k
        assert grad_ref.rel_err(r32[k], rows[k]) <= 1e-5
    sc, cam, _ = gc.case("clamp")
    mut = grad_ref.gradients(sc, cam, *g, mask_near=False, straight_through=True)["full"]["means"][list(gc.CLAMP.values())]
    off = np.abs(mut - rows["means"]).max(axis=1) / np.abs(rows["means"]).max()
    assert off.min() > 100 * GPU_FACTOR * grad_ref.rel_err(r32["means"], rows["means"]), off


def test_special_case_clamps_alpha_at_its_pixel():
    """From the reference alone: the opacity-1 Gaussian of "special" has o e^-sigma beyond 0.999 by more than the margin at
    grad_cases.CLAMP_PIXEL, that pixel is not masked, the Gaussian is the frontmost entry there, and the reference passes nothing through
    the clamp to its opacity, conic or mean while its colour receives."""
    sc, cam, g = gc.case("special")
    x, y = gc.CLAMP_PIXEL
    i = gc.SPECIAL["clamped"]
    ref = gc.reference("special")
    with torch.no_grad():
        _, _, I, F = grad_ref.forward(sc, cam)
    m2, con = I["means2d"][i].numpy(), I["conics"][i].numpy()
    dx, dy = m2[0] - (x + 0.5), m2[1] - (y + 0.5)
    oE = float(I["opacities"][i]) * np.exp(-(0.5 * (con[0] * dx * dx + con[2] * dy * dy) + con[1] * dx * dy))
    assert oE > 0.999 * (1 + grad_ref.MARGIN), oE
    assert not ref["near"][y, x]
    assert bool(I["valid"][i]) and float(I["depths"][i]) < float(I["depths"][:i][I["valid"][:i]].min())
    only = np.zeros(ref["near"].shape, bool)
    only[y, x] = True
    one = grad_ref.gradients(sc, cam, *[gi * (only[..., None] if gi.ndim == 3 else only) for gi in g], mask_near=False)["screen"]
    assert all(np.all(one[k][i] == 0) for k in ("opacities", "means2d", "conics")) and np.all(one["colors"][i] != 0)
    assert (1.0 - ref["frame"]["alpha"][y, x]) < 0.0011   # T behind the clamped entry is 1 - 0.999 at most


def test_refine_camera_pose_on_the_reference_renderer():
    """register.refine_camera_pose with its ``loss_and_grad`` hook: the same optimiser on the float64 reference, a 120-Gaussian scene at
    32x32, 3 degrees and 3 cm off, two levels of 45 iterations."""
    import lift_ref as lr
    from sim_a_splat_amd.register import refine_camera_pose, se3_exp
    sc = lr.blob_scene(120, 3, 0.12)
    V, K, W, H = sc_kit.ring(32, 32, f=30.0, yaw=10.0, elev=0.2)
    P = {k: (None if v is None else v.detach()) for k, v in grad_ref.leaves(sc).items()}

    def frame(Vc, Kc, w, h, grad):
        vm = torch.tensor(np.asarray(Vc, np.float64)[:3], requires_grad=grad)
        return vm, grad_ref.finish(grad_ref.forward(sc, (Vc, Kc, w, h), viewmat=vm, P=P)[3])["rgb"]

    def loss_and_grad(Vc, Kc, w, h, target, mask):
        vm, rgb = frame(Vc, Kc, w, h, True)
        loss = (mask.double()[..., None] * (rgb - target.double()) ** 2).sum() / (3 * mask.sum())
        loss.backward()
        return float(loss.detach()), vm.grad.numpy()
    with torch.no_grad():
        target = frame(V, K, W, H, False)[1].float().numpy()
    xi = np.array([0.03, -0.03, 0.02, 0.02, -0.015, 0.017])
    xi[:3] *= np.deg2rad(3.0) / np.linalg.norm(xi[:3])
    xi[3:] *= 0.03 / np.linalg.norm(xi[3:])
    V0 = se3_exp(xi) @ np.asarray(V, np.float64)
    res = refine_camera_pose(None, target, V0, K, W, H, iters=90, factors=(2, 1), loss_and_grad=loss_and_grad, pivot_depth=3.0)
    a0, d0 = gc.pose_error(V0, V)
    a1, d1 = gc.pose_error(res.viewmat, V)
    assert a0 > 2.9 and d0 > 0.02
    assert a1 < 0.1 * a0 and d1 < 0.2 * d0, (a1, d1)   # (90 iterations: the GPU test runs 300 and holds both to a tenth)
    assert res.history[-1][1] < 1e-3 * res.history[0][1]


def test_float32_error_table_of_the_gpu_test_is_current():
    """tests/test_gpu_t_backward.py's F32_ERR (its bounds are four times it) is what grad_cases.float32_errors computes for today's cases:
    the same keys, every figure within 25 % (the table keeps three digits; float32 sums may differ in their last bits between hosts)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpu_t_backward", Path(__file__).resolve().parent / "test_gpu_t_backward.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert set(mod.F32_ERR) == {f"{n}:{m}" for n, m in gc.RUNS} | {"two_views", "clamp:extras"} | set(gc.L2_KEYS)
    for name, mode in gc.RUNS:
        now = gc.float32_errors(name, mode)
        for part in ("screen", "full"):
            table = mod.F32_ERR[f"{name}:{mode}"][part]
            assert set(table) == set(now[part])
            for k, v in now[part].items():
                assert abs(table[k] - v) <= 0.25 * v + 1e-12, (name, mode, part, k, table[k], v)
    a, b = gc.two_view_reference()[0], gc.two_view_reference("float32")[0]
    rows = [("two_views", a, b), ("clamp:extras", gc.extras_reference(), gc.extras_reference("float32"))]
    rows += [(key, gc.l2_reference(name)[0], gc.l2_reference(name, "float32")[0]) for key, name in gc.L2_KEYS.items()]
    for key, x64, x32 in rows:
        assert set(mod.F32_ERR[key]) == set(x64)
        for k in x64:
            v = grad_ref.rel_err(x32[k], x64[k])
            assert abs(mod.F32_ERR[key][k] - v) <= 0.25 * v + 1e-12, (key, k, mod.F32_ERR[key][k], v)
