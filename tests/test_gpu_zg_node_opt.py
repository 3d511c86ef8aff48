"""GPU: the node optimiser on the device (sas_nodes_rigidity, sas_nodes_twist_step; Rasterizer.node_rigidity / node_twist_step,
deform.NodeOptimizer, fit_node_transforms(optimizer="device"), fit_dynamic_scene(optimizer="device"); DESIGN.md 3, "Deformation") against
tests/tools/node_opt_ref.py.  The rigidity kernel is held to deform.rigidity(table=) within the kit's derived rounding bound; the step kernel to
deform._twist_step within FOUR times the kit's yardstick, which is the float64 reference's own error against np.longdouble (the measured ratios
are printed); the loops to the existing recovery tests' conditions."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import node_opt_ref as no  # noqa: E402
import skin_grad_ref as sg  # noqa: E402
import skin_ref as sr  # noqa: E402
import skin_rest_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(r, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(r.device)


def _rigidity(r, c, T=None):
    nb, (rs, re) = c["nb"], c["rev"]
    has = nb.shape[1] > 0
    res = r.node_rigidity(_dev(r, c["nodes"]), _dev(r, c["T"] if T is None else T), _dev(r, nb) if has else None, _dev(r, rs) if has else None,
                          _dev(r, re) if has else None)
    return float(res["value"].cpu()), res["d_transforms"].cpu().numpy()


# ---- the rigidity kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(no.RIGIDITY_CASES))
def test_rigidity_kernel_is_the_host_rigidity_within_the_rounding_bound(rasterizer, name):
    c = no.rigidity_case(name)
    value, grad = _rigidity(rasterizer, c)
    off = np.abs(grad - c["grad"])
    print(f"  {name}: value {value:.6e} off by {abs(value - c['value']):.2e} (bound {c['value_bound']:.2e}); gradient off by {off.max():.2e}, "
          f"the largest |device - host| / bound {np.max(off / np.maximum(c['grad_bound'], 1e-300)):.3f}")
    assert abs(value - c["value"]) <= c["value_bound"]
    assert (off <= c["grad_bound"]).all()
    if c["nb"].shape[1] == 0:
        assert value == 0.0 and not grad.any()
    again = _rigidity(rasterizer, c)
    assert again[0] == value and np.array_equal(again[1], grad)   # no atomics: the same bits


def test_one_rigid_motion_of_all_nodes_is_zero_at_the_rounding_bound(rasterizer):
    c = no.rigidity_case("drawn2049")
    T = np.repeat(no.rigid_transforms(np.random.default_rng(3), 1), 2049, axis=0)
    vb, gb = no.rigidity_bound(c["nodes"], T, c["nb"])
    value, grad = _rigidity(rasterizer, c, T)
    print(f"  one rigid motion: value {value:.2e} (bound {vb:.2e}), gradient {np.abs(grad).max():.2e} (bound {gb.max():.2e})")
    assert abs(value) <= vb and (np.abs(grad) <= gb).all()


# ---- the step kernel ----------------------------------------------------------------------------------------------------------------------------
def _rates(c):
    it, per = c["it"], c["per"]
    decay = 0.05 ** (it / max(1, per - 1))
    return dict(lr=(c["step"][0] * decay, c["step"][1] * decay), c1=1 - 0.9 ** (it + 1), c2=1 - 0.999 ** (it + 1))


def _step(r, c, d32=True, d64=True, weight=None, d64_values=None):
    T, m1, m2 = _dev(r, c["T"]), _dev(r, c["m1"]), _dev(r, c["m2"])
    T32 = torch.full(c["T"].shape, float("nan"), dtype=torch.float32, device=r.device)
    r.node_twist_step(_dev(r, c["nodes"]), T, m1, m2, T32, _dev(r, c["d32"]) if d32 else None,
                      _dev(r, c["d64"] if d64_values is None else d64_values) if d64 else None, c["weight"] if weight is None else weight, **_rates(c))
    return T.cpu().numpy(), m1.cpu().numpy(), m2.cpu().numpy(), T32.cpu().numpy()


STEP_HAS_ZERO = {name: spec[5] for name, spec in no.STEP_CASES.items()}


@pytest.mark.parametrize("name", list(no.STEP_CASES))
def test_step_kernel_within_four_yardsticks_of_the_host_step(rasterizer, name):
    c = no.step_case(name)
    T, m1, m2, T32 = _step(rasterizer, c)
    ratios = no.step_ratios(c, T, m1, m2)
    print(f"  {name}: device / yardstick " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 4.0, ratios
    assert np.array_equal(T32.view(np.uint32), T.astype(np.float32).view(np.uint32))   # rounded once
    again = _step(rasterizer, c)
    assert all(np.array_equal(a, b) for a, b in zip(again, (T, m1, m2, T32)))
    if STEP_HAS_ZERO[name]:   # the exponential's series branch: a zero gradient on zero moments moves nothing
        z = c["nodes"].shape[0] // 2
        assert np.abs(T[z] - c["T"][z]).max() <= 4.0 * no.step_yardstick(c)["T"] and not m1[z].any() and not m2[z].any()


def test_step_kernel_gradient_parts_are_consistent(rasterizer):
    r = rasterizer
    c = no.step_case("mid_m257")
    alone32 = _step(r, c, d64=False)
    # ... is the sum with a weight of zero, and is the float64 part alone when that holds the same numbers
    assert all(np.array_equal(a, b) for a, b in zip(alone32, _step(r, c, weight=0.0)))
    assert all(np.array_equal(a, b) for a, b in zip(alone32, _step(r, c, d32=False, weight=1.0, d64_values=c["d32"].astype(np.float64))))
    # either part alone is the host's step on that part
    from sim_a_splat_amd import deform
    for kw, dT in ((dict(d64=False), c["d32"].astype(np.float64)), (dict(d32=False), c["weight"] * c["d64"])):
        part = dict(c, dT=dT, ref=deform._twist_step(c["T"], dT, c["nodes"].astype(np.float64), c["m1"], c["m2"], c["it"], c["per"], c["step"]))
        ratios = no.step_ratios(part, *_step(r, c, **kw)[:3])
        print(f"  {sorted(kw)[0]} off: device / yardstick " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
        assert max(ratios.values()) <= 4.0, ratios


def test_a_thousand_chained_steps_stay_rigid(rasterizer):
    from sim_a_splat_amd import deform
    r = rasterizer
    c = no.step_case("first_m257")
    rng = np.random.default_rng(9)
    pool = [_dev(r, rng.normal(size=c["d32"].shape).astype(np.float32) * 0.05) for _ in range(8)]
    g, T, m1, m2 = _dev(r, c["nodes"]), _dev(r, c["T"]), _dev(r, c["m1"]), _dev(r, c["m2"])
    T32 = torch.empty(c["T"].shape, dtype=torch.float32, device=r.device)
    for it in range(1000):
        decay = 0.05 ** (it / 999)
        r.node_twist_step(g, T, m1, m2, T32, pool[it % 8], lr=(0.01 * decay, 0.01 * decay), c1=1 - 0.9 ** (it + 1), c2=1 - 0.999 ** (it + 1))
    out, R = T32.cpu().numpy(), T.cpu().numpy()[:, :, :3]
    deform.check_node_transforms(out)
    drift = np.abs(np.einsum("mki,mkj->mij", R, R) - np.eye(3)).max()
    moved = np.abs(T.cpu().numpy() - c["T"]).max()
    print(f"  1000 steps: the float64 state's |R^T R - I| {drift:.2e}; the transforms moved by up to {moved:.3f}")
    assert drift < 1e-12 and moved > 0.1


# ---- NodeOptimizer.step against the host --------------------------------------------------------------------------------------------------------
def test_node_optimizer_step_is_rigidity_and_twist_step_on_the_host(rasterizer):
    """The recovery case's nodes and sheet, a drawn start, the gradient of ONE real deform_backward: the rigidity kernel against
    deform.rigidity(table=) within the rounding bound, and the step against deform._twist_step on double(dT) + w * (the device's rigidity
    gradient, read back) within four yardsticks -- each kernel's bound on its own part."""
    from sim_a_splat_amd import deform
    from sim_a_splat_amd.autograd import prechain
    r = rasterizer
    c = sg.recovery_case()
    r.upload(**c["upload"])
    r.set_skin(c["indices"], c["weights"])
    start = no.rigid_transforms(np.random.default_rng(5), 9, angle=0.05, shift=0.02)
    opt = deform.NodeOptimizer(r, c["nodes"], transforms=start)
    assert opt.k == 6 and np.array_equal(opt.table.cpu().numpy(), no.knn_table(c["nodes"], 6))
    assert np.array_equal(opt.table.cpu().numpy(), deform._neighbour_table(c["nodes"], 6))   # (spacing 0.5: the two searches agree)
    assert np.array_equal(opt.transforms.cpu().numpy(), start.astype(np.float32)) and np.array_equal(opt.read(), start)
    r.deform(opt.transforms)
    V, K = c["cams"][0][0].astype(np.float32), c["cams"][0][1].astype(np.float32)
    out = r.render(V, K, sg.RECOVER_W, sg.RECOVER_H, (0.0, 0.0, 0.0))
    rgb, alpha, depth = out["rgb"].clone(), out["alpha"].clone(), out["depth"].clone()
    diff = rgb - torch.from_numpy(c["images"][0].astype(np.float32)).to(r.device)
    g_acc, g_a, g_z = prechain(rgb, alpha, depth, (0.0, 0.0, 0.0), 2.0 * diff / diff.numel(), None, None)
    dT = r.deform_backward(r.render_backward(V, K, sg.RECOVER_W, sg.RECOVER_H, g_acc, g_a, g_z, want=("means", "quats")))
    # the rigidity part
    value, d_reg = opt.rigidity()
    value, d_reg = float(value.cpu()), d_reg.cpu().numpy()
    host_value, host_reg = deform.rigidity(c["nodes"], start, table=opt.table.cpu().numpy())
    vb, gb = no.rigidity_bound(c["nodes"], start, opt.table.cpu().numpy())
    assert abs(value - host_value) <= vb and (np.abs(d_reg - host_reg) <= gb).all() and host_value > 0.0
    # the step
    it, per, w = 3, 30, 0.01
    opt.m1.copy_(_dev(r, np.random.default_rng(1).normal(size=(9, 6)) * 1e-3))
    opt.m2.copy_(_dev(r, np.random.default_rng(2).uniform(0.5, 2.0, (9, 6)) * 1e-6))
    m1, m2 = opt.m1.cpu().numpy(), opt.m2.cpu().numpy()
    total = dT.double().cpu().numpy() + w * d_reg
    case = dict(T=start, dT=total, nodes=c["nodes"], m1=m1, m2=m2, it=it, per=per, step=(0.01, 0.01),
                ref=deform._twist_step(start, total, c["nodes"].astype(np.float64), m1, m2, it, per, (0.01, 0.01)))
    got = opt.step(dT, it, per, (0.01, 0.01), w)
    assert float(got.cpu()) == value
    ratios = no.step_ratios(case, opt.read(), opt.m1.cpu().numpy(), opt.m2.cpu().numpy())
    print(f"  NodeOptimizer.step: rigidity {value:.4e} (host {host_value:.4e}); device / yardstick " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 4.0, ratios
    assert np.array_equal(opt.transforms.cpu().numpy(), opt.read().astype(np.float32))
    opt.reset_moments()
    assert not opt.m1.any() and not opt.m2.any()
    assert float(opt.step(dT, 0, per, (0.01, 0.01), 0.0).cpu()) == 0.0   # a weight of zero: no rigidity kernel, an exact zero
    r.clear_skin()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(rasterizer):
    from sim_a_splat_amd import deform
    r, L = rasterizer, _capi.lib()
    c = no.rigidity_case("grid3x3")
    g, T, nb = _dev(r, c["nodes"]), _dev(r, c["T"]), _dev(r, c["nb"])
    rs, re = _dev(r, c["rev"][0]), _dev(r, c["rev"][1])
    d, v = torch.empty((9, 3, 4), dtype=torch.float64, device=r.device), torch.empty(1, dtype=torch.float64, device=r.device)
    p = lambda t: t.data_ptr()
    rig = lambda m, kn, nodes=p(g): L.sas_nodes_rigidity(r._ctx, m, nodes, p(T), kn, p(nb), p(rs), p(re), p(d), p(v), None)
    assert rig(9, 6) == 0
    for m, kn in ((0, 6), (65537, 6), (9, 9), (9, -1)):
        assert rig(m, kn) == -1, (m, kn)
    assert rig(9, 6, None) == -1
    assert rig(9, 9) == -1 and b"kn=9" in L.sas_last_error(r._ctx)
    m1, m2 = torch.zeros((9, 6), dtype=torch.float64, device=r.device), torch.zeros((9, 6), dtype=torch.float64, device=r.device)
    T32, d32 = torch.empty((9, 3, 4), dtype=torch.float32, device=r.device), torch.zeros((9, 3, 4), dtype=torch.float32, device=r.device)
    before = T.clone()

    def step(m=9, d32p=p(d32), d64p=None, **kw):
        cfg = _capi.NodeStepConfig(**dict(dict(lr_rot=0.01, lr_trans=0.01, beta1=0.9, beta2=0.999, c1=0.1, c2=0.001, eps=1e-12, gain1=0.1, gain2=0.001), **kw))
        return L.sas_nodes_twist_step(r._ctx, m, p(g), d32p, d64p, 1.0, p(T), p(m1), p(m2), p(T32), ctypes.byref(cfg), None)
    for bad in (dict(m=0), dict(m=65537), dict(d32p=None), dict(lr_rot=-1.0), dict(lr_trans=float("nan")), dict(lr_rot=float("inf")), dict(beta1=1.0),
                dict(beta2=-0.1), dict(c1=0.0), dict(c2=-1.0), dict(gain1=0.0), dict(eps=float("nan"))):
        assert step(**bad) == -1, bad
    assert step(d32p=None) == -1 and b"d_Rt32 and d_Rt64" in L.sas_last_error(r._ctx)
    torch.cuda.synchronize(r.device)
    assert torch.equal(T, before)   # a refused call changes nothing
    assert step() == 0
    # the mirrors
    with pytest.raises(ValueError, match="out of"):
        r.node_rigidity(torch.zeros((0, 3), device=r.device), torch.zeros((0, 3, 4), dtype=torch.float64, device=r.device))
    with pytest.raises(ValueError, match="kn <= 8"):
        r.node_rigidity(g, T, torch.zeros((9, 9), dtype=torch.int32, device=r.device), rs, re)
    with pytest.raises(ValueError, match="rev_edge"):
        r.node_rigidity(g, T, nb, rs, re[:10])
    with pytest.raises(ValueError, match="transforms64"):
        r.node_rigidity(g, T.float(), nb, rs, re)
    with pytest.raises(ValueError, match="one of d_transforms"):
        r.node_twist_step(g, T, m1, m2, T32, lr=(0.01, 0.01), c1=0.1, c2=0.001)
    with pytest.raises(ValueError, match="neighbours=9"):
        deform.NodeOptimizer(r, c["nodes"], neighbours=9)
    bad = c["nodes"].copy()
    bad[4, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        deform.NodeOptimizer(r, bad)
    with pytest.raises(ValueError, match="not with loss_and_grad"):
        deform.fit_node_transforms(r, np.zeros((1, 4, 4, 3)), np.eye(4)[None], np.eye(3)[None], 4, 4, c["nodes"], optimizer="device",
                                   loss_and_grad=lambda *a: (0.0, np.zeros((9, 3, 4))))
    with pytest.raises(ValueError, match="optimizer must be"):
        deform.fit_node_transforms(r, np.zeros((1, 4, 4, 3)), np.eye(4)[None], np.eye(3)[None], 4, 4, c["nodes"], optimizer="gpu")
    single = deform.NodeOptimizer(r, c["nodes"][:1])   # one node: no neighbours, no table
    assert single.k == 0 and single.table is None and float(single.rigidity()[0].cpu()) == 0.0


# ---- recovery ---------------------------------------------------------------------------------------------------------------------------------------
def test_fit_node_transforms_on_the_device_recovers_the_bend(rasterizer):
    """test_gpu_ze_skin_grad.py's recovery test with optimizer="device": its two conditions, r left deformed at the result, the history."""
    from sim_a_splat_amd import deform
    r = rasterizer
    c = sg.recovery_case()
    r.upload(**c["upload"])
    r.set_skin(c["indices"], c["weights"])
    V, K = np.stack([cam[0] for cam in c["cams"]]), np.stack([cam[1] for cam in c["cams"]])
    res = deform.fit_node_transforms(r, c["images"], V, K, sg.RECOVER_W, sg.RECOVER_H, c["nodes"], iters=sg.RECOVER_ITERS, optimizer="device")
    e0, e1 = sg.recovery_error(c, sr.identity_transforms(9)), sg.recovery_error(c, res.transforms)
    print(f"  recovery with the device optimiser: mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start (the reference run: "
          f"{sg.RECOVER_REF_END}); loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    assert abs(e1 / e0 - sg.RECOVER_REF_END) < 0.05
    assert e1 < sg.RECOVER_FRACTION * e0
    assert res.transforms.shape == (9, 3, 4) and res.transforms.dtype == np.float64 and len(res.history) == sg.RECOVER_ITERS + 1
    assert all(np.isfinite(x) for _, x in res.history) and [f for f, _ in res.history] == [2] * 30 + [1] * 31 and res.loss == res.history[-1][1]
    now = r.read_scene()["means"].cpu().numpy()
    want = sr.deform_ref(c["rest"], c["indices"], c["weights"], res.transforms.astype(np.float32))["means"]
    assert np.abs(now - want).max() < 1e-5
    r.clear_skin()


def _look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(wxyz, position) of a camera at ``position`` looking at ``target``: camera-to-world, OpenCV axes (x right, y down, z forward)."""
    from sim_a_splat_amd.poses import matrix_to_quat_wxyz
    p = np.asarray(position, np.float64)
    z = np.asarray(target, np.float64) - p
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return tuple(matrix_to_quat_wxyz(np.stack([x, np.cross(z, x), z], axis=1))), tuple(p)


def test_door_b_fits_its_deformable_group_with_the_device_optimiser():
    """test_gpu_ze_skin_grad.py's Door B test through SplatScene.fit_deformation(..., optimizer="device"): its condition."""
    from sim_a_splat_amd.scene import SplatScene
    W, H = 64, 48
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
        scene.bind_deformable(cloth, c["nodes"], k=4)
        cams = [_look_at((0.0, -0.5, 1.4)), _look_at((1.1, 0.3, 1.0))]
        rows = slice(n0, n0 + sg.RECOVER_N)
        scene.deform(c["truth"].astype(np.float32))
        images = scene.get_renders(H, W, cams, fov=0.9).copy()
        truth = scene._raster.read_scene()["means"].cpu().numpy()[rows]
        scene.deform(sr.identity_transforms(9))
        rest_frame = scene.get_render(H, W, *cams[0], fov=0.9).astype(np.float64)
        rest = scene._raster.read_scene()["means"].cpu().numpy()[rows]
        res = scene.fit_deformation(images, H, W, cams, fov=0.9, iters=sg.RECOVER_ITERS, optimizer="device")
        after = scene._raster.read_scene()["means"].cpu().numpy()[rows]
        e0, e1 = np.linalg.norm(rest - truth, axis=1).mean(), np.linalg.norm(after - truth, axis=1).mean()
        f1 = scene.get_render(H, W, *cams[0], fov=0.9).astype(np.float64)
        d0, d1 = np.abs(rest_frame - images[0]).mean(), np.abs(f1 - images[0]).mean()
        print(f"  Door B with the device optimiser: mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start; frame difference {d0:.3f} -> "
              f"{d1:.3f} (of 255); loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
        assert e1 < sg.RECOVER_FRACTION * e0
        assert d1 < 0.5 * d0
        assert res.transforms.shape == (9, 3, 4) and scene._raster.has_skin
    finally:
        scene.close()


def test_fit_dynamic_scene_joint_with_the_device_optimiser_follows_the_host_run(rasterizer):
    """skin_rest_ref's joint case, fit_transforms=True, with both optimisers on the same rasterizer: the device run's loss history is held to the
    host run's as test_gpu_zf_skin_rest.py holds the host run to its reference -- every iteration within 0.05 of the start loss."""
    from sim_a_splat_amd import deform
    r = rasterizer
    c = rr.dynamic_case()
    runs = {}
    for mode in ("host", "device"):
        r.upload(**c["start"])
        r.set_skin(c["indices"], c["weights"])
        runs[mode] = deform.fit_dynamic_scene(r, c["frames"], c["nodes"], optimizer=mode, **rr.dynamic_settings(True))
        r.clear_skin()
    host, dev = runs["host"], runs["device"]
    off = np.abs(np.asarray(dev.history) - np.asarray(host.history)).max() / host.history[0]
    moved = np.abs(dev.transforms[1] - host.transforms[1]).max()
    print(f"  joint fit: the device optimiser's loss history is within {off:.2e} of the start loss of the host optimiser's; loss {dev.history[0]:.4e} -> "
          f"{dev.history[-1]:.4e}; the fitted transforms differ by up to {moved:.2e}")
    assert len(dev.history) == len(host.history) == rr.DYN_ITERS and all(np.isfinite(dev.history)) and off < 0.05
    assert np.array_equal(dev.transforms[0], c["bends"][0]) and not np.array_equal(dev.transforms[1], sr.identity_transforms(9).astype(np.float64))
    assert dev.transforms.dtype == np.float64 and dev.transforms.shape == host.transforms.shape


# ---- last: the bounds-checked build -----------------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
