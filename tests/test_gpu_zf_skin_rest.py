"""GPU: the adjoint of the deformation to the REST arrays and Adam under a skin (sas_scene_deform_backward_rest, sas_scene_adam_step_rest;
Rasterizer.deform_backward_rest, adam_step(rest=True), autograd.render_differentiable(rest_params=True), deform.fit_dynamic_scene,
SplatScene.fit_dynamic; DESIGN.md 3, "Deformation") against tests/tools/skin_rest_ref.py.  Every gradient case is held to the float64
reference within four times the float32 restatement's own error, per array (F32_ERR below; the measured ratios are printed); what the
contract makes exact -- pass-through, zeros, accumulation, the two paths, repeated runs, the stepped scene -- is compared bit for bit.
Scenes have 1, 257 and 300 Gaussians in 2 groups, as quaternions and as covariances; frames are 64x48."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import Rasterizer, SasError

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import scene_cases as sc_kit  # noqa: E402
import skin_grad_ref as sg  # noqa: E402
import skin_ref as sr  # noqa: E402
import skin_rest_child  # noqa: E402
import skin_rest_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = sg.RECOVER_W, sg.RECOVER_H
BG = (0.0, 0.0, 0.0)

# python tests/tools/skin_rest_ref.py
F32_ERR = {   # (case, form): per array, float32 restatement against float64, the largest of 4 shuffled entry orders
    ("n1_m9_k1", "quats"): dict(means=4.08e-08, quats=1.22e-07),
    ("n1_m9_k1", "covariances"): dict(means=6.06e-08, covariances=1.43e-07),
    ("n257_m9_k4", "quats"): dict(means=1.51e-07, quats=1.58e-07),
    ("n257_m9_k4", "covariances"): dict(means=2.01e-07, covariances=5.51e-07),
    ("n300_m256_k5", "quats"): dict(means=2.24e-07, quats=1.21e-07),
    ("n300_m256_k5", "covariances"): dict(means=1.84e-07, covariances=5.39e-07),
    ("n300_m257_k8", "quats"): dict(means=3.57e-07, quats=1.67e-07),
    ("n300_m257_k8", "covariances"): dict(means=2.19e-07, covariances=5.21e-07),
    ("n300_m9_far", "quats"): dict(means=1.09e-07, quats=9.84e-08),
    ("n300_m9_far", "covariances"): dict(means=9.79e-08, covariances=8.04e-07),
    ("n300_m9_group", "quats"): dict(means=1.62e-07, quats=1.00e-07),
    ("n300_m9_group", "covariances"): dict(means=1.26e-07, covariances=4.31e-07),
    ("n300_m70_dead", "quats"): dict(means=1.32e-07, quats=1.69e-07),
    ("n300_m70_dead", "covariances"): dict(means=1.67e-07, covariances=4.50e-07),
}
ALL = [(name, form) for name in rr.CASES for form in rr.FORMS]


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _held(got, ref, f32, what):
    """The four-times rule per array; prints the ratios."""
    e = rr.errs(got, ref)
    print(f"  {what}: " + ", ".join(f"{k} device {v:.3e} = {v / f32[k]:.2f} x float32 restatement" if f32[k] > 0 else f"{k} device {v:.3e}, restatement exact"
                                   for k, v in e.items()))
    assert set(got) == set(ref)
    for k, v in e.items():
        assert v <= 4.0 * f32[k], (what, k, v, f32[k])


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


# ---- every case against the float64 reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", ALL)
def test_every_case_is_the_reference(rasterizer, name, form):
    r = rasterizer
    c = rr.case(name, form)
    idx, w = _bind(r, c)
    r.deform(c["transforms"])
    g = _grads(r, c)
    res = r.deform_backward_rest(g)
    assert set(res) == {"means", form}
    for k, t in res.items():
        assert t.device == r.device and t.dtype == torch.float32 and tuple(t.shape) == tuple(g[k].shape)
    got = _np(res)
    ref = rr.grad64(name, form) if w is c["weights"] else rr.rest_grad_ref(c["rest"], idx, w, c["transforms"], c["d_means"], c["d_orient"])
    _held(got, ref, F32_ERR[(name, form)], f"{name} {form}")
    # Gaussians without a live entry: the gradient passes through bit for bit; bound_only: zeros, and the others unchanged
    dead = ~rr.live_rows(idx, w, c["m"])
    if name in ("n300_m9_far", "n300_m9_group", "n300_m70_dead"):
        assert dead.any() and not dead.all()
    up = dict(means=c["d_means"], **{form: c["d_orient"]})
    only = _np(r.deform_backward_rest(g, bound_only=True))
    for k in got:
        assert _bits(got[k][dead], up[k][dead]) and (only[k][dead] == 0.0).all() and _bits(only[k][~dead], got[k][~dead]), k
        assert np.isfinite(got[k]).all()
    # no atomics: a second run gives the same bits
    again = _np(r.deform_backward_rest(g))
    assert all(_bits(again[k], got[k]) for k in got)


@pytest.mark.parametrize("form", rr.FORMS)
def test_zero_accumulation_single_arrays_and_identity(rasterizer, form):
    r = rasterizer
    name = "n300_m70_dead"
    c = rr.case(name, form)
    _bind(r, c)
    r.deform(c["transforms"])
    g = _grads(r, c)
    one = _np(r.deform_backward_rest(g))
    # an all-zero gradient adds nothing to what out holds
    rng = np.random.default_rng(12)
    held = {k: torch.from_numpy(rng.normal(size=tuple(v.shape)).astype(np.float32)).to(r.device) for k, v in g.items()}
    before = _np(held)
    res = r.deform_backward_rest({k: torch.zeros_like(v) for k, v in g.items()}, out=held)
    assert all(res[k] is held[k] for k in held) and all(_bits(before[k], held[k].cpu().numpy()) for k in held)
    # two calls into one out are the float32 sum of two single calls
    acc = r.deform_backward_rest(g)
    acc = r.deform_backward_rest(g, out=acc)
    for k in one:
        assert _bits(acc[k].cpu().numpy(), one[k] + one[k]), k
    # the means alone and the orientation alone: each output depends on its own input, so the same bits as together -- and the reference's
    m_only, o_only = _np(r.deform_backward_rest(_grads(r, c, orient=False))), _np(r.deform_backward_rest(_grads(r, c, means=False)))
    assert set(m_only) == {"means"} and set(o_only) == {form}
    assert _bits(m_only["means"], one["means"]) and _bits(o_only[form], one[form])
    f32 = F32_ERR[(name, form)]
    _held(m_only, rr.grad64(name, form, True, False), f32, f"means alone {form}")
    _held(o_only, rr.grad64(name, form, False, True), f32, f"orientation alone {form}")
    # identity transforms return the incoming gradient, within the rule
    I = sr.identity_transforms(c["m"])
    r.deform(I)
    up = dict(means=c["d_means"].astype(np.float64), **{form: c["d_orient"].astype(np.float64)})
    ref = rr.rest_grad_ref(c["rest"], c["indices"], c["weights"], I, c["d_means"], c["d_orient"])
    for k in up:
        assert np.abs(ref[k] - up[k]).max() <= 1e-14 * np.abs(up[k]).max()   # (the reference returns it too)
    _held(_np(r.deform_backward_rest(g)), up, rr.f32_err_of(c["rest"], c["indices"], c["weights"], I, c["d_means"], c["d_orient"]), f"identity {form}")


# ---- the paths ------------------------------------------------------------------------------------------------------------------------------
def test_lds_and_global_paths_give_the_same_bits(rasterizer, tmp_path):
    """SAS_SKIN_LDS=0 (every lane reads its node records from global memory) in a fresh child process: the same bits as this process' default,
    in every case."""
    out = tmp_path / "skin_rest_child.npz"
    env = dict(os.environ, SAS_SKIN_LDS="0")
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "tools" / "skin_rest_child.py"), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "skin rest child ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
    assert "SAS_SKIN_LDS" not in os.environ   # (this process runs the default budget)
    with np.load(out) as z:
        for name, form in skin_rest_child.CASES:
            mine = _np(skin_rest_child.rest_grad(rasterizer, rr.case(name, form)))
            for k, v in mine.items():
                assert _bits(z[f"{name}_{form}_{k}"], v), (name, form, k)


# ---- the chain on real gradients ------------------------------------------------------------------------------------------------------------
def test_chain_on_real_gradients_and_autograd(rasterizer):
    """render_backward on the skinned 300-Gaussian sheet of the recovery case at 64x48, chained through the adjoint.  The reference chains the
    SAME device gradients through the float64 restatement, so only the new kernel is under test."""
    from sim_a_splat_amd.autograd import render_differentiable
    r = rasterizer
    c = sg.recovery_case()
    r.upload(**c["upload"])
    r.set_skin(c["indices"], c["weights"])
    T = c["truth"].astype(np.float32)
    r.deform(T)
    V, K = c["cams"][0][0], c["cams"][0][1]
    g_rgb = np.random.default_rng(33).normal(size=(H, W, 3)).astype(np.float32)
    r.render(V, K, W, H, BG)
    dev = r.render_backward(V, K, W, H, g_rgb=g_rgb, want=("means", "quats", "colors"))
    assert float(dev["means"].abs().max()) > 0.0
    got = _np(r.deform_backward_rest(dev))
    assert set(got) == {"means", "quats"}   # colours are untouched by a deformation and no part of it
    dm, dq = dev["means"].cpu().numpy(), dev["quats"].cpu().numpy()
    ref = rr.rest_grad_ref(c["rest"], c["indices"], c["weights"], T, dm, dq)
    f32 = rr.f32_err_of(c["rest"], c["indices"], c["weights"], T, dm, dq)
    _held(got, ref, f32, "render_backward chained")
    # render_differentiable(node_transforms=T, rest_params=True) routes the same way.  Its own render_backward sums with float atomics, so its
    # upstream gradients differ from `dev` in their last bits: the comparison is of the routing, at 1e-4 of the largest entry, not of rounding.
    P = {k: torch.from_numpy(np.ascontiguousarray(c["upload"][k])).to(r.device).requires_grad_(True) for k in ("means", "quats", "colors")}
    frame = render_differentiable(r, torch.from_numpy(np.asarray(V, np.float32)), K, W, H, params=P, background=BG,
                                  node_transforms=torch.from_numpy(T), rest_params=True)
    rgb = r.render(V, K, W, H, BG)["rgb"]
    assert bool((rgb < 1).all())   # (no pixel at the clamp: the upstream gradient of the raw accumulator is g_rgb itself)
    (frame["rgb"] * torch.from_numpy(g_rgb).to(r.device)).sum().backward()
    for k in ("means", "quats"):
        assert sr.rel_err(P[k].grad.cpu().numpy(), got[k]) < 1e-4, k
    assert sr.rel_err(P["colors"].grad.cpu().numpy().reshape(-1), dev["colors"].cpu().numpy().reshape(-1)) < 1e-4
    # ... and without rest_params the gradients are the deformed arrays', as before
    P2 = {"means": torch.from_numpy(np.ascontiguousarray(c["upload"]["means"])).to(r.device).requires_grad_(True)}
    frame = render_differentiable(r, torch.from_numpy(np.asarray(V, np.float32)), K, W, H, params=P2, background=BG, node_transforms=torch.from_numpy(T))
    (frame["rgb"] * torch.from_numpy(g_rgb).to(r.device)).sum().backward()
    assert sr.rel_err(P2["means"].grad.cpu().numpy(), dm) < 1e-4 and sr.rel_err(P2["means"].grad.cpu().numpy(), got["means"]) > 1e-3


# ---- state and refusals ---------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(rasterizer):
    r = rasterizer
    L = _capi.lib()
    c = rr.case("n257_m9_k4", "quats")
    n = c["n"]
    r.upload(**c["scene"])
    g = _grads(r, c)
    om, oq = torch.zeros((n, 3), device=r.device), torch.zeros((n, 4), device=r.device)
    oc = torch.zeros((n, 6), device=r.device)

    def call(dm=g["means"].data_ptr(), dq=g["quats"].data_ptr(), dc=None, o_m=om.data_ptr(), o_q=oq.data_ptr(), o_c=None, flags=0):
        return L.sas_scene_deform_backward_rest(r._ctx, dm, dq, dc, o_m, o_q, o_c, flags, None)

    err = lambda: L.sas_last_error(r._ctx)
    with pytest.raises(SasError, match="no skin"):
        r.deform_backward_rest(g)
    assert call() == -1 and b"no skin is bound" in err()
    r.set_skin(c["indices"], c["weights"])
    with pytest.raises(SasError, match="no deform"):
        r.deform_backward_rest(g)
    assert call() == -1 and b"no sas_scene_deform since" in err()
    r.deform(c["transforms"])
    assert call() == 0
    assert call(flags=2) == -1 and b"unknown flags" in err()
    assert call(dm=None, dq=None, o_m=None, o_q=None) == -1 and b"all NULL" in err()
    assert call(dc=g["means"].data_ptr(), o_c=oc.data_ptr()) == -1 and b"d_cov6 must be NULL" in err()
    assert call(o_m=None) == -1 and b"go together" in err()
    assert call(dm=None) == -1 and b"go together" in err()
    assert call(o_m=g["means"].data_ptr()) == -1 and b"overlaps" in err()          # in place
    assert call(o_q=g["means"].data_ptr()) == -1 and b"overlaps" in err()          # an output over another input
    assert call(o_q=om.data_ptr()) == -1 and b"overlaps" in err()                  # two outputs over each other
    assert call() == 0
    with pytest.raises(SasError, match="overlaps"):
        r.deform_backward_rest(g, out=g)
    cov = torch.zeros((n, 6), device=r.device)
    with pytest.raises(ValueError, match="uploaded as quats"):
        r.deform_backward_rest({"means": g["means"], "covariances": cov})
    for bad in ({"means": g["means"][:-1].contiguous()}, {"means": g["means"].double()}, {"means": g["means"].cpu()}, {"quats": g["quats"].half()}):
        with pytest.raises(ValueError, match="contiguous float32"):
            r.deform_backward_rest(bad)
    with pytest.raises(ValueError, match="contiguous float32"):
        r.deform_backward_rest(g, out={"means": torch.zeros((n, 4), device=r.device)})
    with pytest.raises(ValueError, match="neither means nor"):
        r.deform_backward_rest({"opacities": torch.zeros(n, device=r.device)})
    with pytest.raises(ValueError, match="dict"):
        r.deform_backward_rest(g["means"])
    # a rebind and a clear reset the state; an upload drops the skin
    r.set_skin(c["indices"], c["weights"])
    assert call() == -1
    r.deform(c["transforms"])
    r.clear_skin()
    assert call() == -1 and b"no skin is bound" in err()
    # before an upload: no scene
    r2 = Rasterizer(0)
    try:
        assert L.sas_scene_deform_backward_rest(r2._ctx, g["means"].data_ptr(), None, None, om.data_ptr(), None, None, 0, None) == -3   # SAS_ERR_NO_SCENE
    finally:
        r2.close()


# ---- Adam under a skin ----------------------------------------------------------------------------------------------------------------------
LRS = dict(means=1.6e-3, opacities=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4, quats=1e-3, scales=5e-3)


def _draw(shapes, seed, zero_rows=None):
    rng = np.random.default_rng(seed)
    g = {k: (10.0 ** rng.uniform(-4.0, 0.0, s) * rng.choice([-1.0, 1.0], s)).astype(np.float32) for k, s in shapes.items()}
    if zero_rows is not None:
        for v in g.values():
            v[zero_rows] = 0.0
    return g


def _same_scene(a, b):
    assert set(a) == set(b)
    for k in a:
        assert _bits(a[k].cpu().numpy(), b[k].cpu().numpy()), k


@pytest.mark.parametrize("form", rr.FORMS)
def test_adam_under_a_skin_is_adam_then_skin(rasterizer, form):
    """Context A steps the rest scene under its skin; context B never skins while stepping: it steps, binds the same entries, deforms, is
    read, and clears.  The scenes agree bit for bit after every step, after clear_skin, and after a fourth, unskinned step (the moments)."""
    A = rasterizer
    c = rr.case("n300_m70_dead", form)
    T = c["transforms"]
    V, K = sc_kit.ring(W, H, f=55.0, yaw=25.0, elev=0.3)[:2]
    B = Rasterizer(0)
    try:
        A.upload(**c["scene"])
        B.upload(**c["scene"])
        shapes = {k: v for k, v in A._scene_shapes().items() if k != "covariances"}
        hidden = np.arange(c["n"]) % 5 == 2
        steps = [_draw(shapes, 70), _draw(shapes, 71, hidden), _draw(shapes, 72), _draw(shapes, 73)]
        on = lambda r, g: {k: torch.from_numpy(v).to(r.device) for k, v in g.items()}
        A.set_skin(c["indices"], c["weights"])
        # refusals: rest=False under a skin changes nothing; rest=True without one
        before = A.read_scene()
        with pytest.raises(SasError, match="scene is skinned"):
            A.adam_step(on(A, steps[0]), LRS, 1)
        _same_scene(A.read_scene(), before)
        with pytest.raises(SasError, match="no skin is bound"):
            B.adam_step(on(B, steps[0]), LRS, 1, rest=True)
        _same_scene(B.read_scene(), before)
        for t in (1, 2, 3):
            vis = t == 2
            if t == 2:
                held = {k: v.cpu().numpy()[hidden] for k, v in A.read_scene().items()}
            A.adam_step(on(A, steps[t - 1]), LRS, t, visible_only=vis, rest=True)
            B.adam_step(on(B, steps[t - 1]), LRS, t, visible_only=vis)
            if t == 1:   # before any deform the live planes are the stepped rest planes
                _same_scene(A.read_scene(), B.read_scene())
                A.deform(T)
            B.set_skin(c["indices"], c["weights"])
            B.deform(T)
            a, b = A.read_scene(), B.read_scene()
            B.clear_skin()
            _same_scene(a, b)
            if t == 2:   # visible_only: Gaussians whose gradient is zero everywhere keep their bits (their moments: the steps after)
                for k, v in held.items():
                    assert _bits(a[k].cpu().numpy()[hidden], v), k
        assert not _bits(a["means"].cpu().numpy(), c["scene"]["means"])
        # the frame after the step is the frame of a fresh context that uploads A's read_scene()
        frame = sc_kit.to_numpy(A.render(V, K, W, H, BG))
        C = Rasterizer(0)
        try:
            C.upload(**{k: v for k, v in a.items()}, sh_degree=-1, group_id=c["scene"]["group_id"], n_groups=sr.GROUPS)
            other = sc_kit.to_numpy(C.render(V, K, W, H, BG))
        finally:
            C.close()
        assert frame["alpha"].max() > 0.5
        sc_kit.same(frame, other, keys=("rgb", "alpha", "depth"))
        # clear_skin returns the STEPPED rest scene, and the moments survive it
        A.clear_skin()
        _same_scene(A.read_scene(), B.read_scene())
        A.adam_step(on(A, steps[3]), LRS, 4)
        B.adam_step(on(B, steps[3]), LRS, 4)
        _same_scene(A.read_scene(), B.read_scene())
    finally:
        B.close()


# ---- recovery: the rest scene from pictures of two bends ------------------------------------------------------------------------------------
def _fit_on_device(r, joint):
    from sim_a_splat_amd import deform
    c = rr.dynamic_case()
    r.upload(**c["start"])
    r.set_skin(c["indices"], c["weights"])
    res = deform.fit_dynamic_scene(r, c["frames"], c["nodes"], **rr.dynamic_settings(joint))
    bent = r.read_scene()["means"].cpu().numpy()
    r.clear_skin()
    rest = r.read_scene()
    return c, res, bent, rest


def test_fit_dynamic_scene_recovers_the_rest_means(rasterizer):
    """The CPU test's recovery case with the same settings, on the device: the run ends where the float64 reference run ends, within 5 % of
    the start error, and below the fraction of the start the kit records (DYN_REF_END 0.8572, DYN_FRACTION 0.9: no case of this size comes
    near the truth, skin_rest_ref.py says why)."""
    r = rasterizer
    c, res, bent, rest = _fit_on_device(r, False)
    e0, e1 = rr.rest_error(c, c["start"]["means"]), rr.rest_error(c, rest["means"].cpu().numpy())
    print(f"  dynamic fit on the device: rest means' mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start (the reference run: {rr.DYN_REF_END}); "
          f"loss {res.history[0]:.4e} -> {res.history[-1]:.4e}")
    assert abs(e1 / e0 - rr.DYN_REF_END) < 0.05
    assert e1 < rr.DYN_FRACTION * e0
    assert res.steps == rr.DYN_ITERS and np.array_equal(res.transforms, c["bends"])
    # r was left deformed at the last time step
    want = sr.deform_ref(dict(means=rest["means"].cpu().numpy(), quats=rest["quats"].cpu().numpy()), c["indices"], c["weights"], c["bends"][1].astype(np.float32))["means"]
    assert np.abs(bent - want).max() < 1e-5
    with pytest.raises(ValueError, match="no skin is bound"):
        from sim_a_splat_amd import deform
        deform.fit_dynamic_scene(r, c["frames"], c["nodes"], iters=1)


def test_fit_dynamic_scene_joint(rasterizer):
    """fit_transforms=True: step 0 the anchor, the second bend's transforms from the identity; held to its own reference run (DYN_JOINT_REF_END
    0.8629) the same way."""
    r = rasterizer
    c, res, bent, rest = _fit_on_device(r, True)
    e0, e1 = rr.rest_error(c, c["start"]["means"]), rr.rest_error(c, rest["means"].cpu().numpy())
    print(f"  joint fit on the device: rest means' mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start (the reference run: {rr.DYN_JOINT_REF_END}); "
          f"loss {res.history[0]:.4e} -> {res.history[-1]:.4e}")
    assert abs(e1 / e0 - rr.DYN_JOINT_REF_END) < 0.05
    assert e1 < rr.DYN_JOINT_FRACTION * e0
    assert np.array_equal(res.transforms[0], c["bends"][0]) and not np.array_equal(res.transforms[1], sr.identity_transforms(9).astype(np.float64))
    # no case of this size finds the second bend (skin_rest_ref.DYN_JOINT_HISTORY says so with the numbers): the loss history follows the reference's
    off = np.abs(np.asarray(res.history) - rr.DYN_JOINT_HISTORY).max() / rr.DYN_JOINT_HISTORY[0]
    print(f"  the loss history is within {off:.2e} of the start loss of the reference's")
    assert len(res.history) == rr.DYN_ITERS and off < 0.05


def _look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(wxyz, position) of a camera at ``position`` looking at ``target``: camera-to-world, OpenCV axes (x right, y down, z forward)."""
    from sim_a_splat_amd.poses import matrix_to_quat_wxyz
    p = np.asarray(position, np.float64)
    z = np.asarray(target, np.float64) - p
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return tuple(matrix_to_quat_wxyz(np.stack([x, np.cross(z, x), z], axis=1))), tuple(p)


def test_door_b_fits_its_deformable_group_and_leaves_the_static_one():
    """SplatScene.fit_dynamic on a two-group scene whose second group is the kit's sheet, perturbed: frames of the true sheet in two bends
    (get_renders after deform), then the fit.  The static group's arrays are bit-identical before and after; the sheet's means move towards
    the truth and the loss falls."""
    from sim_a_splat_amd.scene import SplatScene
    c = rr.dynamic_case()
    rng = np.random.default_rng(96)
    n0 = 150
    static = ((rng.normal(0.0, 0.08, (n0, 3)) + (0.0, 0.62, 0.0)).astype(np.float32), np.tile(np.eye(3, dtype=np.float32) * 2e-3, (n0, 1, 1)),
              rng.uniform(0, 1, (n0, 3)).astype(np.float32), rng.uniform(0.5, 0.9, n0).astype(np.float32))
    M = sr.quat_to_matrix(c["rest"]["quats"]) * c["scales"].astype(np.float64)[:, None, :]
    cov = (M @ np.swapaxes(M, 1, 2)).astype(np.float32)
    cams = [_look_at((0.0, -0.5, 1.4)), _look_at((1.1, 0.3, 1.0))]
    rows = slice(n0, n0 + sg.RECOVER_N)
    bends = c["bends"].astype(np.float32)

    def build(means, colors, bind=True):
        scene = SplatScene(0, background=(0.0, 0.0, 0.0))
        scene.add_gaussian_splats("static", *static)
        cloth = scene.add_gaussian_splats("cloth", means, cov, colors, c["op"], position=(0.0, -0.05, 0.0))
        if bind:
            scene.bind_deformable(cloth, c["nodes"], k=4)
        return scene

    true = build(c["upload"]["means"], c["upload"]["colors"])
    try:
        frames = []
        for T in bends:
            true.deform(T)
            frames.append(dict(images=true.get_renders(H, W, cams, fov=0.9).copy(), cam_poses=cams))
    finally:
        true.close()
    unbound = build(c["start"]["means"], c["start"]["colors"], bind=False)
    try:
        with pytest.raises(RuntimeError, match="bind_deformable first"):
            unbound.fit_dynamic(frames, H, W, fov=0.9, transforms=bends, iters=1)
    finally:
        unbound.close()
    scene = build(c["start"]["means"], c["start"]["colors"])
    try:
        scene.deform(sr.identity_transforms(9))
        r = scene._raster
        before = {k: v.cpu().numpy() for k, v in r.read_scene().items()}
        res = scene.fit_dynamic(frames, H, W, fov=0.9, transforms=bends, iters=rr.DYN_ITERS, lrs=rr.DYN_LRS, extent=1.0)
        r.clear_skin()
        after = {k: v.cpu().numpy() for k, v in r.read_scene().items()}
        for k in before:
            assert _bits(after[k][:n0], before[k][:n0]), k   # the static group: not a bit moved
        truth = c["upload"]["means"].astype(np.float64)
        e0 = np.linalg.norm(before["means"][rows] - truth, axis=1).mean()
        e1 = np.linalg.norm(after["means"][rows] - truth, axis=1).mean()
        print(f"  Door B: rest means' mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start; loss {res.history[0]:.4e} -> {res.history[-1]:.4e}")
        assert e1 < e0 and res.history[-1] < 0.5 * res.history[0]
        assert not _bits(after["colors"][rows], before["colors"][rows])
        # the fitted arrays replaced the group's own: a later upload keeps them
        assert _bits(scene._groups[1]["centers"], after["means"][rows]) and _bits(scene._groups[0]["centers"], before["means"][:n0])
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
