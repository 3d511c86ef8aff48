"""CPU: the group-pose gradient's yardstick (tests/tools/group_pose_ref.py), its cases (tests/tools/group_pose_cases.py), the twist chain and
the pose optimiser of sim_a_splat_amd.register on the float64 reference, and the C ABI's declaration of sas_render_backward_poses.  The GPU
side is tests/test_gpu_x_group_pose_grad.py."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import grad_cases as gc  # noqa: E402
import grad_ref  # noqa: E402
import group_pose_cases as gpc  # noqa: E402
import group_pose_ref as gpr  # noqa: E402

from sim_a_splat_amd import _capi  # noqa: E402
from sim_a_splat_amd import register  # noqa: E402

EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("name", gpc.NAMES)
def test_case_conditions(name):
    """At most MAX_MASKED of the pixels are masked, no Gaussian has a marginal projection decision -- from the reference alone."""
    sc, cam, _ = gpc.case(name)
    ref = gpc.reference(name)
    assert ref["near"].mean() <= gpc.MAX_MASKED, ref["near"].mean()
    assert ref["margin"].sum() == 0
    gid, n = np.asarray(sc["gid"]), len(sc["means"])
    if name.startswith("gp600") or name in ("gp_rare", "gp_behind"):
        assert 512 < n <= 768   # three workgroups of 256
    if name.startswith("gp600"):
        assert all(len(set(gid[w:w + 64].tolist())) == 5 for w in range(0, n, 64))   # every wave holds all five groups
        assert np.abs(ref["full"]["group_poses"]).reshape(5, -1).max(axis=1).min() > 1.0   # every group's row carries signal
    if name == "gp_rare":
        assert (gid == gpc.RARE_GROUP).sum() == gpc.RARE_COUNT
        assert np.abs(ref["full"]["group_poses"][gpc.RARE_GROUP]).max() > 0
    if name == "gp_behind":
        mine = gid == gpc.BEHIND_GROUP
        assert mine.sum() > 100 and not ref["valid"][mine].any() and ref["valid"][~mine].all()
        assert np.all(ref["full"]["group_poses"][gpc.BEHIND_GROUP] == 0)
        assert np.all(ref["full"]["means"][mine] == 0)
    if name == "gp_clamp":
        import torch
        n, extras = len(gid), [len(gid) + i for i in gc.CLAMP.values()]
        assert np.all(gid[extras] == gc.CLAMP_GROUP) and ref["valid"][extras].all()
        G = np.asarray(sc["Rt"], np.float64).reshape(-1, 3, 4)[gc.CLAMP_GROUP]
        assert not np.allclose(G[:, :3], np.eye(3), atol=1e-2) and np.abs(G[:, 3]).max() > 1e-2   # a pose that is not the identity
        with torch.no_grad():
            I = gpr.forward(sc, cam)[3]
        (xp, xn, yp, yn), u, m = I["limits"], I["ratios"].numpy(), 1 + grad_ref.MARGIN
        k = {key: n + i for key, i in gc.CLAMP.items()}   # placed through the pose: beyond the limits AFTER posing
        assert u[k["x_pos"], 0] > xp * m and u[k["x_neg"], 0] < -xn * m and u[k["y_pos"], 1] > yp * m and u[k["y_neg"], 1] < -yn * m
        assert u[k["corner"], 0] > xp * m and u[k["corner"], 1] < -yn * m


def test_clamp_case_is_sensitive_in_its_group_pose():
    """grad_ref.project's straight-through mutant (the clamp's gradient passed to x and y, the same forward) moves dL/dG of the group
    that holds the clamped Gaussians of "gp_clamp" by more than 100 times the GPU bound, four times the float32 reference's figure: the
    clamp's z route flows into that group's pose, and the case would show an implementation that lost it."""
    ref, mut = gpc.reference("gp_clamp")["full"]["group_poses"], gpc.mutant_reference("gp_clamp")["group_poses"]
    f32 = gpc.float32_errors("gp_clamp")["group_poses"]
    assert f32 <= 1e-5
    d = np.abs(mut[gc.CLAMP_GROUP] - ref[gc.CLAMP_GROUP]).max() / np.abs(ref).max()   # in the measure of the GPU test: over the whole array
    print(f"GROUP POSE straight-through mutant on gp_clamp: group {gc.CLAMP_GROUP} off by {d:.3e}, GPU bound {4.0 * f32:.3e}")
    assert d > 100 * 4.0 * f32


def test_posing_in_front_changes_nothing_else():
    """The helper poses the scene itself and calls grad_ref.project without groups: the other gradients are grad_ref.gradients' own, and
    the quaternion and cov6 forms of one scene (same upstream gradients) agree on dL/dG."""
    sc, cam, g = gpc.case("gp600")
    a, b = gpc.reference("gp600")["full"], grad_ref.gradients(sc, cam, *g)["full"]
    for k in b:
        assert grad_ref.rel_err(a[k], b[k]) <= 1e-12, k
    c = gpc.reference("gp600_cov6")["full"]
    assert grad_ref.rel_err(c["group_poses"], a["group_poses"]) <= 1e-6   # cov6 is stored as float32: 6e-8 per entry
    assert grad_ref.rel_err(c["viewmat"], a["viewmat"]) <= 1e-6


ENTRIES = ((0, 0), (1, 2), (2, 1), (0, 3), (2, 3), (1, 3))   # rotation and translation entries of a pose [3,4]


@pytest.mark.parametrize("name", ["gp600", "gp600_cov6", "gp_sh2", "gp_rare", "gp_clamp"])
def test_reference_against_central_differences(name):
    """dL/dG of the yardstick against central differences of the float64 loss with the mask held fixed.  The step is fixed; the
    tolerance per entry is derived here: the central difference at h errs by h^2 f'''/6, which the difference at 2h shows fourfold, so
    |D(2h) - D(h)| / 3 estimates it (Richardson); twice that, plus the rounding of the loss itself, 8 eps |L| / h."""
    sc, cam, g = gpc.case(name)
    ref = gpc.reference(name)
    keep = ~ref["near"]
    G0 = np.asarray(sc["Rt"], np.float64).reshape(-1, 3, 4)
    h = 1e-5
    L0 = abs(gpr.loss_at(sc, cam, G0, g, keep))
    assert abs(L0 - abs(ref["loss"])) <= 1e-9 * max(1.0, L0)

    def diff(grp, rc, step):
        Gp, Gm = G0.copy(), G0.copy()
        Gp[grp][rc] += step
        Gm[grp][rc] -= step
        return (gpr.loss_at(sc, cam, Gp, g, keep) - gpr.loss_at(sc, cam, Gm, g, keep)) / (2.0 * step)

    # every group of the two cases that are cheap or new in kind; of the same scene's other forms the groups that differ
    groups = {"gp600": range(G0.shape[0]), "gp_sh2": range(G0.shape[0]), "gp600_cov6": (0, 3), "gp_rare": (gpc.RARE_GROUP,), "gp_clamp": (gc.CLAMP_GROUP,)}[name]
    for grp in groups:
        for rc in (ENTRIES[grp % 2::2] if name == "gp_sh2" else ENTRIES[grp % 3::3]):   # a few entries of each group: rotation and translation
            d1, d2 = diff(grp, rc, h), diff(grp, rc, 2.0 * h)
            tol = 2.0 * abs(d2 - d1) / 3.0 + 8.0 * EPS * max(1.0, L0) / h
            got = ref["full"]["group_poses"][grp][rc]
            print(f"GROUP POSE fd {name} group {grp} entry {rc}: autograd {got:.9e} differences {d1:.9e} tolerance {tol:.2e}")
            assert abs(got - d1) <= tol, (grp, rc, got, d1, tol)


def test_twist_gradient_on_a_group_pose():
    """register.twist_gradient(d_G, G) is the chain for G(xi) = se3_exp(xi) G: against central differences along se3_exp, tolerance as above."""
    name, grp = "gp_sh2", 1
    sc, cam, g = gpc.case(name)
    ref = gpc.reference(name)
    keep = ~ref["near"]
    G0 = np.asarray(sc["Rt"], np.float64).reshape(-1, 3, 4)
    G4 = np.eye(4)
    G4[:3] = G0[grp]
    tw = register.twist_gradient(ref["full"]["group_poses"][grp], G4)
    L0, h = abs(ref["loss"]), 1e-5

    def along(k, step):
        xi = np.zeros(6)
        out = []
        for s in (step, -step):
            xi[k] = s
            G = G0.copy()
            G[grp] = (register.se3_exp(xi) @ G4)[:3]
            out.append(gpr.loss_at(sc, cam, G, g, keep))
        return (out[0] - out[1]) / (2.0 * step)

    for k in range(6):
        d1, d2 = along(k, h), along(k, 2.0 * h)
        tol = 2.0 * abs(d2 - d1) / 3.0 + 8.0 * EPS * max(1.0, L0) / h
        assert abs(tw[k] - d1) <= tol, (k, tw[k], d1, tol)


def test_symbol_is_declared_and_listed():
    header = (ROOT / "include" / "sim_a_splat_amd.h").read_text()
    assert re.search(r"\bint\s+sas_render_backward_poses\s*\(", header)
    assert re.search(r"#define\s+SAS_MAX_POSE_GRAD_GROUPS\s+32\b", header) and _capi.SAS_MAX_POSE_GRAD_GROUPS == 32
    assert "sas_render_backward_poses" in _capi.EXPORTS
    from sim_a_splat_amd import build
    build.build()
    L = _capi.lib()
    assert len(L.sas_render_backward_poses.argtypes) == 20
    assert len(L.sas_render_backward.argtypes) == 17   # the plain call keeps its signature


class _Poses:
    """What refine_group_poses asks of a rasterizer when ``loss_and_grad`` stands in for the renderer."""
    def __init__(self, Rt):
        self.Rt = np.asarray(Rt, np.float32).reshape(-1, 12).copy()

    def get_group_poses(self):
        return self.Rt.copy()

    def set_group_poses(self, Rt):
        self.Rt = np.asarray(Rt, np.float32).reshape(-1, 12).copy()


def recover_on_reference():
    """The recovery case run on the float64 reference (shared with the GPU test): (result, start and end errors)."""
    sc, cams, true, start, pivot = gpc.recovery_case()
    images = np.stack([gpr.frame(sc, cam, true) for cam in cams])
    holder = _Poses(start)
    W, H = cams[0][2], cams[0][3]
    res = register.refine_group_poses(holder, images, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), W, H,
                                      [gpc.RECOVER_GROUP], iters=gpc.RECOVER_ITERS, pivots=pivot, factors=(1,),
                                      loss_and_grad=gpr.mse_loss_and_grad(sc, [gpc.RECOVER_GROUP]))
    e0 = gpc.pose_error(start[gpc.RECOVER_GROUP], true[gpc.RECOVER_GROUP], pivot)
    e1 = gpc.pose_error(res.poses[gpc.RECOVER_GROUP], true[gpc.RECOVER_GROUP], pivot)
    return res, holder, e0, e1


def test_refine_group_poses_recovers_on_the_reference():
    res, holder, (a0, d0), (a1, d1) = recover_on_reference()
    sc, cams, true, start, pivot = gpc.recovery_case()
    print(f"GROUP POSE recovery on the reference: {a0:.3f} deg, {d0:.4f} -> {a1:.4f} deg, {d1:.5f}; loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    assert 3.4 < a0 < 3.6 and 0.029 < d0 < 0.033
    assert a1 < 0.1 * a0 and d1 < 0.1 * d0
    assert abs(a1 - gpc.RECOVER_REF_END[0]) < 0.002 * a0 and abs(d1 - gpc.RECOVER_REF_END[1]) < 0.002 * d0   # the GPU test's comparison point
    assert res.poses.shape == true.shape and res.poses.dtype == np.float64
    others = [g for g in range(len(true)) if g != gpc.RECOVER_GROUP]
    assert np.array_equal(res.poses[others], start[others])   # unselected rows as they were
    np.testing.assert_allclose(holder.Rt.reshape(-1, 3, 4), res.poses, atol=1e-6)   # the poses are left at the result
    assert len(res.history) == gpc.RECOVER_ITERS + 1 and res.loss < 1e-2 * res.history[0][1]
