"""CPU: the yardstick of the deformation's adjoint (tests/tools/skin_grad_ref.py) and the host side of the fit (deform.rigidity,
deform.fit_node_transforms; DESIGN.md 3, "Deformation").  The restatement's float64 gradient is held to central differences of
skin_ref.deform_ref; every case of the kit keeps its decisions 1e-4 from their thresholds; rigidity's analytic gradient is held to torch
autograd; fit_node_transforms runs on the float64 reference (grad_ref's renderer chained with the restatement) and recovers the bend of the
kit's sheet.  No GPU."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import skin_grad_ref as sg  # noqa: E402
import skin_ref as sr  # noqa: E402
from sim_a_splat_amd import _capi, deform, register  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("form", sg.FORMS)
def test_restatement_against_central_differences(form):
    """All 60 entries of m5_k3.  deform_ref takes float32 transforms, so the differences are taken of deform_torch in float64 (the same
    expressions: the first assertion holds the two together), with the decisions' margins keeping every step on one branch."""
    c = sg.case("m5_k3", form)
    key = sg.orient_key(c["rest"])
    T0 = c["transforms"].astype(np.float64)
    ref = sr.deform_ref(c["rest"], c["indices"], c["weights"], c["transforms"])
    mine = sg.deform_torch(c["rest"], c["indices"], c["weights"], torch.from_numpy(T0))
    for k in ("means", key):
        np.testing.assert_allclose(mine[k].numpy(), ref[k], rtol=0, atol=1e-13)
    dm, do = c["d_means"].astype(np.float64), c["d_orient"].astype(np.float64)

    def loss(T):
        with torch.no_grad():
            o = sg.deform_torch(c["rest"], c["indices"], c["weights"], torch.from_numpy(T))
        return float((o["means"].numpy() * dm).sum() + (o[key].numpy() * do).sum())

    got = sg.grad64("m5_k3", form)
    L0, h = abs(loss(T0)), 1e-5
    for a in range(5):
        for i in range(3):
            for j in range(4):
                def diff(step):
                    Tp, Tm = T0.copy(), T0.copy()
                    Tp[a, i, j] += step
                    Tm[a, i, j] -= step
                    return (loss(Tp) - loss(Tm)) / (2.0 * step)
                d1, d2 = diff(h), diff(2.0 * h)
                tol = 2.0 * abs(d2 - d1) / 3.0 + 8.0 * EPS * max(1.0, L0) / h
                assert abs(got[a, i, j] - d1) <= tol, (form, a, i, j, got[a, i, j], d1, tol)


@pytest.mark.parametrize("name", tuple(sg.CASES))
def test_cases_keep_their_margins(name):
    c = sg.case(name)
    mg = sg.margins(c["indices"], c["weights"], c["transforms"])
    print(f"  {name}: branch {mg['branch']:.1e}, |dot| {mg['dot']:.1e}, n2 {mg['n2']:.1e}, branches {mg['branches']}, flips {mg['flips']}, unnamed {mg['unnamed']}")
    assert mg["branch"] >= sg.MARGIN and mg["dot"] >= sg.MARGIN and mg["n2"] >= sg.MARGIN
    if "angle" in sg.CASES[name][2]:
        assert all(b > 0 for b in mg["branches"]) and mg["flips"] > 0   # every branch of the conversion, and sign flips
    if name in ("m257_k8", "m2048_k4", "m2049_k4", "m70_far"):
        assert mg["unnamed"] > 0
    # float32 decides alike: the float32 restatement's gradient is the float64's up to rounding, not up to a branch
    e = sg.split_err(sg.node_grad_ref(c["rest"], c["indices"], c["weights"], c["transforms"], c["d_means"], c["d_orient"], torch.float32), sg.grad64(name))
    assert max(e) < 1e-5, e


def test_kit_sizes_follow_the_library():
    assert sg.GRAD_LDS_NODES * 64 == _capi.SAS_SKIN_GRAD_LDS_BYTES
    text = (ROOT / "sim_a_splat_amd" / "csrc" / "sas_internal.h").read_text()
    assert re.search(r"#define\s+SAS_SKIN_GRAD_LDS_BYTES\s+%d\b" % _capi.SAS_SKIN_GRAD_LDS_BYTES, text)
    assert "sas_scene_deform_backward" in _capi.EXPORTS
    assert re.search(r"\bint\s+sas_scene_deform_backward\s*\(", (ROOT / "include" / "sim_a_splat_amd.h").read_text())


def test_rigidity_gradient_is_autograds():
    nodes = sr.nodes("m70").astype(np.float64)
    T = sr.transforms(nodes, angle=1.2).astype(np.float64)
    val, d = deform.rigidity(nodes, T)
    nb = deform._neighbour_table(nodes, 6)
    Tt = torch.from_numpy(T).requires_grad_(True)
    g = torch.from_numpy(nodes)
    gj = g[torch.from_numpy(nb)]
    at = lambda Ti: torch.einsum("mkab,mkb->mka", Ti[:, :, :, :3], gj) + Ti[:, :, :, 3]
    mine, theirs = at(Tt[:, None].expand(-1, nb.shape[1], -1, -1)), at(Tt[torch.from_numpy(nb)])
    ref = ((mine - theirs) ** 2).sum() / (nodes.shape[0] * nb.shape[1])
    ref.backward()
    assert abs(val - float(ref)) <= 1e-12 * abs(float(ref)) and val > 0
    np.testing.assert_allclose(d, Tt.grad.numpy(), rtol=0, atol=1e-12 * np.abs(Tt.grad.numpy()).max())
    # neighbours as transforms_from_positions takes them; one rigid motion of all nodes costs nothing; degenerate sizes
    assert nb.shape == (70, 6) and all(i not in nb[i] for i in range(70))
    d2 = ((nodes[:, None] - nodes[None]) ** 2).sum(axis=2)
    assert np.array_equal(nb[0], [j for j in np.argsort(d2[0], kind="stable") if j != 0][:6])
    one = np.tile(sr.transforms(nodes[:1], angle=1.0).astype(np.float64), (70, 1, 1))
    v1, d1 = deform.rigidity(nodes, one)
    assert v1 < 1e-12 and np.abs(d1).max() < 1e-6
    assert deform.rigidity(nodes[:1], T[:1]) == (0.0, pytest.approx(np.zeros((1, 3, 4))))
    assert deform.rigidity(nodes[:3], T[:3], neighbours=6)[0] > 0
    with pytest.raises(ValueError, match="70 nodes but 3 transforms"):
        deform.rigidity(nodes, T[:3])


def test_batched_twists_are_registers():
    rng = np.random.default_rng(3)
    xi = rng.normal(0.0, 0.3, (7, 6))
    xi[0] = 0.0
    xi[1, :3] = 1e-10
    E = deform.se3_exp_batch(xi)
    for i in range(7):
        np.testing.assert_allclose(E[i], register.se3_exp(xi[i]), rtol=0, atol=1e-14)
    T = sr.transforms(sr.nodes("m5"), angle=2.0).astype(np.float64)
    d = rng.normal(size=(5, 3, 4))
    piv = rng.normal(size=(5, 3))
    tw, twp = deform.twist_gradient_batch(d, T), deform.twist_gradient_batch(d, T, piv)
    for i in range(5):
        T4 = np.eye(4)
        T4[:3] = T[i]
        ref = register.twist_gradient(d[i], T4)
        np.testing.assert_allclose(tw[i], ref, rtol=0, atol=1e-13)
        ref[:3] += np.cross(ref[3:], piv[i])
        np.testing.assert_allclose(twp[i], ref, rtol=0, atol=1e-13)


def test_fit_node_transforms_recovers_the_bend_on_the_reference():
    res, e0, e1 = sg.recover_on_reference()
    print(f"  recovery on the reference: mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start; loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    assert 0.02 < e0 < 0.03
    assert e1 < sg.RECOVER_FRACTION * e0
    assert abs(e1 / e0 - sg.RECOVER_REF_END) < 0.002   # the GPU test's comparison point
    assert res.transforms.shape == (9, 3, 4) and res.transforms.dtype == np.float64
    assert len(res.history) == sg.RECOVER_ITERS + 1 and [f for f, _ in res.history[:2]] == [2, 2] and res.history[-1][0] == 1
    assert res.loss < 0.05 * res.history[0][1]
    R = res.transforms[:, :, :3]
    assert np.abs(np.einsum("mki,mkj->mij", R, R) - np.eye(3)).max() < 1e-9   # the twists keep every node rigid
    assert deform.RIGIDITY_WEIGHT == sg.RECOVER_WEIGHT


def test_fit_node_transforms_refusals():
    c = sg.recovery_case()
    V, K = np.stack([cam[0] for cam in c["cams"]]), np.stack([cam[1] for cam in c["cams"]])
    fn = lambda *a: (0.0, np.zeros((9, 3, 4)))
    W, H = sg.RECOVER_W, sg.RECOVER_H
    with pytest.raises(ValueError, match="start must be"):
        deform.fit_node_transforms(None, c["images"], V, K, W, H, c["nodes"], iters=2, start=np.zeros((3, 3, 4)), loss_and_grad=fn)
    with pytest.raises(ValueError, match="rigidity_weight"):
        deform.fit_node_transforms(None, c["images"], V, K, W, H, c["nodes"], iters=2, rigidity_weight=-1.0, loss_and_grad=fn)
    with pytest.raises(ValueError, match="need nodes"):
        deform.fit_node_transforms(None, c["images"], V, np.concatenate([K, K[:1]]), W, H, c["nodes"], iters=2, loss_and_grad=fn)
    with pytest.raises(ValueError, match="no skin is bound"):
        deform.fit_node_transforms(object(), c["images"], V, K, W, H, c["nodes"], iters=2)
    # a gradient of zero moves nothing: the start comes back, and the history has one entry per evaluation
    start = sr.transforms(c["nodes"]).astype(np.float64)
    res = deform.fit_node_transforms(None, c["images"], V, K[:1], W, H, c["nodes"], iters=4, start=start, rigidity_weight=0.0, loss_and_grad=fn)
    assert np.array_equal(res.transforms, start) and len(res.history) == 5 and res.loss == 0.0
