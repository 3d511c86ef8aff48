"""CPU: the yardstick of the deformation's adjoint to the REST arrays (tests/tools/skin_rest_ref.py) and the host side of the fit across
time steps (deform.fit_dynamic_scene; DESIGN.md 3, "Deformation").  The restatement (skin_grad_ref.deform_torch) called with rest tensors
is held to itself called with rest arrays bit for bit; its float64 gradient is held to central differences; every case keeps its decisions 1e-4 from their
thresholds in every entry order of the yardstick; the header, the exports and the Python front end carry the two new entry points;
fit_dynamic_scene runs on the float64 reference and its rest means approach the truth.  No GPU."""
import inspect
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
import skin_rest_ref as rr  # noqa: E402
from sim_a_splat_amd import _capi, autograd, deform  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.scene import SplatScene  # noqa: E402

EPS = np.finfo(np.float64).eps
ALL = [(name, form) for name in rr.CASES for form in rr.FORMS]


@pytest.mark.parametrize("name,form", ALL)
def test_tensor_form_is_deform_torch_bit_for_bit(name, form):
    """The one restatement called with rest TENSORS (the form gradients flow through) against itself called with rest arrays."""
    c = rr.case(name, form)
    for dt in (torch.float64, torch.float32):
        theirs = sg.deform_torch(c["rest"], c["indices"], c["weights"], torch.from_numpy(c["transforms"]).to(dt), dt)
        mine = sg.deform_torch({k: torch.from_numpy(v) for k, v in c["rest"].items()}, c["indices"], c["weights"], torch.from_numpy(c["transforms"]), dt)
        assert set(mine) == set(theirs)
        for k in theirs:
            assert mine[k].dtype == dt and torch.equal(mine[k], theirs[k]), (name, form, dt, k)


@pytest.mark.parametrize("form", rr.FORMS)
def test_reference_against_central_differences(form):
    """Every rest entry of the first 12 Gaussians of the dead-entry case (among them rows without a live entry) and of the one-Gaussian case.
    The forward is linear in each rest array, so the differences are exact up to rounding."""
    for name, rows in (("n300_m70_dead", range(12)), ("n1_m9_k1", range(1))):
        c = rr.case(name, form)
        key = sg.orient_key(c["rest"])
        dm, do = c["d_means"].astype(np.float64), c["d_orient"].astype(np.float64)
        base = {k: v.astype(np.float64) for k, v in c["rest"].items()}

        def loss(rest):
            with torch.no_grad():
                o = sg.deform_torch({k: torch.from_numpy(v) for k, v in rest.items()}, c["indices"], c["weights"], torch.from_numpy(c["transforms"]))
            return float((o["means"].numpy() * dm).sum() + (o[key].numpy() * do).sum())

        got = rr.grad64(name, form)
        L0, h = abs(loss(base)), 1e-3
        live = rr.live_rows(c["indices"], c["weights"], c["m"])
        assert name == "n1_m9_k1" or not live[list(rows)].all()
        for k in ("means", key):
            for i in rows:
                for j in range(base[k].shape[1]):
                    p, m = {a: v.copy() for a, v in base.items()}, {a: v.copy() for a, v in base.items()}
                    p[k][i, j] += h
                    m[k][i, j] -= h
                    d = (loss(p) - loss(m)) / (2.0 * h)
                    assert abs(got[k][i, j] - d) <= 64.0 * EPS * max(1.0, L0) / h, (name, form, k, i, j, got[k][i, j], d)


@pytest.mark.parametrize("name", tuple(rr.CASES))
def test_cases_keep_their_margins_and_cover_the_paths(name):
    c = rr.case(name)
    mg = rr.case_margins(name)
    none = int((~rr.live_rows(c["indices"], c["weights"], c["m"])).sum())
    print(f"  {name}: branch {mg['branch']:.1e}, |dot| {mg['dot']:.1e}, n2 {mg['n2']:.1e}, branches {mg['branches']}, flips {mg['flips']}, without a live entry {none}")
    assert mg["branch"] >= rr.MARGIN and mg["dot"] >= rr.MARGIN and mg["n2"] >= rr.MARGIN
    assert all(b > 0 for b in mg["branches"])   # every branch of the conversion among the nodes
    if c["k"] > 1:
        assert mg["flips"] > 0
    if name in ("n300_m9_far", "n300_m9_group", "n300_m70_dead"):
        assert 0 < none < c["n"]
    for form in rr.FORMS:   # float32 decides alike: its gradient is the float64's up to rounding, not up to a branch
        e = rr.f32_err(name, form)
        assert max(e.values()) < 1e-5, (form, e)
        # without a live entry the gradient passes through exactly; with bound_only it is zero
        cf = rr.case(name, form)
        dead = ~rr.live_rows(cf["indices"], cf["weights"], cf["m"])
        g, gb = rr.grad64(name, form), rr.grad64(name, form, bound_only=True)
        key = sg.orient_key(cf["rest"])
        assert np.array_equal(g["means"][dead], cf["d_means"][dead].astype(np.float64)) and np.array_equal(g[key][dead], cf["d_orient"][dead].astype(np.float64))
        assert (gb["means"][dead] == 0).all() and (gb[key][dead] == 0).all() and np.array_equal(gb["means"][~dead], g["means"][~dead])


def test_kit_sizes_and_entry_points_follow_the_library():
    assert {rr.case(n)["m"] for n in rr.CASES} >= {9, sr.LDS_NODES, sr.LDS_NODES + 1} and sr.LDS_NODES * 64 == _capi.SAS_SKIN_LDS_BYTES
    assert {rr.case(n)["n"] for n in rr.CASES} == {1, 257, 300} and {rr.case(n)["k"] for n in rr.CASES} == {1, 4, 5, 8}
    header = (ROOT / "include" / "sim_a_splat_amd.h").read_text()
    for name in ("sas_scene_deform_backward_rest", "sas_scene_adam_step_rest"):
        assert name in _capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert re.search(r"#define\s+SAS_DEFORM_REST_BOUND_ONLY\s+%du\b" % _capi.SAS_DEFORM_REST_BOUND_ONLY, header)
    # the Python front end
    assert "bound_only" in inspect.signature(Rasterizer.deform_backward_rest).parameters
    assert inspect.signature(Rasterizer.adam_step).parameters["rest"].default is False
    assert inspect.signature(autograd.render_differentiable).parameters["rest_params"].default is False
    assert callable(SplatScene.fit_dynamic)
    # one bounds code per checked site of the file, each a literal written once; the rest adjoint's three stand in its kernel, as arguments
    # of SAS_IN or of the helper that checks under the caller's code
    text = (ROOT / "sim_a_splat_amd" / "csrc" / "sas_skin.hip").read_text()
    code = "\n".join(line.split("//")[0] for line in text.split("\n"))
    assert sorted(int(v) for v in re.findall(r"\b15\d\d\b", code)) == list(range(1501, 1520))
    body = code[code.index("void k_deform_rest_grad"):]
    body = body[:body.index("\n}\n")]
    assert sorted(int(v) for v in re.findall(r"\([^;]*?, (15\d\d)\)", body)) == [1517, 1518, 1519]


def test_fit_dynamic_scene_on_the_reference():
    """Transforms known: the rest means, perturbed by noise, approach the truth from pictures of two bends while the tinted colours are
    fitted with them.  The error is the rest means' (the colours of Gaussians that lie under others are not determined by the pictures)."""
    res, e0, e1, R = rr.recover_on_reference()
    c = rr.dynamic_case()
    print(f"  dynamic fit on the reference: rest means' mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start; loss {res.history[0]:.4e} -> {res.history[-1]:.4e}")
    assert 0.03 < e0 < 0.06
    assert e1 < e0 and e1 < rr.DYN_FRACTION * e0
    assert abs(e1 / e0 - rr.DYN_REF_END) < 0.002   # the GPU test's comparison point
    assert res.steps == rr.DYN_ITERS == len(res.history) and res.history[-1] < 0.3 * res.history[0]
    assert res.transforms.shape == (2, 9, 3, 4) and np.array_equal(res.transforms, c["bends"])   # known transforms stay as given
    assert not np.array_equal(R.read_scene()["colors"].numpy().reshape(-1, 3), c["start"]["colors"].astype(np.float64))   # the colours were stepped too


def test_fit_dynamic_scene_joint_on_the_reference():
    """The second bend's transforms start at the identity and are fitted with the rest scene; step 0 is the anchor."""
    res, e0, e1, R = rr.recover_on_reference(joint=True)
    c = rr.dynamic_case()
    t0 = float(np.abs(sr.identity_transforms(9) - c["bends"][1]).max()), float(np.abs(res.transforms[1] - c["bends"][1]).max())
    print(f"  joint fit on the reference: rest means' mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start; loss {res.history[0]:.4e} -> "
          f"{res.history[-1]:.4e}; the second bend's transforms' largest entry error {t0[0]:.4f} -> {t0[1]:.4f}")
    assert abs(e1 / e0 - rr.DYN_JOINT_REF_END) < 0.002
    assert e1 < rr.DYN_JOINT_FRACTION * e0
    assert np.array_equal(res.transforms[0], c["bends"][0])   # the anchor stays fixed
    assert not np.array_equal(res.transforms[1], sr.identity_transforms(9).astype(np.float64))
    Rm = res.transforms[1, :, :, :3]
    assert np.abs(np.einsum("mki,mkj->mij", Rm, Rm) - np.eye(3)).max() < 1e-9   # the twists keep every node rigid
    assert res.history[-1] < 0.5 * res.history[0]
    assert len(rr.DYN_JOINT_HISTORY) == rr.DYN_ITERS and np.abs(np.asarray(res.history) - rr.DYN_JOINT_HISTORY).max() < 1e-6   # the GPU test's comparison point
    assert t0[1] < t0[0]


def test_fit_dynamic_scene_refusals():
    c = rr.dynamic_case()
    R = rr.DynRefRenderer(c, c["start"])
    kw = dict(renderer=R, iters=1)
    with pytest.raises(ValueError, match="what must name"):
        deform.fit_dynamic_scene(None, c["frames"], c["nodes"], what=("covariances",), **kw)
    with pytest.raises(ValueError, match=r"transforms must be \[2,9,3,4\]"):
        deform.fit_dynamic_scene(None, c["frames"], c["nodes"], transforms=c["bends"][:1], **kw)
    with pytest.raises(ValueError, match="frames is empty"):
        deform.fit_dynamic_scene(None, [], c["nodes"], **kw)
    with pytest.raises(ValueError, match="rigidity_weight"):
        deform.fit_dynamic_scene(None, c["frames"], c["nodes"], rigidity_weight=-1.0, **kw)
    with pytest.raises(ValueError, match="no skin is bound"):
        deform.fit_dynamic_scene(object(), c["frames"], c["nodes"], iters=1)
    with pytest.raises(ValueError, match="one size for all time steps"):
        deform.fit_dynamic_scene(None, [c["frames"][0], dict(c["frames"][1], images=c["frames"][1]["images"][:, :-1])], c["nodes"], **kw)
    with pytest.raises(ValueError, match="two answers"):
        deform.fit_dynamic_scene(None, c["frames"], c["nodes"], loss="dssim", loss_and_grad=lambda *a: None, **kw)
