"""GPU: the optimiser step on the resident scene (sas_scene_adam_step / sas_scene_adam_reset / sas_scene_read, Rasterizer.adam_step,
fit.fit_scene; DESIGN.md 3, "Optimiser step") against tests/tools/fit_ref.py, the float64 numpy restatement of the step.

Measure per variable group, through read_scene: max |x - x_ref| / max |x_ref| (fit_ref.rel_err).  Bound: FOUR times the same measure of
the reference evaluated in float32 against float64 on the same case -- fit_cases.F32_ERR, held current by tests/test_fit_cpu.py (float32
cannot do better than itself; the factor covers the kernel's legal differences: its exp, log and division).  What must not change is
compared bit for bit."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, fit
from sim_a_splat_amd.rasterizer import Rasterizer, SasError

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import fit_cases as fc  # noqa: E402
import fit_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _dev(r, g):
    return {k: torch.tensor(v, device=r.device) for k, v in g.items()}


def _read(r):
    return {k: v.cpu().numpy() for k, v in r.read_scene().items()}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _uploaded(sc):
    """What read_scene returns straight after sc_kit.upload(r, sc)."""
    n = sc["means"].shape[0]
    d = dict(means=sc["means"], opacities=sc["op"], colors=np.asarray(sc["colors"]).reshape(n, -1, 3))
    d.update(dict(quats=sc["quats"], scales=sc["scales"]) if sc["cov6"] is None else dict(covariances=sc["cov6"]))
    return d


def _steps(r, grads, lrs=fc.LRS, first=1, **kw):
    for t, g in enumerate(grads, start=first):
        r.adam_step(_dev(r, g), lrs, t, **kw)


def _hold(what, got, ref, f32_err):
    rows = [(k, fit_ref.rel_err(got[k], ref[k]), FACTOR * f32_err[k]) for k in f32_err]
    for k, e, b in rows:
        print(f"FIT {what:24s} {k:10s} hip {e:.3e}  float32 ref {f32_err[k]:.3e}  ratio {e / f32_err[k]:.2f}  bound {b:.3e}  {'ok' if e <= b else 'MISS'}")
    bad = [(k, e, b) for k, e, b in rows if not e <= b]
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", fc.NAMES)
def test_case_against_reference(rasterizer, name):
    r = rasterizer
    sc = fc.scene(name)
    sc_kit.upload(r, sc)
    up = _read(r)
    for k, v in _uploaded(sc).items():   # read_scene straight after upload: the uploaded arrays
        assert _bits(up[k], v), k
    _steps(r, fc.draw_gradients(name))
    got = _read(r)
    _hold(name, got, fc.reference(name)["x"], fc.F32_ERR[name])
    for k in fc.groups_of(name):
        assert not _bits(got[k], up[k]), k
    if name == "cov6":
        assert _bits(got["covariances"], sc["cov6"])   # not a variable


def test_groups_without_gradient_or_rate_stay(rasterizer):
    r = rasterizer
    name = "sh3"
    sc_kit.upload(r, fc.scene(name))
    up = _read(r)
    g = fc.draw_gradients(name, steps=4)
    _steps(r, g[:2], lrs=dict(opacities=5e-2, means=0.0))               # every gradient given, one rate
    a = _read(r)
    assert not _bits(a["opacities"], up["opacities"]) and all(_bits(a[k], up[k]) for k in ("means", "colors", "quats", "scales"))
    _steps(r, [dict(colors=d["colors"]) for d in g[:2]], lrs=fc.LRS)   # every rate given, one gradient
    b = _read(r)
    assert not _bits(b["colors"], a["colors"]) and all(_bits(b[k], a[k]) for k in ("means", "opacities", "quats", "scales"))
    _steps(r, g[2:], lrs=dict(sh_dc=1e-2), first=3)                     # the DC triple alone
    c = _read(r)
    assert _bits(c["colors"][:, 1:], b["colors"][:, 1:]) and not np.any(c["colors"][:, 0] == b["colors"][:, 0])
    assert all(_bits(c[k], b[k]) for k in ("means", "opacities", "quats", "scales"))


def test_visible_only_skips_unseen_gaussians_and_their_moments(rasterizer):
    """Gaussians 20..59 are seen in steps 1-3, unseen (exact zeros) in steps 4-8, seen again in steps 9-12.  While unseen they keep their
    bits; afterwards they follow the reference that skipped them (its float32 error on this run, times four) and are far from the one
    whose momentum went on."""
    r = rasterizer
    name = "sh2"
    sc = fc.scene(name)
    g = fc.draw_gradients(name, steps=12, seed_offset=5)
    Z = slice(20, 60)
    for d in g[3:8]:
        for k in d:
            d[k][Z] = 0.0
    sc_kit.upload(r, sc)
    _steps(r, g[:3], visible_only=True)
    a = _read(r)
    _steps(r, g[3:8], first=4, visible_only=True)
    b = _read(r)
    for k in a:
        assert _bits(b[k][Z], a[k][Z]), k
        assert not _bits(b[k][60:], a[k][60:]), k
    _steps(r, g[8:], first=9, visible_only=True)
    got = _read(r)
    rs = fc.ref_scene(sc)
    ref, ref32 = fit_ref.run(rs, g, fc.LRS, visible_only=True)["x"], fit_ref.run(rs, g, fc.LRS, np.float32, visible_only=True)["x"]
    plain = fit_ref.run(rs, g, fc.LRS)["x"]
    f32 = {k: fit_ref.rel_err(ref32[k], ref[k]) for k in ref}
    _hold("visible_only", got, ref, f32)
    for k in ref:
        assert fit_ref.rel_err(got[k][Z], plain[k][Z]) > 100 * FACTOR * f32[k], k


def test_non_finite_gradients_and_values_outside_the_domain_change_nothing(rasterizer):
    r = rasterizer
    name = "sh1"
    sc = fc.scene(name)
    sc["op"] = sc["op"].copy()
    sc["scales"] = sc["scales"].copy()
    sc["op"][:5] = [0.0, 1.0, 1.5, -0.25, np.nan]
    sc["scales"][:4, 1] = [0.0, -1.0, np.inf, np.nan]
    g = fc.draw_gradients(name, seed_offset=9)
    poison = dict(means=(7, 2), colors=(9, 1, 0), opacities=(11,), quats=(13, 3), scales=(15, 0))
    for t, d in enumerate(g):
        for k, idx in poison.items():
            d[k][idx] = (np.nan, np.inf, -np.inf)[t % 3]
    sc_kit.upload(r, sc)
    up = _read(r)
    _steps(r, g)
    got = _read(r)
    for k, idx in poison.items():
        assert _bits(got[k][idx], up[k][idx]), k
    assert _bits(got["opacities"][:5], up["opacities"][:5]) and _bits(got["scales"][:4, 1], up["scales"][:4, 1])
    assert not np.any(got["scales"][:4, 0] == up["scales"][:4, 0])   # per element: the other components of those Gaussians step
    rs = fc.ref_scene(sc)
    ref, ref32 = fit_ref.run(rs, g, fc.LRS)["x"], fit_ref.run(rs, g, fc.LRS, np.float32)["x"]
    fin = {k: np.isfinite(ref[k]) for k in ref}
    assert all(np.array_equal(np.isfinite(got[k]), fin[k]) for k in ref)
    clean = lambda x: {k: np.where(fin[k], x[k], 0.0) for k in ref}
    _hold("non-finite", clean(got), clean(ref), {k: fit_ref.rel_err(clean(ref32)[k], clean(ref)[k]) for k in ref})


@pytest.mark.parametrize("name", ["groups3", "sh2"])
def test_planes_stay_well_formed(rasterizer, name):
    """After the steps a frame of the stepped context equals, bit for bit, a frame of a second context freshly uploaded with read_scene's
    arrays (groups and group poses included), and the oracle's frame of those arrays; features uploaded before the steps still render."""
    import oracle
    r = rasterizer
    sc = fc.scene(name)
    V, K, W, H = fc.camera()
    feats = np.random.default_rng(3).normal(size=(fc.N, 5)).astype(np.float32)
    sc_kit.upload(r, sc)
    r.upload_features(feats)
    before = sc_kit.to_numpy(r.render(V, K, W, H, fc.BACKGROUND, want=sc_kit.OUTS))
    _steps(r, fc.draw_gradients(name))
    x = _read(r)
    now = dict(sc, means=x["means"], op=x["opacities"], colors=x["colors"], quats=x["quats"], scales=x["scales"])
    a = sc_kit.to_numpy(r.render(V, K, W, H, fc.BACKGROUND, want=sc_kit.OUTS))
    fa = r.render_features(V, K, W, H)["features"].cpu().numpy()
    assert r.n == fc.N and r.n_groups == sc["G"] and r.n_features == 5
    fresh = Rasterizer(0)
    try:
        sc_kit.upload(fresh, now)
        fresh.upload_features(feats)
        b = sc_kit.to_numpy(fresh.render(V, K, W, H, fc.BACKGROUND, want=sc_kit.OUTS))
        fb = fresh.render_features(V, K, W, H)["features"].cpu().numpy()
    finally:
        fresh.close()
    sc_kit.same(a, b)
    assert _bits(fa, fb)
    assert np.abs(a["rgb"] - before["rgb"]).max() > 1e-3 and (a["alpha"] > 0.5).mean() > 0.1   # the steps show, and something is in view
    ref = sc_kit.oracle_frame(now, (V, K, W, H), fc.BACKGROUND)
    for k in ("rgb", "alpha"):
        assert np.abs(a[k] - ref[k]).max() <= 1e-4, k


def test_read_projection_after_a_step_is_of_the_new_scene(rasterizer):
    r = rasterizer
    name = "sh1"
    sc = fc.scene(name)
    V, K, W, H = fc.camera()
    sc_kit.upload(r, sc)
    r.render(V, K, W, H)
    p0 = r.read_projection()
    _steps(r, fc.draw_gradients(name, steps=3))
    with pytest.raises(SasError, match="no frame rendered"):
        r.read_projection()
    with pytest.raises(SasError, match="no frame rendered"):
        r.read_tile_lists(1)
    r.render(V, K, W, H)
    p1 = r.read_projection()
    x = _read(r)
    fresh = Rasterizer(0)
    try:
        sc_kit.upload(fresh, dict(sc, means=x["means"], op=x["opacities"], colors=x["colors"], quats=x["quats"], scales=x["scales"]))
        fresh.render(V, K, W, H)
        p2 = fresh.read_projection()
    finally:
        fresh.close()
    for k in p1:
        assert np.array_equal(p1[k], p2[k]), k
    assert not np.array_equal(p1["means2d"], p0["means2d"]) and (p1["radii"] > 0).any()


def test_state_goes_with_reset_and_upload(rasterizer):
    """After adam_reset, and after a new upload, steps counted from 1 give what a fresh context gives from the same arrays, bit for bit."""
    r = rasterizer
    name = "sh1"
    sc = fc.scene(name)
    g = fc.draw_gradients(name, steps=8, seed_offset=2)
    sc_kit.upload(r, sc)
    _steps(r, g[:4])
    x = _read(r)
    mid = dict(sc, means=x["means"], op=x["opacities"], colors=x["colors"], quats=x["quats"], scales=x["scales"])
    r.adam_reset()
    assert all(_bits(v, x[k]) for k, v in _read(r).items())   # the scene itself stays
    _steps(r, g[4:])
    after_reset = _read(r)
    sc_kit.upload(r, sc)
    _steps(r, g[:2])
    sc_kit.upload(r, mid)       # a new upload drops the state of the two steps before it
    _steps(r, g[4:])
    after_upload = _read(r)
    fresh = Rasterizer(0)
    try:
        sc_kit.upload(fresh, mid)
        _steps(fresh, g[4:])
        want = _read(fresh)
    finally:
        fresh.close()
    carried = fit_ref.run(fc.ref_scene(sc), g, fc.LRS)["x"]   # (moments carried over the reset would have given this instead)
    for k in want:
        assert _bits(after_reset[k], want[k]) and _bits(after_upload[k], want[k]), k
        assert fit_ref.rel_err(want[k], carried[k]) > 1e-4, k


def test_error_paths(rasterizer):
    r = rasterizer
    L = _capi.lib()
    name = "sh1"
    g = _dev(r, fc.draw_gradients(name, steps=1)[0])
    fresh = Rasterizer(0)
    try:
        fresh.n, fresh.sh_degree = fc.N, 1
        with pytest.raises(SasError, match="status -3.*before sas_scene_upload"):
            fresh.adam_step(g, fc.LRS, 1)
        with pytest.raises(SasError, match="status -3.*before sas_scene_upload"):
            fresh.read_scene()
        fresh.adam_reset()
    finally:
        fresh.close()
    sc_kit.upload(r, fc.scene(name))
    up = _read(r)
    with pytest.raises(SasError, match="status -1.*every gradient is NULL"):
        r.adam_step({}, fc.LRS, 1)
    with pytest.raises(SasError, match="status -1.*step 0 < 1"):
        r.adam_step(g, fc.LRS, 0)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(SasError, match="status -1.*learning rate"):
            r.adam_step(g, dict(fc.LRS, scales=bad), 1)
    with pytest.raises(SasError, match="status -1.*betas"):
        r.adam_step(g, fc.LRS, 1, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="unknown learning rates"):
        r.adam_step(g, dict(colors=1e-3), 1)
    with pytest.raises(ValueError, match="must be a contiguous float32"):
        r.adam_step(dict(means=g["means"][:-1]), fc.LRS, 1)
    cfg = _capi.AdamConfig(1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 0.9, 0.999, 1e-15, 1, 2)
    assert L.sas_scene_adam_step(r._ctx, ctypes.byref(cfg), g["means"].data_ptr(), None, None, None, None, None) == -1
    assert b"unknown flags" in L.sas_last_error(r._ctx)
    assert L.sas_scene_adam_step(r._ctx, None, g["means"].data_ptr(), None, None, None, None, None) == -1
    out6 = torch.zeros((fc.N, 6), device=r.device)
    assert L.sas_scene_read(r._ctx, None, None, None, out6.data_ptr(), None, None) == -1 and b"quaternions and scales" in L.sas_last_error(r._ctx)
    assert all(_bits(v, up[k]) for k, v in _read(r).items())   # none of the refused calls touched the scene
    # a scene of covariances: they are not variables
    sc = fc.scene("cov6")
    sc_kit.upload(r, sc)
    cfg.flags = 0
    for args in ((None, None, None, g["quats"].data_ptr(), None), (None, None, None, None, g["scales"].data_ptr())):
        assert L.sas_scene_adam_step(r._ctx, ctypes.byref(cfg), *args, None) == -1 and b"covariances" in L.sas_last_error(r._ctx)
    with pytest.raises(ValueError, match="covariances, which are not variables"):
        r.adam_step(g, fc.LRS, 1)
    out4 = torch.zeros((fc.N, 4), device=r.device)
    assert L.sas_scene_read(r._ctx, None, out4.data_ptr(), None, None, None, None) == -1
    host = np.zeros((fc.N, 3), np.float32)   # a host destination
    assert L.sas_scene_read(r._ctx, host.ctypes.data, None, None, None, None, None) == 0 and _bits(host, sc["means"])
    r.adam_step(dict(means=g["means"], opacities=g["opacities"]), fc.LRS, 1)   # the context stays usable
    assert not _bits(_read(r)["means"], sc["means"])


def test_fit_scene_end_to_end(rasterizer):
    """The fit case of tests/test_fit_cpu.py through the HIP renderer: the float64 reference loop reaches a quarter of the initial loss;
    half of it is asked here -- the room for float32 and for the backward pass's atomic summation order."""
    r = rasterizer
    true, start, V, K, W, H = fc.fit_case()
    targets = fc.fit_targets(true, V, K, W, H)
    sc_kit.upload(r, start)
    first = fit.mean_loss(r, V, K, W, H, targets, background=fc.FIT_BACKGROUND)
    res = fit.fit_scene(r, V, K, W, H, targets, fc.FIT["iters"], what=fc.FIT["what"], lrs=fc.FIT["lrs"], views_per_step=fc.FIT["views_per_step"],
                        background=fc.FIT_BACKGROUND)
    last = fit.mean_loss(r, V, K, W, H, targets, background=fc.FIT_BACKGROUND)
    print(f"FIT end to end (HIP): loss {first:.4e} -> {last:.4e} ({last / first:.3f}); history {res.history[0]:.4e} .. {res.history[-1]:.4e}")
    assert res.steps == fc.FIT["iters"]
    assert first > 0.02 and last <= 0.5 * first, (first, last)
    x = _read(r)
    assert _bits(x["means"], start["means"]) and _bits(x["scales"], start["scales"]) and _bits(x["quats"], start["quats"])


def test_door_a_fit():
    """GaussianSplat.fit is fit_scene on the model's rasterizer with camera 0's intrinsics and the model's background; the fitted arrays
    go back into the model's raw parameters."""
    from sim_a_splat_amd.gaussian_splat import GaussianSplat, PinholeCamera, SplatModel
    from sim_a_splat_amd.synthetic import c2w_opengl_from_viewmat
    rng = np.random.default_rng(2)
    n, W, H = 600, 48, 40
    par = lambda: (rng.normal(0, 0.4, (n, 3)), np.log(rng.uniform(0.05, 0.12, (n, 3))), rng.normal(size=(n, 4)))
    geo = par()
    dc, rest, op = rng.normal(size=(n, 3)), rng.normal(0, 0.1, (n, 15, 3)), rng.normal(0.5, 1.5, (n, 1))
    poses = np.stack([c2w_opengl_from_viewmat(sc_kit.ring(W, H, f=40.0, yaw=30.0 + 120.0 * k, elev=0.1)[0]) for k in range(3)])
    cam = PinholeCamera(torch.from_numpy(poses[0, :3]), 40.0, 40.0, W / 2, H / 2, W, H)
    true = GaussianSplat.from_model(SplatModel(*geo, dc, rest, op), cam)
    model = SplatModel(*geo, 0.6 * dc + 0.3, 0.6 * rest, op - 0.8)
    gs = GaussianSplat.from_model(model, cam)
    try:
        images = torch.stack([true.render(p)["rgb"].clone() for p in poses])
        loss = lambda: float(np.mean([float((gs.render(p)["rgb"] - im).abs().mean()) for p, im in zip(poses, images)]))
        first = loss()
        dc0, means0 = model.features_dc.clone(), model.means.clone()
        res = gs.fit(poses, images, iters=60, views_per_step=2, lrs=dict(sh_dc=3e-2, sh_rest=3e-3))
        last = loss()
        print(f"FIT door A: loss {first:.4e} -> {last:.4e}")
        assert res.steps == 60 and last < 0.5 * first
        assert not torch.equal(model.features_dc, dc0) and torch.equal(model.means, means0)
        x = model._rasterizer().read_scene()
        assert torch.allclose(torch.sigmoid(model.opacities).reshape(-1), x["opacities"].cpu(), atol=1e-6)
        assert torch.equal(model.features_dc.reshape(-1, 3), x["colors"][:, 0].cpu())
    finally:
        model._rasterizer().close()
        true.pipeline.model._rasterizer().close()
