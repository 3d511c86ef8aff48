"""GPU: density control on the resident scene (sas_density_accumulate / sas_scene_densify / sas_scene_reset_opacity, Rasterizer.densify,
fit.fit_scene(densify=); DESIGN.md 3, "Density control") against tests/tools/densify_ref.py, the numpy restatement.

The cases (tests/tools/densify_cases.py) keep every decision a factor two from its threshold, so parents, counts and everything that is
copied are compared EXACTLY; the children's scales are one float32 division, bit for bit; the children's means are held to the float64
restatement within FOUR times the float32 restatement's own error on the case (densify_cases.F32_ERR, held current by
tests/test_densify_cpu.py) -- sinf / cosf / logf of Box-Muller are the legal differences.  The carried optimiser state is held to fit_ref
under tests/test_gpu_u_fit.py's rule."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, fit
from sim_a_splat_amd.rasterizer import Rasterizer, SasError

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import densify_cases as dc  # noqa: E402
import densify_ref  # noqa: E402
import fit_cases as fc  # noqa: E402
import fit_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ARRAYS = ("means", "opacities", "colors", "quats", "scales")
OFF = dict(grow=False, prune_opacity_on=False, prune_scale_on=False)


def _read(r):
    return {k: v.cpu().numpy() for k, v in r.read_scene().items()}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _dev(r, d):
    return {k: torch.tensor(v, device=r.device) for k, v in d.items()}


def _steps(r, grads, first=1, lrs=fc.LRS):
    for t, g in enumerate(grads, start=first):
        r.adam_step(_dev(r, g), lrs, t)


def _gradients(n, kk, steps, seed):
    """[steps] dicts of float32 gradients for all five groups at n Gaussians: magnitudes log-uniform in [1e-4, 1], random signs."""
    rng = np.random.default_rng(seed)
    shapes = dict(means=(n, 3), opacities=(n,), colors=(n, kk, 3), quats=(n, 4), scales=(n, 3))
    return [{k: (10.0 ** rng.uniform(-4.0, 0.0, s) * rng.choice([-1.0, 1.0], s)).astype(np.float32) for k, s in shapes.items()} for _ in range(steps)]


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_against_restatement(rasterizer, name):
    r = rasterizer
    sc, stats, cfg = dc.case(name)
    ref = dc.reference(name)
    old = dc.ref_scene(sc)
    sc_kit.upload(r, sc)
    res = r.densify(_dev(r, stats), **cfg)
    # 1. parents, N_new and the counts
    assert (res["n"], res["cloned"], res["split"], res["pruned"]) == (ref["n"], ref["cloned"], ref["split"], ref["pruned"])
    assert r.n == ref["n"] and r.n_groups == sc["G"]
    parents = res["parents"].cpu().numpy()
    assert parents.dtype == np.int32 and np.array_equal(parents, ref["parents"])
    got = _read(r)
    first = ref["n_survivors"] + ref["cloned"]
    # 2. survivors and clones are their parents, bit for bit; children inherit everything but mean and scale
    for k in ARRAYS:
        assert _bits(got[k][:first], old[k][parents[:first]]), k
    for k in ("opacities", "colors", "quats"):
        assert _bits(got[k][first:], old[k][parents[first:]]), k
    # 3. the children's scales: scale / 1.6 in float32
    assert _bits(got["scales"][first:], ref["scene"]["scales"][first:])
    # 4. the children's means against float64
    if ref["split"]:
        x64 = ref["scene"]["means"][first:]
        err = float(np.abs(got["means"][first:].astype(np.float64) - x64).max() / np.abs(x64).max())
        f32 = dc.F32_ERR[name]
        print(f"DENSIFY {name:20s} children's means: hip {err:.3e}  float32 ref {f32:.3e}  ratio {err / f32:.2f}  bound {FACTOR * f32:.3e}  {'ok' if err <= FACTOR * f32 else 'MISS'}")
        assert err <= FACTOR * f32, (name, err, f32)
        kids = got["means"][first:].reshape(-1, 2, 3)
        assert not np.any(np.all(kids[:, 0] == kids[:, 1], axis=1))
    else:
        assert name not in dc.F32_ERR
    # 2b. the groups: a posed frame of the densified context against one of the restated scene uploaded fresh (poses stay, children move
    # with their parents' group)
    if sc["G"]:
        V, K, W, H = dc.camera()
        assert np.array_equal(r.get_group_poses().reshape(-1), np.asarray(sc["Rt"], np.float32).reshape(-1))
        a = sc_kit.to_numpy(r.render(V, K, W, H, fc.BACKGROUND))
        fresh = Rasterizer(0)
        try:
            sc_kit.upload(fresh, dc.kit_scene(sc, ref["scene"]))
            b = sc_kit.to_numpy(fresh.render(V, K, W, H, fc.BACKGROUND))
            sc_kit.upload(fresh, dict(dc.kit_scene(sc, ref["scene"]), gid=np.zeros(ref["n"], np.uint8)))   # everything in group 0: another frame
            c = sc_kit.to_numpy(fresh.render(V, K, W, H, fc.BACKGROUND))
        finally:
            fresh.close()
        for k in ("rgb", "alpha"):
            assert np.abs(a[k] - b[k]).max() <= 1e-4, (k, np.abs(a[k] - b[k]).max())
        moved = float(np.abs(a["rgb"] - c["rgb"]).max())   # (a scene of huge splats is a flat frame: ten times the bound is asked)
        assert moved > 1e-3 and (a["alpha"] > 0.5).mean() > 0.1, moved


def _carry_reference(sc, stats, cfg, g_old, g_new, dtype):
    S = fit_ref.new_state(fc.ref_scene(sc), dtype)
    for t, g in enumerate(g_old, start=1):
        fit_ref.step(S, g, fc.LRS, t)
    res = densify_ref.densify(dict(S["x"], gid=sc["gid"]), stats, cfg, dtype)
    T = densify_ref.carry_state(S, res, fit_ref)
    for t, g in enumerate(g_new, start=len(g_old) + 1):
        fit_ref.step(T, g, fc.LRS, t)
    return res, T


def test_optimiser_state_is_carried(rasterizer):
    """Two steps, densify, two more steps at the new N: fit_ref on the restated scene with the restated carried moments, under
    test_gpu_u_fit.py's bound.  With adam_reset() after the densify the result is far from it: the moments really were carried."""
    r = rasterizer
    name = "n600_sh3"
    sc, stats, cfg = dc.case(name)
    n, kk = sc["means"].shape[0], sc["colors"].shape[1]
    g_old = _gradients(n, kk, 2, 41)
    n_new = dc.reference(name)["n"]
    g_new = _gradients(n_new, kk, 2, 42)
    res, T = _carry_reference(sc, stats, cfg, g_old, g_new, np.float64)
    _, T32 = _carry_reference(sc, stats, cfg, g_old, g_new, np.float32)
    assert res["n"] == n_new and np.array_equal(res["parents"], dc.reference(name)["parents"])   # (the two steps flipped no decision)
    f32 = {k: fit_ref.rel_err(T32["x"][k], T["x"][k]) for k in ARRAYS}
    runs = {}
    for reset in (False, True):
        sc_kit.upload(r, sc)
        _steps(r, g_old)
        out = r.densify(_dev(r, stats), **cfg)
        assert out["n"] == n_new and np.array_equal(out["parents"].cpu().numpy(), res["parents"])
        if reset:
            r.adam_reset()
        _steps(r, g_new, first=3)
        runs[reset] = _read(r)
    bad = []
    for k in ARRAYS:
        e, lost = fit_ref.rel_err(runs[False][k], T["x"][k]), fit_ref.rel_err(runs[True][k], T["x"][k])
        print(f"DENSIFY carried state {k:10s} hip {e:.3e}  float32 ref {f32[k]:.3e}  ratio {e / f32[k]:.2f}  bound {FACTOR * f32[k]:.3e}  after adam_reset {lost:.3e}")
        if not e <= FACTOR * f32[k] or not lost > 10 * FACTOR * f32[k]:
            bad.append((k, e, lost, f32[k]))
    assert not bad, bad


def test_order_renewal_alone(rasterizer):
    """Every flag off: the scene is the same bits, parents is arange(N), and the next Adam step is the step without the call, bit for bit."""
    r = rasterizer
    sc, stats, _ = dc.case("n600_sh3")
    n, kk = sc["means"].shape[0], sc["colors"].shape[1]
    g = _gradients(n, kk, 3, 43)
    lrs = dict(fc.LRS, means=0.05)   # (the means move far: the new order is another one)
    sc_kit.upload(r, sc)
    _steps(r, g[:2], lrs=lrs)
    a = _read(r)
    out = r.densify(_dev(r, stats), **OFF)
    assert (out["n"], out["cloned"], out["split"], out["pruned"]) == (n, 0, 0, 0) and np.array_equal(out["parents"].cpu().numpy(), np.arange(n))
    b = _read(r)
    assert all(_bits(a[k], b[k]) for k in ARRAYS)
    _steps(r, g[2:], first=3, lrs=lrs)
    c = _read(r)
    sc_kit.upload(r, sc)
    _steps(r, g, lrs=lrs)
    d = _read(r)
    assert all(_bits(c[k], d[k]) for k in ARRAYS) and not _bits(c["means"], a["means"])


def test_reset_opacity(rasterizer):
    r = rasterizer
    name, cap = "sh1", 0.3
    sc = fc.scene(name)
    g = fc.draw_gradients(name, steps=3, seed_offset=7)
    sc_kit.upload(r, sc)
    _steps(r, g[:2])
    a = _read(r)
    assert np.abs(a["opacities"] - np.float32(cap)).min() > 1e-5
    r.reset_opacity(cap)
    with pytest.raises(SasError, match="no frame rendered"):
        r.read_projection()
    b = _read(r)
    over = a["opacities"] > np.float32(cap)
    assert 20 < over.sum() < fc.N - 20
    assert np.all(b["opacities"][over] == np.float32(cap)) and _bits(b["opacities"][~over], a["opacities"][~over])
    assert all(_bits(a[k], b[k]) for k in ARRAYS if k != "opacities")
    r.adam_step(_dev(r, dict(opacities=g[2]["opacities"])), fc.LRS, 3)
    got = _read(r)["opacities"]
    ref = {}
    for dtype in (np.float64, np.float32):
        S = fit_ref.run(fc.ref_scene(sc), g[:2], fc.LRS, dtype)
        dt = S["dt"]
        ch = S["x"]["opacities"] > dt(np.float32(cap))
        assert np.array_equal(ch, over)
        S["x"]["opacities"][ch] = dt(np.float32(cap))
        S["m"]["opacities"][ch] = 0
        S["v"]["opacities"][ch] = 0
        S["raw"]["opacities"][ch] = fit_ref.inverse_activation("opacities", S["x"]["opacities"][ch], dt)
        fit_ref.step(S, dict(opacities=g[2]["opacities"]), fc.LRS, 3)
        ref[dtype] = S["x"]["opacities"]
    f32 = fit_ref.rel_err(ref[np.float32], ref[np.float64])
    e = fit_ref.rel_err(got, ref[np.float64])
    print(f"DENSIFY reset_opacity: step after the reset hip {e:.3e}  float32 ref {f32:.3e}  ratio {e / f32:.2f}  bound {FACTOR * f32:.3e}")
    assert e <= FACTOR * f32
    # without optimiser state the planes alone change
    sc_kit.upload(r, sc)
    r.reset_opacity(cap)
    assert _bits(_read(r)["opacities"], np.minimum(sc["op"], np.float32(cap)))


def test_error_paths(rasterizer):
    r = rasterizer
    L = _capi.lib()
    fresh = Rasterizer(0)
    try:
        z = dict(grad_sum=torch.zeros(4, device=r.device), count=torch.zeros(4, dtype=torch.int32, device=r.device))
        fresh.n = 4
        with pytest.raises(SasError, match="status -3.*before sas_scene_upload"):
            fresh.densify(z)
        with pytest.raises(SasError, match="status -3.*before sas_scene_upload"):
            fresh.reset_opacity()
        with pytest.raises(SasError, match="status -3"):
            fresh.density_accumulate(64, 48, z)
    finally:
        fresh.close()
    sc, stats, cfg = dc.case("all_but_one_pruned")
    sc_kit.upload(r, sc)
    up = _read(r)
    st = _dev(r, stats)
    with pytest.raises(SasError, match="status -3.*no backward frame"):
        r.density_accumulate(64, 48, st)
    with pytest.raises(SasError, match="status -1.*every Gaussian would be pruned"):
        r.densify(st, **dict(cfg, prune_opacity=0.99, prune_scale_on=False, grow=False))
    for bad in (dict(grow_grad2d=-1.0), dict(prune_opacity=float("nan")), dict(scene_extent=0.0), dict(split_factor=1.0), dict(max_gaussians=-1)):
        with pytest.raises(SasError, match="status -1"):
            r.densify(st, **dict(cfg, **bad))
    with pytest.raises(ValueError, match="unknown settings"):
        r.densify(st, grow_grad=1.0)
    with pytest.raises(ValueError, match="new_density_stats"):
        r.densify(dict(grad_sum=st["grad_sum"][:-1], count=st["count"]))
    with pytest.raises(SasError, match="status -1.*outside"):
        r.reset_opacity(1.0)
    c = _capi.DensifyConfig(2e-4, 0.01, 0.005, 0.1, 1.0, 1.6, 0, 0, 8)
    counts = (ctypes.c_int64 * 4)()
    assert L.sas_scene_densify(r._ctx, ctypes.byref(c), st["grad_sum"].data_ptr(), st["count"].data_ptr(), None, counts, None) == -1
    assert b"unknown flags" in L.sas_last_error(r._ctx)
    assert L.sas_scene_densify(r._ctx, None, st["grad_sum"].data_ptr(), st["count"].data_ptr(), None, counts, None) == -1
    assert r.n == sc["means"].shape[0] and all(_bits(v, up[k]) for k, v in _read(r).items())   # none of the refused calls touched the scene
    # a scene of covariances has no scales: only opacity pruning applies
    cov = fc.scene("cov6")
    sc_kit.upload(r, cov)
    zc = r.new_density_stats()
    for on in (dict(grow=True, prune_scale_on=False), dict(grow=False, prune_scale_on=True)):
        with pytest.raises(SasError, match="status -1.*covariances"):
            r.densify(zc, **on)
    assert _bits(_read(r)["covariances"], cov["cov6"]) and r.n == fc.N
    out = r.densify(zc, grow=False, prune_scale_on=False, prune_opacity=0.5)
    keep = np.flatnonzero(~(cov["op"] < np.float32(0.5)))
    assert out["n"] == len(keep) and np.array_equal(out["parents"].cpu().numpy(), keep) and out["pruned"] == fc.N - len(keep)
    x = _read(r)
    assert _bits(x["covariances"], cov["cov6"][keep]) and _bits(x["means"], cov["means"][keep]) and _bits(x["colors"], cov["colors"][keep])


def _view(k):
    return sc_kit.ring(64, 48, f=50.0, yaw=25.0 + 70.0 * k, elev=0.2)[:2]


def _accumulate_scene():
    """600 Gaussians of moderate size: some culled, most seen."""
    rng = np.random.default_rng(61)
    n = 600
    means = rng.normal(0.0, 0.8, (n, 3)).astype(np.float32)
    means[:40, 2] += 6.0   # behind the first camera
    return dict(means=means, op=rng.uniform(0.2, 0.9, n).astype(np.float32), colors=rng.uniform(0.0, 1.0, (n, 1, 3)).astype(np.float32), sh=0,
                quats=rng.normal(size=(n, 4)).astype(np.float32), scales=rng.uniform(0.02, 0.1, (n, 3)).astype(np.float32), cov6=None, gid=None, G=0, Rt=None)


def test_accumulate_explicit_path_is_the_float32_restatement(rasterizer):
    """Two views of a 64x48 frame (0.5 W != 0.5 H), d_means2d from render_backward(screen_space=True) and the radii from read_projection:
    the same inputs, correctly rounded unfused operations, one add per call -- every statistic bit for bit."""
    r = rasterizer
    sc = _accumulate_scene()
    sc_kit.upload(r, sc)
    W, H = 64, 48
    g_rgb = np.random.default_rng(62).normal(size=(H, W, 3)).astype(np.float32)
    stats = r.new_density_stats()
    ref = dict(grad_sum=np.zeros(600, np.float32), count=np.zeros(600, np.int32), max_radius=np.zeros(600, np.float32))
    for k in range(2):
        V, K = _view(k)
        d = r.render_backward(V, K, W, H, g_rgb, screen_space=True, want=("means2d",))["means2d"]
        radii = r.read_projection()["radii"]
        r.density_accumulate(W, H, stats, d_means2d=d)
        densify_ref.accumulate(ref, d.cpu().numpy(), radii, W, H)
    got = {k: v.cpu().numpy() for k, v in stats.items()}
    assert 0 < (ref["count"] == 0).sum() and (ref["count"] == 2).sum() > 100 and (ref["grad_sum"] > 0).sum() > 100
    assert np.array_equal(got["count"], ref["count"]) and _bits(got["max_radius"], ref["max_radius"]) and _bits(got["grad_sum"], ref["grad_sum"])
    only = dict(grad_sum=stats["grad_sum"], count=stats["count"])   # max_radius may be left out
    r.render_backward(V, K, W, H, g_rgb, screen_space=True, want=("means2d",))
    r.density_accumulate(W, H, only, d_means2d=d)
    assert _bits(stats["max_radius"].cpu().numpy(), ref["max_radius"]) and np.array_equal(stats["count"].cpu().numpy(), ref["count"] + (radii[:, 0] > 0))
    with pytest.raises(SasError, match="status -3.*holds no sums"):   # a screen-space frame leaves no sums in the context
        r.density_accumulate(W, H, only)
    r.render(V, K, W, H)
    with pytest.raises(SasError, match="status -3.*no backward frame"):   # ... and any other frame ends the backward frame
        r.density_accumulate(W, H, only, d_means2d=d)


def test_accumulate_scratch_path(rasterizer):
    """After a full render_backward the context's own sums are used: count and max_radius are exact; grad_sum is held to the restatement on
    a separately computed screen-space gradient within four times the largest difference two such runs show between themselves (the float
    atomics' order), plus one float32 ulp of the sum."""
    r = rasterizer
    sc = _accumulate_scene()
    sc_kit.upload(r, sc)
    W, H = 64, 48
    g_rgb = np.random.default_rng(62).normal(size=(H, W, 3)).astype(np.float32)
    V, K = _view(0)
    norms = []
    for _ in range(2):
        d = r.render_backward(V, K, W, H, g_rgb, screen_space=True, want=("means2d",))["means2d"].cpu().numpy()
        radii = r.read_projection()["radii"]
        z = dict(grad_sum=np.zeros(600, np.float32), count=np.zeros(600, np.int32), max_radius=np.zeros(600, np.float32))
        norms.append(densify_ref.accumulate(z, d, radii, W, H))
    a, b = norms[0]["grad_sum"].astype(np.float64), norms[1]["grad_sum"].astype(np.float64)
    spread = float(np.abs(a - b).max() / np.abs(a).max())
    stats = r.new_density_stats()
    r.render_backward(V, K, W, H, g_rgb, want=("means",))
    r.density_accumulate(W, H, stats)
    got = {k: v.cpu().numpy() for k, v in stats.items()}
    assert np.array_equal(got["count"], norms[0]["count"]) and _bits(got["max_radius"], norms[0]["max_radius"])
    diff = np.abs(got["grad_sum"].astype(np.float64) - a)
    allowed = FACTOR * spread * np.abs(a).max() + np.spacing(norms[0]["grad_sum"]).astype(np.float64)
    print(f"DENSIFY accumulate (scratch path): two screen-space runs differ by {spread:.3e} of the largest norm; the scratch path by "
          f"{float(diff.max() / np.abs(a).max()):.3e}; {int((diff > 0).sum())} of {int((a > 0).sum())} sums differ")
    assert np.all(diff <= allowed), float((diff - allowed).max())


def test_fit_scene_with_densify_end_to_end(rasterizer):
    """The demo's scheme at toy size: targets from a 2 000-Gaussian synthetic scene, the fit started from a tenth of it, 60 steps with
    densification after every tenth.  N grows, the loss is finite and falls, every later frame renders.  No gap against the fixed-N fit
    is asserted: at 64x48 nearly every Gaussian exceeds the published gradient threshold, N doubles at every call, and the densified fit
    ends above the fixed-N one (measured on an MI355X: 2.87e-1 against 2.66e-1; the float64 CPU stand-in was not run at this size).  The
    figures of both fits are printed."""
    from sim_a_splat_amd.synthetic import make_scene
    r = rasterizer
    s = make_scene(2000, seed=5, log_scale_mean=float(np.log(0.04)))
    W, H = 64, 48
    cams = [sc_kit.ring(W, H, f=50.0, yaw=90.0 * k + 10.0, elev=0.3) for k in range(4)]
    V, K = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    full = dict(means=s.means, op=s.opacities, colors=s.sh, sh=s.sh_degree, quats=s.quats, scales=s.scales, cov6=None, gid=None, G=0, Rt=None)
    sc_kit.upload(r, full)
    targets = torch.stack([r.render(V[k], K[k], W, H)["rgb"].clone() for k in range(4)]).cpu().numpy()
    keep = np.sort(np.random.default_rng(6).choice(2000, 200, replace=False))
    what = ("means", "opacities", "colors", "quats", "scales")
    cfgd = fit.DensifyConfig(start=10, every=10, reset_every=0)
    out = {}
    for key, cfg in (("fixed", None), ("densify", cfgd)):
        sc_kit.upload(r, full, keep=keep)
        res = fit.fit_scene(r, V, K, W, H, targets, 60, what=what, loss="dssim", densify=cfg, seed=3)
        last = fit.mean_loss(r, V, K, W, H, targets, loss="dssim")
        out[key] = (res, last, r.n)
        print(f"DENSIFY end to end ({key}): N {len(keep)} -> {r.n}; history {res.history[0]:.4e} .. {res.history[-1]:.4e}; mean loss {last:.4e}")
    res, last, n = out["densify"]
    assert out["fixed"][0].n_history == [] and out["fixed"][2] == 200
    assert len(res.n_history) == 60 and res.n_history[:9] == [200] * 9 and res.n_history[-1] == n and n > 200
    assert all(b >= 1 for b in res.n_history) and np.all(np.isfinite(res.history)) and np.isfinite(last)
    assert np.mean(res.history[-10:]) < np.mean(res.history[:10])
    r.render(V[0], K[0], W, H)
    assert (r.read_projection()["radii"] > 0).any()   # the frame after the last densify rendered


def test_door_a_fit_with_densify():
    """GaussianSplat.fit(densify=) passes the config through and replaces every per-Gaussian parameter of the model at the new N."""
    from sim_a_splat_amd.gaussian_splat import GaussianSplat, PinholeCamera, SplatModel
    from sim_a_splat_amd.synthetic import c2w_opengl_from_viewmat
    rng = np.random.default_rng(2)
    n, W, H = 600, 48, 40
    geo = (rng.normal(0, 0.4, (n, 3)), np.log(rng.uniform(0.05, 0.12, (n, 3))), rng.normal(size=(n, 4)))
    dc_, rest, op = rng.normal(size=(n, 3)), rng.normal(0, 0.1, (n, 15, 3)), rng.normal(0.5, 1.5, (n, 1))
    poses = np.stack([c2w_opengl_from_viewmat(sc_kit.ring(W, H, f=40.0, yaw=30.0 + 120.0 * k, elev=0.1)[0]) for k in range(3)])
    cam = PinholeCamera(torch.from_numpy(poses[0, :3]), 40.0, 40.0, W / 2, H / 2, W, H)
    true = GaussianSplat.from_model(SplatModel(*geo, dc_, rest, op), cam)
    keep = np.arange(0, n, 4)
    model = SplatModel(*(a[keep] for a in geo), dc_[keep], rest[keep], op[keep])
    gs = GaussianSplat.from_model(model, cam)
    try:
        images = torch.stack([true.render(p)["rgb"].clone() for p in poses])
        res = gs.fit(poses, images, iters=30, what=ARRAYS, views_per_step=2, loss="dssim", densify=fit.DensifyConfig(start=10, every=10, reset_every=0))
        m = model.num_points
        assert res.steps == 30 and res.n_history[-1] == m == model._rasterizer().n and m > len(keep)
        assert tuple(model.quats.shape) == (m, 4) and tuple(model.scales.shape) == (m, 3) and tuple(model.opacities.shape) == (m, 1)
        assert tuple(model.features_dc.shape) == (m, 3) and tuple(model.features_rest.shape) == (m, 15, 3)
        x = model._rasterizer().read_scene()
        assert torch.equal(model.means, x["means"].cpu()) and torch.equal(model.features_dc.reshape(-1, 3), x["colors"][:, 0].cpu())
        assert torch.isfinite(gs.render(poses[0])["rgb"]).all()
    finally:
        model._rasterizer().close()
        true.pipeline.model._rasterizer().close()
