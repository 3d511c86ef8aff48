"""CPU: the yardstick of the optimiser step (tests/tools/fit_ref.py), what the GPU tests assume of their cases (tests/tools/fit_cases.py)
and the fitting loop on a CPU stand-in renderer.

- fit_ref is torch.optim.Adam on the raw variables, in float64, to 1e-12,
- its skip rules: non-finite gradients, values outside an activation's domain, groups without gradient or rate, visible-only,
- the float32 error table the GPU bounds rest on is current,
- the new entry points are declared, bound and built,
- sim_a_splat_amd.fit.fit_scene brings the fit case's loss to a quarter on the float64 reference renderer."""
import sys
from pathlib import Path

import numpy as np
import torch

from sim_a_splat_amd import _capi, build, fit

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import fit_cases as fc  # noqa: E402
import fit_ref  # noqa: E402


def test_symbols_declared_listed_and_built():
    header = (Path(build.PKG).parent / "include" / "sim_a_splat_amd.h").read_text()
    L = _capi.lib()
    for name in ("sas_scene_adam_step", "sas_scene_adam_reset", "sas_scene_read"):
        assert name in _capi.EXPORTS and f"int {name}(" in header and hasattr(L, name)
    assert build.CSRC / "sas_fit.hip" in build.SOURCES
    assert "typedef struct sas_adam_config" in header and "#define SAS_ADAM_VISIBLE_ONLY 1u" in header
    import ctypes
    assert ctypes.sizeof(_capi.AdamConfig) == 44 and len(L.sas_scene_adam_step.argtypes) == 8 and len(L.sas_scene_read.argtypes) == 7


def test_fit_ref_is_torch_adam_on_the_raw_variables():
    name = "sh1"
    h = lambda v: float(np.float32(v))   # the hyper-parameters as the C ABI carries them
    S = fit_ref.new_state(fc.ref_scene(fc.scene(name)))
    x = {k: torch.tensor(v) for k, v in S["x"].items()}
    raw = dict(means=x["means"].clone(), quats=x["quats"].clone(), dc=x["colors"][:, :1].clone(), rest=x["colors"][:, 1:].clone(),
               opacities=torch.logit(x["opacities"]), scales=torch.log(x["scales"]))
    rate = dict(means="means", quats="quats", dc="sh_dc", rest="sh_rest", opacities="opacities", scales="scales")
    opt = torch.optim.Adam([dict(params=[p.requires_grad_(True)], lr=h(fc.LRS[rate[k]])) for k, p in raw.items()], betas=(h(0.9), h(0.999)), eps=h(1e-15))
    for t, g in enumerate(fc.draw_gradients(name, steps=8), start=1):
        G = {k: torch.tensor(v.astype(np.float64)) for k, v in g.items()}
        o, s = torch.sigmoid(raw["opacities"].detach()), torch.exp(raw["scales"].detach())
        raw["means"].grad, raw["quats"].grad = G["means"], G["quats"]
        raw["dc"].grad, raw["rest"].grad = G["colors"][:, :1].clone(), G["colors"][:, 1:].clone()
        raw["opacities"].grad, raw["scales"].grad = G["opacities"] * o * (1 - o), G["scales"] * s
        opt.step()
        fit_ref.step(S, g, fc.LRS, t)
    got = dict(means=raw["means"], quats=raw["quats"], colors=torch.cat([raw["dc"], raw["rest"]], dim=1), opacities=torch.sigmoid(raw["opacities"]),
               scales=torch.exp(raw["scales"]))
    for k, v in got.items():
        moved = np.abs(S["x"][k] - x[k].numpy()).max()
        assert moved > 1e-4, (k, moved)
        assert np.abs(S["x"][k] - v.detach().numpy()).max() <= 1e-12, k


def test_fit_ref_skip_rules():
    sc = fc.ref_scene(fc.scene("sh1"))
    sc["opacities"] = sc["opacities"].copy()
    sc["scales"] = sc["scales"].copy()
    sc["opacities"][:5] = [0.0, 1.0, 1.5, -0.25, np.nan]
    sc["scales"][:4, 1] = [0.0, -1.0, np.inf, np.nan]
    g = fc.draw_gradients("sh1", steps=3)
    for d in g:
        d["means"][7, 2] = np.nan
        d["colors"][9, 1, 0] = np.inf
        d["opacities"][11] = -np.inf
        for k in d:
            d[k][20:40] = 0.0
    for dtype in (np.float64, np.float32):
        S0 = fit_ref.new_state(sc, dtype)
        S = fit_ref.run(sc, g, dict(fc.LRS, quats=0.0), dtype, visible_only=True)
        same = lambda k, idx: np.array_equal(S["x"][k][idx], S0["x"][k][idx], equal_nan=True)
        assert same("opacities", slice(0, 5)) and same("scales", (slice(0, 4), 1))          # outside the domain: fixed
        assert not same("scales", (slice(0, 4), 0))                                            # ... per element
        assert same("means", (7, 2)) and same("colors", (9, 1, 0)) and same("opacities", 11)   # non-finite gradient elements
        assert not same("means", (7, 0))
        assert all(same(k, slice(20, 40)) for k in S["x"])                                     # visible-only: skipped whole
        assert same("quats", slice(None)) and "quats" not in S["m"]                            # a zero rate: no state
        assert not same("means", slice(40, None))
        assert all(v.dtype == np.dtype(dtype) for v in S["x"].values())
    g = fc.draw_gradients("sh1", steps=3)   # seen in step 1, unseen afterwards: without the flag momentum goes on moving them
    for d in g[1:]:
        for k in d:
            d[k][20:40] = 0.0
    one, flag, plain = fit_ref.run(sc, g[:1], fc.LRS), fit_ref.run(sc, g, fc.LRS, visible_only=True), fit_ref.run(sc, g, fc.LRS)
    for k in ("means", "colors", "quats"):
        assert np.array_equal(flag["x"][k][20:40], one["x"][k][20:40]) and not np.array_equal(plain["x"][k][20:40], one["x"][k][20:40])
        assert np.array_equal(flag["x"][k][40:], plain["x"][k][40:])


def test_float32_error_table_is_current():
    """fit_cases.F32_ERR (the GPU bounds are four times it) is what fit_ref computes today: same keys, every figure within 5 % (the table
    keeps three digits; the restatement's exp and log are float64's, rounded, so the figures do not depend on the host)."""
    assert set(fc.F32_ERR) == set(fc.NAMES)
    for name in fc.NAMES:
        now = fc.float32_errors(name)
        assert set(now) == set(fc.F32_ERR[name]) == set(fc.groups_of(name))
        for k, v in now.items():
            assert v > 0 and abs(fc.F32_ERR[name][k] - v) <= 0.05 * v, (name, k, fc.F32_ERR[name][k], v)


def test_cases_are_what_the_gpu_tests_assume():
    for name in fc.NAMES:
        sc = fc.scene(name)
        n = sc["means"].shape[0]
        assert n == fc.N and n % 64 != 0
        deg = fc.CASES[name][0]
        assert np.asarray(sc["colors"]).size // n == {-1: 3, 1: 12, 2: 27, 3: 48}[deg]
        g = fc.draw_gradients(name)
        assert len(g) == fc.STEPS
        mags = np.abs(np.concatenate([v.reshape(-1) for v in g[0].values()]))
        assert 1e-4 * 0.99 <= mags.min() and mags.max() <= 1.0 and mags.min() < 1e-3 and mags.max() > 0.1
    assert fc.scene("groups3")["G"] == 3 and fc.scene("cov6")["cov6"] is not None and fc.scene("cov6")["quats"] is None


def test_fit_scene_on_the_reference_renderer():
    """The fit case (150 Gaussians, four 48x40 views, two per step, colours tinted and opacities scaled) on the float64 stand-in: the
    mean loss over all views falls to at most a quarter."""
    true, start, V, K, W, H = fc.fit_case()
    targets = fc.fit_targets(true, V, K, W, H)
    R = fc.RefRenderer(start)
    first = fit.mean_loss(R, V, K, W, H, targets, background=fc.FIT_BACKGROUND)
    res = fit.fit_scene(None, V, K, W, H, targets, fc.FIT["iters"], what=fc.FIT["what"], lrs=fc.FIT["lrs"], views_per_step=fc.FIT["views_per_step"],
                        background=fc.FIT_BACKGROUND, renderer=R)
    last = fit.mean_loss(R, V, K, W, H, targets, background=fc.FIT_BACKGROUND)
    print(f"FIT reference loop: loss {first:.4e} -> {last:.4e} ({last / first:.3f})")
    assert res.steps == fc.FIT["iters"] and len(res.history) == res.steps
    assert first > 0.02 and last <= 0.25 * first, (first, last)
    x = R.read_scene()
    assert np.array_equal(x["means"].numpy(), np.asarray(start["means"], np.float64))   # what was not named stays


def test_step_rates_and_default_loss():
    r = fit.step_rates(fit.DEFAULT_LRS, ("means", "colors"), 2.0, 1, 11)
    assert set(r) == {"means", "sh_dc", "sh_rest"} and abs(r["means"] - 3.2e-4) < 1e-12 and abs(r["sh_rest"] * 20 - r["sh_dc"]) < 1e-12
    assert abs(fit.step_rates(fit.DEFAULT_LRS, ("means",), 2.0, 11, 11)["means"] - 3.2e-6) < 1e-12
    rgb = torch.rand(5, 7, 3, dtype=torch.float64, requires_grad=True)
    tgt, mask = torch.rand(5, 7, 3, dtype=torch.float64), torch.rand(5, 7) > 0.4
    for m in (None, mask):
        loss, g = fit.l1_loss_and_grad(rgb.detach(), tgt, m)
        w = torch.ones(5, 7, 1, dtype=torch.float64) if m is None else m.double()[..., None]
        ref = (w * (rgb - tgt).abs()).sum() / (3 * w.sum())
        assert torch.allclose(loss, ref.detach(), rtol=1e-12) and torch.allclose(g, torch.autograd.grad(ref, rgb)[0], rtol=1e-12, atol=1e-15)
