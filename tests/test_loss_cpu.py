"""CPU: the yardstick of the photometric loss (tests/tools/loss_ref.py), the cases the GPU test runs (tests/tools/loss_cases.py) and the
fitting loop with ``loss="dssim"`` on a CPU stand-in renderer.

- loss_ref in float64 is the conv2d-and-autograd form of the definition in torch, value and gradient, to 1e-12, prechained through
  autograd.prechain,
- the float32 error table the GPU bounds rest on is current,
- the entry point is declared, bound and built,
- fit_scene's new arguments are checked, and ``loss=None`` never touches ``photometric_loss``,
- fit_scene(loss="dssim") brings the fit case's combined loss down on the float64 reference renderer."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, build, fit
from sim_a_splat_amd.autograd import prechain

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import fit_cases as fc  # noqa: E402
import loss_cases as lc  # noqa: E402
import loss_ref  # noqa: E402


def torch_loss(x, y, w, lam):
    """The definition as a user would have written it before the kernels: five grouped 11x11 conv2d over [1,3,H,W], in x's dtype."""
    g = torch.as_tensor(loss_ref.window(), dtype=x.dtype, device=x.device)
    k = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    X, Y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    blur = lambda a: torch.nn.functional.conv2d(a, k, padding=5, groups=3)
    mx, my = blur(X), blur(Y)
    vx, vy, cxy = blur(X * X) - mx * mx, blur(Y * Y) - my * my, blur(X * Y) - mx * my
    ssim_p = ((2 * mx * my + loss_ref.C1) * (2 * cxy + loss_ref.C2)) / ((mx * mx + my * my + loss_ref.C1) * (vx + vy + loss_ref.C2))
    W = torch.ones_like(X[:, :1]) if w is None else w.to(x.dtype)[None, None]
    D = torch.clamp(3.0 * W.sum(), min=1.0)
    l1, ssim, mse = (W * (X - Y).abs()).sum() / D, (W * ssim_p).sum() / D, (W * (X - Y) ** 2).sum() / D
    return (1.0 - lam) * l1 + lam * (1.0 - ssim), l1, ssim, mse


@pytest.mark.parametrize("name", lc.NAMES)
def test_reference_is_the_torch_form(name):
    x32, y32 = lc.case(name)
    for masked in (False, True):
        for lam in lc.LAMBDAS + (0.0,):
            x = torch.tensor(x32, dtype=torch.float64, requires_grad=True)
            y = torch.tensor(y32, dtype=torch.float64)
            w = torch.tensor(lc.mask(name)) if masked else None
            terms = torch_loss(x, y, w, lam)
            (gx,) = torch.autograd.grad(terms[0], x)
            ref = loss_ref.evaluate(x32, y32, lc.mask(name) if masked else None, lam)
            pre = loss_ref.evaluate(x32, y32, lc.mask(name) if masked else None, lam, lc.BACKGROUND)
            for a, b in zip(ref["terms"], [t.detach() for t in terms]):
                assert abs(a - float(b)) <= 1e-12 * abs(float(b)), (name, masked, lam)
            scale = float(gx.abs().max())
            assert scale > 0 and np.abs(ref["g_rgb"] - gx.numpy()).max() <= 1e-12 * scale
            zeros = torch.zeros(x.shape[:2], dtype=torch.float64)
            g_acc, g_a, _ = prechain(x.detach(), zeros, zeros, lc.BACKGROUND, gx, None, None)
            assert np.abs(pre["g_rgb"] - g_acc.numpy()).max() <= 1e-12 * scale
            assert np.abs(pre["g_alpha"] - g_a.numpy()).max() <= 1e-12 * scale
            assert np.array_equal(pre["terms"], ref["terms"])


def test_cases_are_what_the_gpu_tests_assume():
    for name in lc.NAMES:
        x, y = lc.case(name)
        W, H = lc.SIZES[name]
        assert x.shape == y.shape == (H, W, 3) and x.dtype == y.dtype == np.float32
        assert x.min() >= 0.0 and x.max() <= 1.0 and y.min() >= 0.0 and y.max() <= 1.0
        zeros = 1.0 - lc.mask(name).mean()
        assert 0.15 < zeros < 0.45, (name, zeros)
    x, y = lc.case("flat")
    assert (x[:, 10:12] == 1.0).all() and (x[:, 30:33] == 0.0).all() and (x == y).mean() >= 0.2
    assert lc.SIZES["tiny"][0] < 11 and lc.SIZES["tiny"][1] < 11 and lc.SIZES["tile"] == (16, 16)
    assert lc.SIZES["ragged"][0] % 16 and lc.SIZES["ragged"][1] % 16   # partial tiles both ways
    assert all(lc.SIZES[n][0] > 32 and lc.SIZES[n][1] > 16 and lc.SIZES[n][1] % 16 for n in ("ragged", "smooth", "flat"))   # 3 x 2 tiles and more
    x, _ = lc.case("frame")
    assert lc.SIZES["frame"] == (fc.FIT["W"], fc.FIT["H"]) and 0.05 < (x == np.float32(0.1))[..., 0].mean() < 0.95   # background shows


def test_float32_error_table_is_current():
    """loss_cases.F32_ERR (the GPU bounds are four times it) is what loss_ref computes today: same keys, every figure within 5 % (the
    table keeps three digits; the restatement uses +, -, *, / and comparisons of binary32 only, so the figures do not depend on the host)."""
    assert set(lc.F32_ERR) == set(lc.keys())
    for key in lc.keys():
        now = lc.float32_errors(*key)
        assert tuple(now) == tuple(lc.F32_ERR[key]) == lc.FIGURES
        for k, v in now.items():
            assert v > 0 and abs(lc.F32_ERR[key][k] - v) <= 0.05 * v, (key, k, lc.F32_ERR[key][k], v)


def test_float32_restatement_skips_ssim_at_lambda_zero():
    x, y = lc.case("ragged")
    r = loss_ref.evaluate(x, y, lc.mask("ragged"), 0.0, dtype=np.float32)
    ref = loss_ref.evaluate(x, y, lc.mask("ragged"), 0.0)
    assert np.isnan(r["terms"][2]) and r["terms"][0] == r["terms"][1] and r["g_rgb"].dtype == np.float32
    assert abs(r["terms"][0] - ref["terms"][0]) <= 1e-6 * ref["terms"][0] and loss_ref.rel_err(r["g_rgb"], ref["g_rgb"]) <= 1e-6


def test_symbol_declared_listed_and_built():
    header = (Path(build.PKG).parent / "include" / "sim_a_splat_amd.h").read_text()
    L = _capi.lib()
    assert "sas_photometric_loss" in _capi.EXPORTS and "int sas_photometric_loss(" in header and hasattr(L, "sas_photometric_loss")
    assert build.CSRC / "sas_loss.hip" in build.SOURCES and len(L.sas_photometric_loss.argtypes) == 13


class _NoLoss:
    """A renderer without photometric_loss: one 2x2 frame, gradients of the right shapes."""

    def __init__(self):
        self.steps = 0

    def render(self, V, K, W, H, background=(0.0, 0.0, 0.0), **kw):
        return dict(rgb=torch.full((H, W, 3), 0.25, dtype=torch.float64), alpha=torch.ones((H, W, 1), dtype=torch.float64),
                    depth=torch.ones((H, W, 1), dtype=torch.float64))

    def render_backward(self, V, K, W, H, g_rgb=None, g_alpha=None, g_depth=None, *, out=None, want=None, **kw):
        return dict(colors=torch.zeros(1, 1, 3), opacities=torch.zeros(1))

    def adam_step(self, grads, lrs, step, **kw):
        self.steps += 1


def test_fit_scene_argument_checks():
    V, K = np.eye(4, dtype=np.float32)[None], np.eye(3, dtype=np.float32)[None]
    images = np.full((1, 2, 2, 3), 0.5, np.float32)
    R = _NoLoss()
    assert not hasattr(R, "photometric_loss")
    res = fit.fit_scene(None, V, K, 2, 2, images, 3, renderer=R)   # loss=None: today's path, no photometric_loss anywhere
    assert res.steps == 3 and R.steps == 3 and all(abs(h - 0.25) < 1e-12 for h in res.history)
    assert abs(fit.mean_loss(R, V, K, 2, 2, images) - 0.25) < 1e-12
    lg = lambda rgb, target, mask: fit.l1_loss_and_grad(rgb, target, mask)
    with pytest.raises(ValueError, match="loss must be None or one of"):
        fit.fit_scene(None, V, K, 2, 2, images, 1, renderer=R, loss="ssim")
    with pytest.raises(ValueError, match="loss_and_grad"):
        fit.fit_scene(None, V, K, 2, 2, images, 1, renderer=R, loss="dssim", loss_and_grad=lg)
    with pytest.raises(ValueError, match="lambda_dssim"):
        fit.fit_scene(None, V, K, 2, 2, images, 1, renderer=R, loss="dssim", lambda_dssim=1.5)
    with pytest.raises(ValueError, match="loss must be None or one of"):
        fit.mean_loss(R, V, K, 2, 2, images, loss="l2")
    with pytest.raises(ValueError, match="loss_and_grad"):
        fit.mean_loss(R, V, K, 2, 2, images, loss="dssim", loss_and_grad=lg)
    assert R.steps == 3   # none of the refused calls rendered or stepped


class LossRefRenderer(fc.RefRenderer):
    """fit_cases' float64 stand-in with Rasterizer.photometric_loss's signature on loss_ref."""
    calls = 0

    def photometric_loss(self, rgb, target, *, mask=None, alpha=None, background=(0.0, 0.0, 0.0), lambda_dssim=0.2, want_grad=True):
        LossRefRenderer.calls += 1
        num = lambda t: None if t is None else (t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
        x = num(rgb)
        r = loss_ref.evaluate(x, num(target).reshape(x.shape), num(mask), lambda_dssim, None if alpha is None else background, grad=want_grad)
        terms = torch.tensor(r["terms"])
        res = dict(terms=terms, loss=terms[0], l1=terms[1], ssim=terms[2], mse=terms[3])
        res.update({k: torch.tensor(r[k]) for k in ("g_rgb", "g_alpha") if k in r})
        return res


def test_fit_scene_dssim_on_the_reference_renderer():
    """The fit case of tests/test_fit_cpu.py descending (1 - 0.2) L1 + 0.2 (1 - SSIM): the combined loss over ALL views falls to at most
    half again above the fraction this float64 loop reaches (loss_cases.FIT_DSSIM_RATIO)."""
    true, start, V, K, W, H = fc.fit_case()
    targets = fc.fit_targets(true, V, K, W, H)
    R = LossRefRenderer(start)
    kw = dict(background=fc.FIT_BACKGROUND, loss="dssim", lambda_dssim=lc.FIT_LAMBDA)
    first = fit.mean_loss(R, V, K, W, H, targets, **kw)
    before = LossRefRenderer.calls
    res = fit.fit_scene(None, V, K, W, H, targets, fc.FIT["iters"], what=fc.FIT["what"], lrs=fc.FIT["lrs"], views_per_step=fc.FIT["views_per_step"],
                        renderer=R, **kw)
    assert LossRefRenderer.calls - before == fc.FIT["iters"] * fc.FIT["views_per_step"]
    last = fit.mean_loss(R, V, K, W, H, targets, **kw)
    print(f"FIT dssim reference loop: loss {first:.4e} -> {last:.4e} ({last / first:.3f}); asserted <= {1.5 * lc.FIT_DSSIM_RATIO:.3f}")
    assert res.steps == fc.FIT["iters"] and len(res.history) == res.steps and all(np.isfinite(res.history))
    assert abs(res.history[0] - first) < 0.5 * first   # history holds the combined loss (of the step's views), not the L1 term
    assert first > 0.04 and last <= 1.5 * lc.FIT_DSSIM_RATIO * first, (first, last)
    x = R.read_scene()
    assert np.array_equal(x["means"].numpy(), np.asarray(start["means"], np.float64))
