"""The drawn cases of the photometric-loss tests (tests/test_loss_cpu.py, tests/test_gpu_v_loss.py): the smallest images at which the
kernels of sas_loss.hip can still go wrong, fixed seeds, each with and without a mask of about 30 % zeros.

    python tests/tools/loss_cases.py        prints F32_ERR as it stands today

  tiny     7x5     the whole image lies inside the window's padding
  tile     16x16   exactly one tile
  ragged   37x23   random; partial tiles in both directions
  smooth   48x33   a smooth target plus noise; halos cross tile borders both ways
  flat     48x33   constant 0.5 against halves of 0.5 / 0.52 (g*x^2 - mu^2 cancels); columns 10-11 are rgb == 1 (the gate closes),
                   columns 30-32 are rgb == 0 (on the lower bound: the gate stays open), the upper left quarter is rgb == target
  frame    48x40   the fit case of fit_cases.py: a frame of the start scene against the true scene's, background (0.1, 0.2, 0.3)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(Path(__file__).resolve().parent)):
    if p not in sys.path:
        sys.path.insert(0, p)
import loss_ref  # noqa: E402

SIZES = {"tiny": (7, 5), "tile": (16, 16), "ragged": (37, 23), "smooth": (48, 33), "flat": (48, 33), "frame": (48, 40)}   # (W, H)
NAMES = tuple(SIZES)
LAMBDAS = (0.2, 1.0)
BACKGROUND = (0.1, 0.2, 0.3)
FIGURES = ("loss", "l1", "ssim", "mse", "g_plain", "g_rgb", "g_alpha")
# fit_cases' fit case descending (1 - 0.2) L1 + 0.2 (1 - SSIM) on the float64 stand-in (tests/test_loss_cpu.py prints it): the combined
# loss over all views goes 4.8771e-02 -> 2.6620e-03.  Both fit tests assert half again above this fraction.
FIT_LAMBDA = 0.2
FIT_DSSIM_RATIO = 0.0546

# The float32 restatement (loss_ref.evaluate(dtype=np.float32)) against the float64 definition, per (case, masked, lambda): the four
# terms relative to the reference's value; the plain gradient, the prechained one and g_alpha as max |g - g_ref| / max |g_ref|
# (float32_errors below; tests/test_loss_cpu.py holds the table to it).  The GPU test's bounds are four times these.
F32_ERR = {
    ('tiny', False, 0.2): dict(loss=1.35e-08, l1=1.78e-08, ssim=3.67e-08, mse=3.61e-08, g_plain=8.36e-08, g_rgb=8.36e-08, g_alpha=8.87e-08),
    ('tiny', False, 1.0): dict(loss=3.90e-08, l1=1.78e-08, ssim=3.67e-08, mse=3.61e-08, g_plain=1.03e-07, g_rgb=1.03e-07, g_alpha=1.05e-07),
    ('tiny', True, 0.2): dict(loss=3.66e-08, l1=6.84e-08, ssim=4.37e-08, mse=3.41e-08, g_plain=1.40e-07, g_rgb=1.40e-07, g_alpha=9.66e-08),
    ('tiny', True, 1.0): dict(loss=4.38e-08, l1=6.84e-08, ssim=4.37e-08, mse=3.41e-08, g_plain=2.08e-07, g_rgb=2.08e-07, g_alpha=1.55e-07),
    ('tile', False, 0.2): dict(loss=1.28e-08, l1=2.53e-08, ssim=9.13e-08, mse=3.20e-08, g_plain=3.38e-07, g_rgb=3.38e-07, g_alpha=2.26e-07),
    ('tile', False, 1.0): dict(loss=3.05e-08, l1=2.53e-08, ssim=9.13e-08, mse=3.20e-08, g_plain=5.53e-07, g_rgb=5.53e-07, g_alpha=5.00e-07),
    ('tile', True, 0.2): dict(loss=1.27e-08, l1=2.10e-08, ssim=2.20e-08, mse=2.04e-08, g_plain=3.16e-07, g_rgb=3.16e-07, g_alpha=1.58e-07),
    ('tile', True, 1.0): dict(loss=6.46e-09, l1=2.10e-08, ssim=2.20e-08, mse=2.04e-08, g_plain=5.78e-07, g_rgb=5.78e-07, g_alpha=3.81e-07),
    ('ragged', False, 0.2): dict(loss=2.41e-08, l1=7.25e-08, ssim=1.02e-07, mse=7.93e-08, g_plain=3.26e-07, g_rgb=3.26e-07, g_alpha=2.10e-07),
    ('ragged', False, 1.0): dict(loss=1.87e-08, l1=7.25e-08, ssim=1.02e-07, mse=7.93e-08, g_plain=4.77e-07, g_rgb=4.77e-07, g_alpha=3.35e-07),
    ('ragged', True, 0.2): dict(loss=1.73e-09, l1=8.63e-08, ssim=8.45e-08, mse=4.12e-08, g_plain=3.01e-07, g_rgb=3.01e-07, g_alpha=1.89e-07),
    ('ragged', True, 1.0): dict(loss=3.14e-08, l1=8.63e-08, ssim=8.45e-08, mse=4.12e-08, g_plain=4.77e-07, g_rgb=4.77e-07, g_alpha=2.57e-07),
    ('smooth', False, 0.2): dict(loss=3.47e-08, l1=3.51e-08, ssim=1.39e-08, mse=1.28e-08, g_plain=6.74e-06, g_rgb=6.74e-06, g_alpha=4.68e-06),
    ('smooth', False, 1.0): dict(loss=8.76e-08, l1=3.51e-08, ssim=1.39e-08, mse=1.28e-08, g_plain=7.92e-06, g_rgb=7.92e-06, g_alpha=5.95e-06),
    ('smooth', True, 0.2): dict(loss=1.30e-07, l1=4.52e-08, ssim=6.07e-08, mse=5.75e-09, g_plain=8.61e-06, g_rgb=8.61e-06, g_alpha=4.17e-06),
    ('smooth', True, 1.0): dict(loss=3.83e-07, l1=4.52e-08, ssim=6.07e-08, mse=5.75e-09, g_plain=1.06e-05, g_rgb=1.06e-05, g_alpha=5.61e-06),
    ('flat', False, 0.2): dict(loss=6.28e-06, l1=3.85e-08, ssim=6.36e-06, mse=4.02e-08, g_plain=6.03e-05, g_rgb=6.03e-05, g_alpha=6.03e-05),
    ('flat', False, 1.0): dict(loss=1.06e-05, l1=3.85e-08, ssim=6.36e-06, mse=4.02e-08, g_plain=7.01e-05, g_rgb=7.01e-05, g_alpha=7.01e-05),
    ('flat', True, 0.2): dict(loss=5.62e-06, l1=2.93e-08, ssim=5.53e-06, mse=3.10e-08, g_plain=5.91e-05, g_rgb=5.91e-05, g_alpha=5.91e-05),
    ('flat', True, 1.0): dict(loss=9.58e-06, l1=2.93e-08, ssim=5.53e-06, mse=3.10e-08, g_plain=7.11e-05, g_rgb=7.11e-05, g_alpha=7.11e-05),
    ('frame', False, 0.2): dict(loss=4.22e-07, l1=5.23e-09, ssim=8.13e-08, mse=5.83e-08, g_plain=5.91e-06, g_rgb=5.91e-06, g_alpha=5.77e-06),
    ('frame', False, 1.0): dict(loss=9.50e-07, l1=5.23e-09, ssim=8.13e-08, mse=5.83e-08, g_plain=6.37e-06, g_rgb=6.37e-06, g_alpha=6.70e-06),
    ('frame', True, 0.2): dict(loss=3.86e-07, l1=2.36e-08, ssim=8.22e-08, mse=3.29e-08, g_plain=7.66e-06, g_rgb=7.66e-06, g_alpha=6.65e-06),
    ('frame', True, 1.0): dict(loss=9.60e-07, l1=2.36e-08, ssim=8.22e-08, mse=3.29e-08, g_plain=8.51e-06, g_rgb=8.51e-06, g_alpha=6.87e-06),
}


def _seed(name):
    return 300 + NAMES.index(name)


_CASES = {}


def _frame():
    import fit_cases as fc
    true, start, V, K, W, H = fc.fit_case()
    x = fc.RefRenderer(start).render(V[0], K[0], W, H, BACKGROUND)["rgb"].detach().numpy()
    y = fc.RefRenderer(true).render(V[0], K[0], W, H, BACKGROUND)["rgb"].detach().numpy()
    return x.astype(np.float32), y.astype(np.float32)


def case(name):
    """(rgb [H,W,3], target [H,W,3]) float32, drawn once."""
    if name in _CASES:
        return _CASES[name]
    W, H = SIZES[name]
    rng = np.random.default_rng(_seed(name))
    if name in ("tiny", "tile", "ragged"):
        x, y = rng.random((H, W, 3)), rng.random((H, W, 3))
    elif name == "smooth":
        v, u = np.mgrid[0:H, 0:W]
        y = np.stack([0.5 + 0.4 * np.sin(0.21 * u + 0.5 * c) * np.cos(0.17 * v - 0.3 * c) for c in range(3)], axis=-1)
        x = np.clip(y + rng.normal(0.0, 0.05, y.shape), 0.0, 0.999)
    elif name == "flat":
        x, y = np.full((H, W, 3), 0.5), np.full((H, W, 3), 0.5)
        y[:, W // 2:] = 0.52
        x[H // 2:, :W // 2] = 0.51
        x[:, 10:12] = 1.0
        x[:, 30:33] = 0.0
    elif name == "frame":
        x, y = _frame()
    _CASES[name] = (np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32))
    return _CASES[name]


def mask(name):
    """[H,W] bool, about 30 % False."""
    W, H = SIZES[name]
    return np.random.default_rng(1000 + _seed(name)).random((H, W)) > 0.3


_REF = {}


def reference(name, masked, lam, prechained, dtype=np.float64):
    """loss_ref.evaluate of the case (computed once, never changed)."""
    key = (name, bool(masked), float(lam), bool(prechained), np.dtype(dtype).name)
    if key not in _REF:
        x, y = case(name)
        _REF[key] = loss_ref.evaluate(x, y, mask(name) if masked else None, lam, BACKGROUND if prechained else None, dtype)
    return _REF[key]


def errors(got_plain, got_pre, name, masked, lam):
    """The FIGURES of results (dicts as loss_ref.evaluate's, the plain and the prechained form) against the float64 reference."""
    ref_plain, ref_pre = reference(name, masked, lam, False), reference(name, masked, lam, True)
    out = {}
    for k, t in enumerate(("loss", "l1", "ssim", "mse")):
        a, b = float(np.asarray(got_pre["terms"], np.float64)[k]), float(ref_pre["terms"][k])
        out[t] = abs(a - b) / abs(b) if b != 0 else abs(a - b)
    out["g_plain"] = loss_ref.rel_err(got_plain["g_rgb"], ref_plain["g_rgb"])
    out["g_rgb"] = loss_ref.rel_err(got_pre["g_rgb"], ref_pre["g_rgb"])
    out["g_alpha"] = loss_ref.rel_err(got_pre["g_alpha"], ref_pre["g_alpha"])
    return out


def float32_errors(name, masked, lam):
    return errors(reference(name, masked, lam, False, np.float32), reference(name, masked, lam, True, np.float32), name, masked, lam)


def keys():
    return [(n, m, lam) for n in NAMES for m in (False, True) for lam in LAMBDAS]


if __name__ == "__main__":
    print("F32_ERR = {")
    for key in keys():
        print(f"    {key!r}: dict(" + ", ".join(f"{k}={v:.2e}" for k, v in float32_errors(*key).items()) + "),")
    print("}")
