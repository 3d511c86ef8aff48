"""The yardstick of the optimiser step ("Optimiser step"): sas_scene_adam_step restated in numpy -- float64 for the
reference, float32 (``dtype``) to measure what float32 arithmetic alone costs.

State of a scene: the activated arrays ``x`` (means, opacities, colors [n,K,3], quats, scales -- what the planes hold), and per group
that has been stepped the moments ``m``, ``v`` and, for opacities and scales, the raw values ``raw`` = logit / log, taken from ``x``
the first time the group is stepped.  One ``step``:

- a group whose gradient is None or whose learning rate is 0 is left alone and gets no state (colors: both of sh_dc and sh_rest 0);
  an element of colors whose own rate is 0 is left alone too,
- the gradient is chained through the activation with the RESIDENT activated value: d_logit = d_o o (1 - o), d_logscale = d_s s,
- an element whose chained gradient is not finite keeps its variable and moments,
- an opacity outside (0, 1) and a scale that is not positive and finite have raw = NaN for good: fixed,
- ``visible_only``: a Gaussian whose gradient is exactly zero in every stepped array is skipped whole,
- Adam with bias correction from the 1-based step ``t``; the hyper-parameters are the float32 values the C ABI carries, the bias
  corrections 1 - beta^t are formed in float64 and rounded once to ``dtype``.

exp and log of the float32 restatement are the float64 functions rounded to float32 (the same on every host)."""
import numpy as np

GROUPS = ("means", "opacities", "colors", "quats", "scales")
LR_KEYS = ("means", "opacities", "sh_dc", "sh_rest", "quats", "scales")


def _exp(a, dt):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(a.astype(np.float64)).astype(dt)


def _log(a, dt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(a.astype(np.float64)).astype(dt)


def new_state(scene, dtype=np.float64):
    """``scene``: means [n,3], opacities [n], colors [n,K,3] and quats [n,4] + scales [n,3] (absent or None: a cov6 scene)."""
    dt = np.dtype(dtype).type
    x = {k: np.asarray(scene[k], np.float32).astype(dt) for k in GROUPS if scene.get(k) is not None}
    n = x["means"].shape[0]
    x["colors"] = x["colors"].reshape(n, -1, 3)
    return dict(x=x, m={}, v={}, raw={}, dt=dt, n=n)


def inverse_activation(k, x, dt):
    """raw values of group ``k`` from its activated values; NaN outside the domain."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if k == "opacities":
            ok = (x > 0) & (x < 1)
            return np.where(ok, _log(np.where(ok, x, dt(0.5)) / (dt(1) - np.where(ok, x, dt(0.5))), dt), dt(np.nan)).astype(dt)
        ok = (x > 0) & np.isfinite(x)
        return np.where(ok, _log(np.where(ok, x, dt(1)), dt), dt(np.nan)).astype(dt)


def _rates(k, lrs, shape, dt):
    h = lambda v: dt(np.float32(v))
    if k == "colors":
        lr = np.full(shape, h(lrs.get("sh_rest", 0.0)), dt)
        lr[:, 0, :] = h(lrs.get("sh_dc", 0.0))
        return lr
    return np.full(shape, h(lrs.get(k, 0.0)), dt)


def step(S, grads, lrs, t, betas=(0.9, 0.999), eps=1e-15, visible_only=False):
    """Advance ``S`` in place by one step; returns it."""
    dt, n = S["dt"], S["n"]
    h = lambda v: dt(np.float32(v))
    b1, b2, ep = h(betas[0]), h(betas[1]), h(eps)
    bc1 = dt(1.0 - float(np.float32(betas[0])) ** int(t))
    bc2 = dt(1.0 - float(np.float32(betas[1])) ** int(t))
    active = {}
    for k in GROUPS:
        g = grads.get(k)
        if g is None or k not in S["x"]:
            continue
        lr = _rates(k, lrs, S["x"][k].shape, dt)
        if not (lr > 0).any():
            continue
        active[k] = (np.asarray(g, np.float32).astype(dt).reshape(S["x"][k].shape), lr)
    skip = np.zeros(n, bool)
    if visible_only and active:
        skip = np.all([np.all(g.reshape(n, -1) == 0, axis=1) for g, _ in active.values()], axis=0)
    for k, (g, lr) in active.items():
        x = S["x"][k]
        if k not in S["m"]:
            S["m"][k], S["v"][k] = np.zeros_like(x), np.zeros_like(x)
            if k in ("opacities", "scales"):
                S["raw"][k] = inverse_activation(k, x, dt)
        m, v = S["m"][k], S["v"][k]
        with np.errstate(all="ignore"):
            if k == "opacities":
                gc, var = g * (x * (dt(1) - x)), S["raw"][k]
            elif k == "scales":
                gc, var = g * x, S["raw"][k]
            else:
                gc, var = g, x
            ok = np.isfinite(gc) & (lr != 0) & ~np.isnan(var) & ~skip.reshape((n,) + (1,) * (x.ndim - 1))
            gz = np.where(ok, gc, dt(0))
            m1 = b1 * m + (dt(1) - b1) * gz
            v1 = b2 * v + (dt(1) - b2) * (gz * gz)
            new = var - (lr * (m1 / bc1)) / (np.sqrt(v1 / bc2) + ep)
            assert new.dtype == np.dtype(dt) and m1.dtype == np.dtype(dt)
            S["m"][k], S["v"][k] = np.where(ok, m1, m), np.where(ok, v1, v)
            var1 = np.where(ok, new, var)
            if k == "opacities":
                S["raw"][k] = var1
                S["x"][k] = np.where(ok, dt(1) / (dt(1) + _exp(-var1, dt)), x)
            elif k == "scales":
                S["raw"][k] = var1
                S["x"][k] = np.where(ok, _exp(var1, dt), x)
            else:
                S["x"][k] = var1
    return S


def run(scene, grads_per_step, lrs, dtype=np.float64, **kw):
    """The activated arrays after ``len(grads_per_step)`` steps from ``scene`` (step counts 1, 2, ...)."""
    S = new_state(scene, dtype)
    for t, g in enumerate(grads_per_step, start=1):
        step(S, g, lrs, t, **kw)
    return S


def rel_err(got, ref):
    """max |got - ref| / max |ref| (0 when they agree everywhere)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got.reshape(ref.shape) - ref).max() if ref.size else 0.0
    top = np.abs(ref).max() if ref.size else 0.0
    return 0.0 if d == 0.0 else d / top if top > 0 else np.inf
