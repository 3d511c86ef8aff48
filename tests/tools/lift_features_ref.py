"""The reference of feature lifting (sas_lift_features; DESIGN.md 3, "Feature lifting"), from code that predates it.

The weight image of Gaussian i, vis_i(p), comes from lift_ref: the C oracle's one-hot frames (weights_oracle) or, beyond a couple of
hundred Gaussians, render_features with explicit one-hot features (weights_features).  From it, in numpy:

    q24[i,p]  = floor(vis_i(p) * 2^24)                                           (exact in float32 and in float64)
    fq[p,k]   = rint(min(max(float32(f[p,k]) * float32(scale), -32767), 32767))  (the float32 product; half to even; NaN -> 0)
    sums      = q24 @ (fq * mask)          weight = q24 @ mask                   (int64)

Nothing here calls lift_features or semantics.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lift_ref as lr  # noqa: E402

ONE = 2 ** 24
FQ_MAX = 32767


def quantise_weights(w):
    """floor(vis * 2^24) as int64."""
    w = np.asarray(w)
    assert w.dtype == np.float32 and (w >= 0).all() and (w < 1).all()
    return np.floor(w.astype(np.float64) * float(ONE)).astype(np.int64)


def quantise_features(f, scale):
    """fq as int64: the float32 product clamped to +-32767 and rounded half to even; NaN -> 0, +-Inf -> +-32767."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.asarray(f, np.float32) * np.float32(scale)
    assert y.dtype == np.float32
    y = np.where(np.isnan(y), np.float32(0.0), np.minimum(np.maximum(y, np.float32(-FQ_MAX)), np.float32(FQ_MAX)))
    return np.rint(y).astype(np.int64)


def auto_scale(images):
    """32767 / max|finite f| (1 if all are zero), as a float32's value."""
    f = np.asarray(images, np.float32)
    f = np.abs(f[np.isfinite(f)])
    top = float(f.max()) if f.size else 0.0
    return float(np.float32(FQ_MAX / top if top > 0.0 else 1.0))


def sums(weights, image, scale, mask=None):
    """(sums [N,C], weight [N]) int64 of ONE view: ``weights [N,H,W]`` float32, ``image [H,W,C]``, ``mask [H,W]`` or None."""
    q = quantise_weights(weights).reshape(len(weights), -1)
    fq = quantise_features(np.asarray(image).reshape(q.shape[1], -1), scale)
    keep = np.ones(q.shape[1], np.int64) if mask is None else (np.asarray(mask).reshape(-1) != 0).astype(np.int64)
    return q @ (fq * keep[:, None]), q @ keep


def reference(sc, cam, image, scale, mask=None, Rt=None, rasterizer=None):
    """(sums, weight) of one view; the oracle's weights up to lift_ref.ORACLE_MAX Gaussians, else the feature path's."""
    if len(sc["means"]) <= lr.ORACLE_MAX:
        w = lr.weights_oracle(sc, cam, Rt)
    else:
        assert rasterizer is not None, "scenes beyond ORACLE_MAX Gaussians need a Rasterizer for the feature path"
        w = lr.weights_features(rasterizer, sc, cam, Rt)
    return sums(w, image, scale, mask)


def float_mean(weights, image, mask=None):
    """(mean [N,C], w [N], n [N]) in float64: sum vis f / sum vis over the contributing pixels (vis > 0, mask != 0), their weight
    sum and their number.  NaN where w == 0."""
    w = np.asarray(weights, np.float64).reshape(len(weights), -1)
    f = np.asarray(image, np.float64).reshape(w.shape[1], -1)
    if mask is not None:
        w = w * (np.asarray(mask).reshape(-1) != 0)
    tot = w.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (w @ f) / tot[:, None], tot, (w > 0).sum(axis=1)
