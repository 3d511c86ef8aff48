"""Per-Gaussian embeddings from feature images, and what is asked of them: mean features from the integer sums of
``Rasterizer.lift_features``, LERF-style relevancy against query embeddings, and per-Gaussian masks from relevancy in the
``{name: bool[N]}`` form ``SplatHandler.from_arrays`` takes.

The lifting is the hot path (HIP: sas_lift_features).  What follows it is small dense algebra on ``[N,D]`` tensors -- an
``N x D . D x (P+Q)`` product and a softmax -- and runs in plain torch on the embeddings' device.  No feature extractor and no
text encoder ship here: the feature images and the query embeddings are the caller's.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .rasterizer import _host

SLAB = 256   # channels per call of Rasterizer.lift_features (SAS_MAX_FEATURES)
WEIGHT_LIMIT = 2 ** 48   # below it no sum can have overflowed: |sums[i,k]| <= 32767 weight[i] < 2^63


def lift_feature_views(rasterizer, viewmats, Ks, W: int, H: int, images, feature_scale: float, mask=None,
                       views_per_call: int = 8) -> Dict[str, object]:
    """``Rasterizer.lift_features`` over any number of views, ``views_per_call`` at a time, and any number of channels, in slabs
    of 256: returns ``{"sums": int64 [N,D], "weight": int64 [N], "feature_scale": float}`` (device tensors).  ``viewmats
    [C,4,4]``, ``Ks [C,3,3]``, ``images [C,H,W,D]`` float32 (an array, a tensor, or a sequence of ``[H,W,D]`` images), ``mask
    [C,H,W]`` or None.  ``feature_scale`` is required: every call of the loop has to quantise alike (``32767 / max|f|`` over ALL
    the images uses the whole range).  Only the first slab adds ``weight``.  Integer sums: the result does not depend on
    ``views_per_call``."""
    V = np.asarray(_host(viewmats), np.float32).reshape(-1, 4, 4)
    K = np.asarray(_host(Ks), np.float32).reshape(-1, 3, 3)
    C = V.shape[0]
    if K.shape[0] != C or len(images) != C or (mask is not None and len(mask) != C):
        raise ValueError(f"{C} view matrices, {K.shape[0]} intrinsics, {len(images)} feature images"
                         + (f", {len(mask)} masks" if mask is not None else ""))
    if C == 0 or views_per_call < 1:
        raise ValueError("lift_feature_views needs at least one view and views_per_call >= 1")
    if feature_scale is None or not np.isfinite(float(feature_scale)) or float(feature_scale) <= 0.0:
        raise ValueError("lift_feature_views needs one finite feature_scale > 0 for all of its calls")

    def batch(seq, a, b, dtype):
        part = seq[a:b]
        if not hasattr(part, "shape"):   # a sequence of images
            part = np.stack([np.asarray(_host(x), dtype) for x in part])
        return part

    D = int(batch(images, 0, 1, np.float32).shape[-1])
    slabs = [(c, min(D, c + SLAB)) for c in range(0, D, SLAB)]
    weight, parts = None, [None] * len(slabs)
    for a in range(0, C, int(views_per_call)):
        b = min(C, a + int(views_per_call))
        img = batch(images, a, b, np.float32)
        if img.shape[-1] != D:
            raise ValueError(f"feature images of {D} and of {img.shape[-1]} channels")
        m = batch(mask, a, b, np.uint8) if mask is not None else None
        for k, (c0, c1) in enumerate(slabs):
            part = img if len(slabs) == 1 else img[..., c0:c1]
            out = rasterizer.lift_features(V[a:b], K[a:b], W, H, part, feature_scale=float(feature_scale), mask=m, sums=parts[k],
                                           weight=weight if k == 0 else False)
            parts[k] = out["sums"]
            if k == 0:
                weight = out["weight"]
            scale = out["feature_scale"]
    return {"sums": parts[0] if len(parts) == 1 else torch.cat(parts, dim=1), "weight": weight, "feature_scale": scale}


def features_from_sums(sums, weight, feature_scale: float, min_weight: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(features float32 [N,D], seen bool [N])`` from the sums of ``lift_features``: ``sums / (weight * feature_scale)``, the
    compositing-weighted mean of the pixels' features, where ``weight > min_weight``; 0 where the Gaussian was not seen.  Raises
    ``OverflowError`` if ``weight.max() >= 2**48``: below that, ``|sums| <= 32767 * weight < 2**63`` cannot have wrapped."""
    s = torch.as_tensor(sums)
    w = torch.as_tensor(weight).to(s.device)
    if s.dim() != 2 or w.shape != (s.shape[0],) or s.dtype != torch.int64 or w.dtype != torch.int64:
        raise ValueError(f"sums must be int64 [N,D] and weight int64 [N], got {tuple(s.shape)} {s.dtype} and {tuple(w.shape)} {w.dtype}")
    if not (float(feature_scale) > 0.0) or not np.isfinite(float(feature_scale)):
        raise ValueError("feature_scale must be finite and > 0")
    if w.numel() and (int(w.max()) >= WEIGHT_LIMIT or int(w.min()) < 0):
        raise OverflowError(f"lift_features: a weight of {int(w.max())} (>= 2**48, or negative) no longer bounds the sums; lift fewer views "
                            "into one buffer")
    seen = w > max(int(min_weight), 0)
    den = torch.where(seen, w, torch.ones_like(w)).to(torch.float64) * float(feature_scale)
    f = (s.to(torch.float64) / den[:, None]).to(torch.float32)
    return torch.where(seen[:, None], f, torch.zeros_like(f)), seen


def _rows(x, name: str, D: Optional[int], device, dtype) -> torch.Tensor:
    t = torch.as_tensor(x).to(device=device, dtype=dtype)
    t = t.reshape(1, -1) if t.dim() == 1 else t
    if t.dim() != 2 or (D is not None and t.shape[1] != D):
        raise ValueError(f"{name} must be [*,{D}], got {tuple(t.shape)}")
    return t


def relevancy(embeds, positives, negatives, temperature: float = 10.0) -> torch.Tensor:
    """LERF's relevancy of ``embeds [N,D]`` to ``positives [P,D]`` against ``negatives [Q,D]`` (``Q >= 1``), ``[N,P]`` in 0..1:
    rows are L2-normalised (a zero row stays zero), and ``relevancy[:, j] = min_k softmax(temperature * [e.p_j, e.n_k])[0]``:
    the least probability the positive query wins against any one negative (canonical negatives: "object", "things", "stuff",
    "texture").  0.5 means "as much as the worst negative".  Plain torch on the embeddings' device."""
    e = torch.as_tensor(embeds)
    if e.dim() != 2:
        raise ValueError(f"embeds must be [N,D], got {tuple(e.shape)}")
    dtype = e.dtype if e.dtype in (torch.float32, torch.float64) else torch.float32
    e = e.to(dtype)
    p = _rows(positives, "positives", e.shape[1], e.device, dtype)
    n = _rows(negatives, "negatives", e.shape[1], e.device, dtype)
    if n.shape[0] < 1 or p.shape[0] < 1:
        raise ValueError("relevancy needs at least one positive and one negative query")

    def unit(x):
        return x / x.norm(dim=1, keepdim=True).clamp_min(torch.finfo(dtype).tiny)

    e, p, n = unit(e), unit(p), unit(n)
    sp = float(temperature) * (e @ p.T)            # [N,P]
    sn = float(temperature) * (e @ n.T)            # [N,Q]
    # softmax([a, b])[0] = sigmoid(a - b); the minimum over the negatives is at the largest b
    return torch.sigmoid(sp - sn.max(dim=1, keepdim=True).values)


def masks_from_relevancy(rel, names: Sequence[str], threshold: float = 0.5, seen=None) -> Dict[str, np.ndarray]:
    """Disjoint ``{name: bool[N]}`` from ``rel [N,P]``: a Gaussian goes to the LOWEST ``j`` that attains its row's maximum, and
    only if that maximum is ``>= threshold`` (and, with ``seen [N]``, only if it was seen).  The form ``SplatHandler.from_arrays``
    takes."""
    r = np.asarray(_host(rel), np.float64)
    names = list(names)
    if r.ndim != 2 or r.shape[1] != len(names):
        raise ValueError(f"rel must be [N,{len(names)}], got {r.shape}")
    if len(set(names)) != len(names):
        raise ValueError("mask names must be distinct")
    if not names:
        return {}
    arg = r.argmax(axis=1)   # (the first index of the maximum)
    own = r[np.arange(len(r)), arg] >= float(threshold)
    if seen is not None:
        s = np.asarray(_host(seen)).astype(bool).reshape(-1)
        if s.shape[0] != len(r):
            raise ValueError(f"seen must be [{len(r)}], got {s.shape}")
        own &= s
    return {name: own & (arg == j) for j, name in enumerate(names)}
