"""NumPy reference of the point-to-mesh query (sas_query_meshes; DESIGN.md 3, "Mesh queries"): one evaluation of the definitions,
parameterised by dtype.  float64 is the reference; float32 -- the same operations, the solid angles summed sequentially in triangle
order -- is the yardstick for what float32 can deliver.  Points and vertices are rounded to float32 first: what the GPU is handed.

Per triangle (A, B, C) and point p, with a, b, c the vertices minus p and e1 = B - A, e2 = C - A, e3 = C - B:
  distance^2 = min over the three edges as segments, and, where n = e1 x e2 is not zero and p projects into the triangle
               (n . (a x e1), n . (b x e3), n . (e2 x c) all >= 0), of (n . a)^2 / (n . n);
  Omega / 2  = atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|), 0 for a triangle with n = 0;
  winding    = sum_k (Omega_k / 2) / (2 pi).
"""
from __future__ import annotations

import numpy as np


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _segment_d2(a, e, dtype):
    """Squared distance from the origin to the segment from ``a [3][N]`` along ``e [3]`` (scalars)."""
    len2 = _dot(e, e)
    if len2 > 0:
        t = np.clip(-_dot(a, e) / len2, dtype(0), dtype(1))
    else:
        t = np.zeros_like(a[0])
    q = (a[0] + t * e[0], a[1] + t * e[1], a[2] + t * e[2])
    return _dot(q, q)


def kept_faces(vertices, faces) -> np.ndarray:
    """The faces whose three vertices are finite (in float32)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return f[np.isfinite(v[f]).all(axis=(1, 2))] if len(f) else f


def query_mesh(points, vertices, faces, dtype=np.float64):
    """(distance [N], winding [N]) of one mesh, no culling; a mesh without a kept face reads (+inf, 0)."""
    dtype = np.dtype(dtype).type
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(dtype)
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(dtype)
    best = np.full(len(p), np.inf, dtype)
    total = np.zeros(len(p), dtype)
    px = (p[:, 0], p[:, 1], p[:, 2])
    with np.errstate(all="ignore"):
        for i0, i1, i2 in kept_faces(vertices, faces):
            A, B, C = v[i0], v[i1], v[i2]
            a = tuple(A[k] - px[k] for k in range(3))
            b = tuple(B[k] - px[k] for k in range(3))
            c = tuple(C[k] - px[k] for k in range(3))
            e1, e2, e3 = tuple(B - A), tuple(C - A), tuple(C - B)
            d2 = np.minimum(np.minimum(_segment_d2(a, e1, dtype), _segment_d2(b, e3, dtype)), _segment_d2(a, e2, dtype))
            n = _cross(e1, e2)
            nn = _dot(n, n)
            if nn > 0:
                s1, s2, s3 = _dot(n, _cross(a, e1)), _dot(n, _cross(b, e3)), _dot(n, _cross(e2, c))
                h = _dot(n, a)
                d2 = np.where((s1 >= 0) & (s2 >= 0) & (s3 >= 0), np.minimum(d2, h * h / nn), d2)
                la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
                num = _dot(a, _cross(b, c))
                den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
                om = np.arctan2(num, den)
                total = total + np.where(np.isfinite(om), om, dtype(0))
            best = np.fmin(best, d2)
    return np.sqrt(best), total * dtype(0.15915494309189535)


def culled(points, vertices, faces, max_distance) -> np.ndarray:
    """bool [N], the box rule in float32: outside the box of the kept faces' vertices inflated by ``max_distance`` (p < lo - md or
    p > hi + md on some axis), a mesh without a kept face, or a point with a non-finite coordinate."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = kept_faces(vertices, faces)
    if len(f) == 0:
        return np.ones(len(p), bool)
    used = v[f.reshape(-1)]
    md = np.float32(max_distance)
    with np.errstate(all="ignore"):
        lo, hi = used.min(axis=0) - md, used.max(axis=0) + md
        outside = ((p < lo) | (p > hi)).any(axis=1)
    return outside | ~np.isfinite(p).all(axis=1)


def query(points, meshes, max_distance=np.inf, dtype=np.float64):
    """``{"distance": [M,N], "winding": [M,N], "culled": bool [M,N]}`` of ``meshes = [(vertices, faces), ...]``: culled pairs read
    +inf / 0, as the library writes them."""
    dist, wind, cull = [], [], []
    for v, f in meshes:
        c = culled(points, v, f, max_distance)
        d, w = query_mesh(points, v, f, dtype)
        dist.append(np.where(c, np.inf, d))
        wind.append(np.where(c, 0, w))
        cull.append(c)
    return {"distance": np.stack(dist), "winding": np.stack(wind), "culled": np.stack(cull)}


def link_masks(points, meshes, distance=0.015, dtype=np.float64):
    """The mask rule of the segmentation step per mesh, bool [M,N]: winding > 0.5 or distance < ``distance`` (queried with
    ``max_distance = distance``: culling never changes a decision, a culled point is further than that and outside)."""
    r = query(points, meshes, distance, dtype)
    return (r["winding"] > 0.5) | (r["distance"] < distance)
