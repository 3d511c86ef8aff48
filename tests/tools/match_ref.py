"""NumPy reference of point matching (sas_match_points; DESIGN.md 3, "Point matching") and of the ICP loop around it.

``match32`` restates the contract in float32 with the kernel's operation order -- p' = ((A_k0 x + A_k1 y) + A_k2 z) + t_k, d2 =
((dx dx + dy dy) + dz dz) with d = q - p', the minimum of the key (bits(d2) << 32 | j) over the targets whose d2 is < inf, the match
held when d2 <= max_distance^2 -- by blockwise brute force: the GPU is bit-equal to it.  ``match64`` is the same in float64 with
nothing rounded: the reference for what float32 costs.  Both have ``Rasterizer.match_points``' signature and result (host arrays),
so either is a ``matcher`` of ``register.register_similarity`` and of ``icp`` below, an independent restatement of that loop.
"""
from __future__ import annotations

import numpy as np

NONE_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
BLOCK = 128   # source points per brute-force block


def _affine(transform, dtype):
    """(A [3,3], t [3]) of a 4x4 / 3x4 transform (None: identity), rounded once to ``dtype``."""
    T = np.eye(4)[:3] if transform is None else np.asarray(transform, np.float64).reshape(-1, 4)[:3]
    T = T.astype(dtype)
    return T[:, :3], T[:, 3]


def moved(source, transform, dtype):
    """p' = A p + t in ``dtype`` with the contract's order: ((A_k0 x + A_k1 y) + A_k2 z) + t_k."""
    p = np.asarray(source, dtype).reshape(-1, 3)
    A, t = _affine(transform, dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((A[k, 0] * x + A[k, 1] * y) + A[k, 2] * z) + t[k] for k in range(3)], axis=1)


def moments64(p, q, d2, index) -> np.ndarray:
    """The 18 moments over the held matches (index >= 0), float64, from ``p' [S,3]``, ``q [T,3]`` and ``d2 [S]`` widened: n, sum p'
    (3), sum q (3), sum q p'^T (9, row-major), sum |p'|^2, sum d2 (``moment_bound``: what a sum in another order may differ by)."""
    return _moment_terms(p, q, d2, index).sum(axis=0)


def _moment_terms(p, q, d2, index) -> np.ndarray:
    held = np.asarray(index) >= 0
    P = np.asarray(p, np.float64).reshape(-1, 3)[held]
    Q = np.asarray(q, np.float64).reshape(-1, 3)[np.asarray(index)[held]]
    D = np.asarray(d2, np.float64).reshape(-1)[held]
    return np.concatenate([np.ones((len(P), 1)), P, Q, (Q[:, :, None] * P[:, None, :]).reshape(-1, 9),
                           ((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])[:, None], D[:, None]], axis=1)


def moment_bound(p, q, d2, index) -> np.ndarray:
    """Per moment ``n eps64 sum |term|``: the classic bound of a floating-point sum of n terms in ANY order (each of the n - 1
    additions errs by at most eps64 / 2 of a partial sum that is at most sum |term|; the products err by eps64 / 2 each)."""
    terms = _moment_terms(p, q, d2, index)
    return max(len(terms), 1) * float(np.finfo(np.float64).eps) * np.abs(terms).sum(axis=0)


def _match(source, target, transform, max_distance, dtype):
    dtype = np.dtype(dtype).type
    q = np.asarray(target, dtype).reshape(-1, 3)
    p = moved(source, transform, dtype)
    S, T = len(p), len(q)
    index = np.full(S, -1, np.int32)
    dist2 = np.full(S, np.inf, dtype)
    j = np.arange(T, dtype=np.uint64)
    with np.errstate(all="ignore"):
        md2 = dtype(max_distance) * dtype(max_distance)
        for s0 in range(0, S if T else 0, BLOCK):
            pb = p[s0:s0 + BLOCK]
            dx, dy, dz = (q[None, :, k] - pb[:, None, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = d2 < np.inf                                          # (false for a NaN)
            if dtype is np.float32:
                key = np.where(ok, (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j[None, :], NONE_KEY)
                best = key.argmin(axis=1)
            else:                                                      # float64: the same order, the first of equal minima
                best = np.where(ok, d2, np.inf).argmin(axis=1)
            b2 = d2[np.arange(len(pb)), best]
            held = ok[np.arange(len(pb)), best] & (b2 <= md2)
            index[s0:s0 + BLOCK] = np.where(held, best, -1)
            dist2[s0:s0 + BLOCK] = np.where(held, b2, np.inf)
    return {"index": index, "dist2": dist2, "moments": moments64(p, q, np.where(index >= 0, dist2, 0), index), "moved": p}


def match32(source, target, transform=None, max_distance=np.inf, slices=None):
    """The contract in float32 (source, target and transform rounded once): what the GPU returns, bit for bit in ``index`` and
    ``dist2``.  ``moved`` is p' (float32)."""
    return _match(source, target, transform, max_distance, np.float32)


def match64(source, target, transform=None, max_distance=np.inf, slices=None):
    """The same in float64, nothing rounded."""
    return _match(source, target, transform, max_distance, np.float64)


def umeyama(moments, with_scaling=True) -> np.ndarray:
    """Similarity from the moments, restated: centred cross-covariance, SVD, reflection fix, scale tr(D S) / var(p')."""
    m = np.asarray(moments, np.float64)
    n = m[0]
    if n < 3:
        raise ValueError("fewer than 3 matches")
    mp, mq = m[1:4] / n, m[4:7] / n
    cov = m[7:16].reshape(3, 3) / n - mq[:, None] * mp[None, :]
    var = m[16] / n - mp @ mp
    U, D, Vt = np.linalg.svd(cov)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U @ Vt) < 0 else 1.0])
    R = U @ S @ Vt
    c = np.trace(np.diag(D) @ S) / var if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mq - c * R @ mp
    return T


def icp(source, target, init, matcher, max_distance=0.2, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, with_scaling=True):
    """The registration loop restated: evaluate; per iteration T <- umeyama . T, evaluate; stop when |d fitness| and |d rmse| are
    both under their limits.  Returns ``{"T", "fitness", "rmse", "iterations", "transforms", "matches"}``: ``transforms[k]`` is the
    float64 T of evaluation k (0: init) and ``matches[k]`` the matcher's result for it."""
    src = np.asarray(source, np.float32).reshape(-1, 3)
    tgt = np.asarray(target, np.float32).reshape(-1, 3)
    T = np.array(init, np.float64).reshape(4, 4)

    def evaluate(T):
        r = matcher(src, tgt, transform=T, max_distance=max_distance)
        n = r["moments"][0]
        return r, n / len(src), (np.sqrt(r["moments"][17] / n) if n > 0 else 0.0)

    r, fit, rmse = evaluate(T)
    transforms, matches, it = [T.copy()], [r], 0
    while it < max_iteration:
        T = umeyama(r["moments"], with_scaling) @ T
        it += 1
        old = (fit, rmse)
        r, fit, rmse = evaluate(T)
        transforms.append(T.copy())
        matches.append(r)
        if abs(old[0] - fit) < relative_fitness and abs(old[1] - rmse) < relative_rmse:
            break
    return {"T": T, "fitness": fit, "rmse": rmse, "iterations": it, "transforms": transforms, "matches": matches}
