"""The point-cloud contract ("Point clouds"; sas_sample_points) restated in NumPy, op for op.

``cloud32`` computes in float32 -- every NumPy operation below is one rounded IEEE operation on float32 arrays, in the contract's
order, nothing fused -- and is what the GPU tests hold the kernels to bit for bit.  ``cloud64`` is the same text in float64 (the
float32 inputs widened): on the dyadic cases of cloud_cases.py, where float32 arithmetic is exact, the two agree exactly
(tests/test_cloud_cpu.py).  ``fps_is_greedy`` checks the sampling order by brute force, without the running-minimum bookkeeping.
"""
import numpy as np


def _cloud(dtype, depth, Ks, transform, n_points, rgb8=None, labels=None, keep=None, bounds=None, voxel=0.0, stride=1, clouds=None,
           n_clouds=1):
    f = dtype
    depth = np.asarray(depth, np.float32)
    if depth.ndim == 4:
        depth = depth[..., 0]
    C, H, W = depth.shape
    K, E = int(n_points), int(n_clouds)
    Ks = np.asarray(Ks, np.float32).reshape(C, 9).astype(f)
    T = (np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (C, 1)) if transform is None else np.asarray(transform, np.float32)).reshape(C, 12).astype(f)
    clouds = np.zeros(C, np.int64) if clouds is None else np.asarray(clouds, np.int64).reshape(C)
    voxel = f(np.float32(voxel))
    lo = hi = None
    if bounds is not None:
        b = np.asarray(bounds, np.float32).reshape(6).astype(f)
        lo, hi = b[:3], b[3:]
    n = None
    if voxel > 0:
        n = np.maximum(1, np.ceil((hi - lo) / voxel).astype(np.int64))
        assert int(n[0]) * int(n[1]) * int(n[2]) <= 2 ** 24
    vs, us = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    vs, us = vs.reshape(-1), us.reshape(-1)                      # (in p order)
    cand = [dict(p=[], w=[], cell=[]) for _ in range(E)]
    for c in range(C):
        p = (c * H + vs) * W + us
        d = depth[c, vs, us].astype(f)
        with np.errstate(all="ignore"):
            ok = (d > 0) & (d < np.inf)
            if labels is not None and keep is not None:
                ok &= np.asarray(keep).reshape(256)[np.asarray(labels, np.uint8).reshape(C, H, W)[c, vs, us]] != 0
            fx, cx, fy, cy = Ks[c, 0], Ks[c, 2], Ks[c, 4], Ks[c, 5]
            x = (us.astype(f) - cx) * d / fx
            y = (vs.astype(f) - cy) * d / fy
            z = d
            A = T[c]
            w = np.stack([((A[4 * k] * x + A[4 * k + 1] * y) + A[4 * k + 2] * z) + A[4 * k + 3] for k in range(3)], axis=1)
            ok &= np.isfinite(w).all(axis=1)
            if lo is not None:
                ok &= ((lo <= w) & (w <= hi)).all(axis=1)
            cell = np.zeros(len(p), np.int64)
            if n is not None:
                i = np.minimum(np.floor((w - lo) / voxel), (n - 1).astype(f))
                i = np.where(ok[:, None], i, 0).astype(np.int64)
                cell = (i[:, 0] * n[1] + i[:, 1]) * n[2] + i[:, 2]
        e = cand[int(clouds[c])]
        e["p"].append(p[ok]); e["w"].append(w[ok]); e["cell"].append(cell[ok])
    out = dict(points=np.zeros((E, K, 3), f), index=np.full((E, K), -1, np.int32), count=np.zeros(E, np.int32), survivors=[], w=[], picks=[])
    if rgb8 is not None:
        out["colors"] = np.zeros((E, K, 3), np.uint8)
    if labels is not None:
        out["labels"] = np.full((E, K), 255, np.uint8)
    for e in range(E):
        p = np.concatenate(cand[e]["p"]) if cand[e]["p"] else np.zeros(0, np.int64)
        w = np.concatenate(cand[e]["w"]) if cand[e]["w"] else np.zeros((0, 3), f)
        cell = np.concatenate(cand[e]["cell"]) if cand[e]["cell"] else np.zeros(0, np.int64)
        order = np.argsort(p, kind="stable")                      # (views of a cloud come in view order: already sorted)
        p, w, cell = p[order], w[order], cell[order]
        if n is not None and len(p):
            _, first = np.unique(cell, return_index=True)         # the first of a cell in p order: the lowest p
            first.sort()
            p, w = p[first], w[first]
        M = len(p)
        out["count"][e] = M
        out["survivors"].append(p)
        out["w"].append(w)
        picks = fps(w, min(K, M))
        out["picks"].append(picks)
        k = len(picks)
        out["points"][e, :k] = w[picks]
        out["index"][e, :k] = p[picks]
        if rgb8 is not None:
            out["colors"][e, :k] = np.asarray(rgb8, np.uint8).reshape(-1, 3)[p[picks]]
        if labels is not None:
            out["labels"][e, :k] = np.asarray(labels, np.uint8).reshape(-1)[p[picks]]
    return out


def fps(w, k):
    """Ranks of ``k`` farthest-point picks among the rows of ``w`` (k <= len(w)), in w's own precision: pick 0 is rank 0; every
    later pick is the unpicked row with the largest running minimum of ((dx dx + dy dy) + dz dz), the lowest rank among equals."""
    M = len(w)
    picks = np.zeros(k, np.int64)
    if k == 0:
        return picks
    dist = np.full(M, np.inf, w.dtype)
    picked = np.zeros(M, bool)
    s = 0
    for j in range(k):
        picks[j] = s
        picked[s] = True
        if j + 1 == k:
            break
        with np.errstate(all="ignore"):
            d = w - w[s]
            dist = np.minimum(dist, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        s = int(np.argmax(np.where(picked, -1.0, dist)))          # (argmax: the first of the largest, the lowest rank)
    return picks


def cloud32(depth, Ks, transform, n_points, **kw):
    return _cloud(np.float32, depth, Ks, transform, n_points, **kw)


def cloud64(depth, Ks, transform, n_points, **kw):
    return _cloud(np.float64, depth, Ks, transform, n_points, **kw)


def fps_is_greedy(points, picks) -> bool:
    """Brute force: every pick after the first has the largest minimum distance to the earlier picks among the rows not picked
    before it, and the lowest rank among the rows that share that distance; pick 0 is row 0; no row is picked twice."""
    w = np.asarray(points)
    picks = [int(s) for s in picks]
    if not picks:
        return True
    if picks[0] != 0 or len(set(picks)) != len(picks):
        return False
    for j in range(1, len(picks)):
        with np.errstate(all="ignore"):
            d = w[:, None, :] - w[None, picks[:j], :]
            d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1)
        d2[picks[:j]] = -1.0
        if picks[j] != int(np.argmax(d2)):
            return False
    return True
