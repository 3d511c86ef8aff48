"""Host-side conveniences around the deformable splats ("Deformation"): where to put control nodes, and how to turn the
moving vertices a physics engine publishes into the rigid per-node transforms ``Rasterizer.deform`` takes.  Plain numpy, float64 inside;
nothing here touches the GPU.

    nodes = grid_nodes(bounds, spacing)                  # or farthest_nodes(points, m)
    r.bind_skin(nodes, k=4)
    r.deform(transforms_from_positions(nodes, moved_nodes))
"""
from __future__ import annotations

import numpy as np

ORTHONORMAL_TOL = 1e-4   # |R^T R - I| a checked node transform may have, per entry


def grid_nodes(bounds, spacing: float) -> np.ndarray:
    """A regular grid of nodes over ``bounds = (lo[3], hi[3])``, at most ``spacing`` apart per axis and with nodes ON both faces of every
    axis: ``ceil(extent / spacing) + 1`` per axis (1 on an axis of zero extent), x fastest.  float32 ``[M,3]``."""
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
    spacing = float(spacing)
    if not (spacing > 0.0 and np.isfinite(spacing)) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError(f"grid_nodes: need finite bounds with hi >= lo and a positive spacing, got {lo}, {hi}, {spacing}")
    counts = [int(np.ceil((hi[a] - lo[a]) / spacing - 1e-9)) + 1 if hi[a] > lo[a] else 1 for a in range(3)]
    if int(np.prod(counts)) > 65536:
        raise ValueError(f"grid_nodes: {counts} is more than 65536 nodes")
    axes = [np.linspace(lo[a], hi[a], counts[a]) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32))


def farthest_nodes(points, m: int, start: int = 0) -> np.ndarray:
    """``m`` of ``points [N,3]`` by farthest-point sampling from ``points[start]`` (ties to the lower index); points with a non-finite
    coordinate are never chosen.  float32 ``[min(m, finite points),3]``.  Host numpy, O(N m): for node sets, not for clouds of millions
    (``Rasterizer.sample_point_cloud`` samples depth frames on the device)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(p).all(axis=1)
    m = int(min(m, int(ok.sum())))
    if m <= 0:
        return np.zeros((0, 3), np.float32)
    cur = int(start) if 0 <= int(start) < p.shape[0] and ok[int(start)] else int(np.argmax(ok))
    dist = np.where(ok, np.inf, -np.inf)
    chosen = []
    for _ in range(m):
        chosen.append(cur)
        d = ((p - p[cur]) ** 2).sum(axis=1)
        dist = np.where(ok, np.minimum(dist, d), -np.inf)
        cur = int(np.argmax(dist))
    return np.ascontiguousarray(p[chosen].astype(np.float32))


def kabsch(src, dst):
    """The rigid ``(R, t)`` (det R = +1) that minimises ``sum |R src_i + t - dst_i|^2``, float64."""
    a, b = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    U, _, Vt = np.linalg.svd((b - cb).T @ (a - ca))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    return R, cb - R @ ca


def transforms_from_positions(rest_nodes, moved_nodes, neighbours: int = 6) -> np.ndarray:
    """Per-node rigid transforms ``[M,3,4]`` float32, rest -> current, from node POSITIONS alone: node i's ``[R | t]`` is the Kabsch fit
    (float64) of itself and its ``neighbours`` nearest rest nodes onto their moved positions, re-centred so that it carries the node
    exactly onto its moved position (``t = moved_i - R rest_i``).  A neighbourhood that does not span a plane and a line off it -- fewer
    than three nodes, or all collinear -- leaves the rotation about its axis undetermined: the fit then returns the least rotation.
    This is the bridge from a physics engine's moving vertices to ``Rasterizer.deform``."""
    a = np.asarray(rest_nodes, np.float64).reshape(-1, 3)
    b = np.asarray(moved_nodes, np.float64).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"rest_nodes {a.shape} and moved_nodes {b.shape} differ in shape")
    M = a.shape[0]
    out = np.zeros((M, 3, 4), np.float64)
    k = int(min(max(neighbours, 0), M - 1))
    d2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(axis=2) if M else np.zeros((0, 0))
    order = np.argsort(d2, axis=1, kind="stable")[:, :k + 1]   # (the node itself first: distance 0; ties to the lower index)
    for i in range(M):
        nb = order[i]
        if i not in nb:
            nb = np.concatenate([[i], nb[:k]])
        R = kabsch(a[nb], b[nb])[0] if k >= 1 else np.eye(3)
        out[i, :, :3] = R
        out[i, :, 3] = b[i] - R @ a[i]
    return np.ascontiguousarray(out.astype(np.float32))


def check_node_transforms(node_transforms) -> np.ndarray:
    """``node_transforms`` as contiguous float32 ``[m,3,4]``, checked as ``Rasterizer.deform`` checks host arrays: the shape, every entry
    finite, and ``R^T R`` within ``ORTHONORMAL_TOL`` of the identity per entry (a sheared or scaled block is refused: the blended
    quaternion would drop the shear silently).  Raises ValueError."""
    a = np.asarray(node_transforms)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"node_transforms must be numeric, got {a.dtype}")
    if a.ndim != 3 or a.shape[1:] != (3, 4):
        raise ValueError(f"node_transforms must be [m,3,4], got {list(a.shape)}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError("node_transforms holds non-finite entries")
    R = a[:, :, :3].astype(np.float64)
    err = np.abs(np.einsum("mki,mkj->mij", R, R) - np.eye(3)).reshape(a.shape[0], -1).max(axis=1) if a.shape[0] else np.zeros(0)
    bad = np.nonzero(err > ORTHONORMAL_TOL)[0]
    if bad.size:
        raise ValueError(f"node_transforms[{int(bad[0])}]: R^T R differs from the identity by {err[bad[0]]:.3g} > {ORTHONORMAL_TOL} "
                         "(node transforms must be rigid: stretch and shear are not represented)")
    mirrored = np.nonzero(np.linalg.det(R) < 0.0)[0] if a.shape[0] else bad
    if mirrored.size:
        raise ValueError(f"node_transforms[{int(mirrored[0])}]: det R < 0 (a reflection is no rotation)")
    return a
