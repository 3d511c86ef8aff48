"""Host-side conveniences around the deformable splats ("Deformation"): where to put control nodes, and how to turn the
moving vertices a physics engine publishes into the rigid per-node transforms ``Rasterizer.deform`` takes.  Plain numpy, float64 inside;
nothing here touches the GPU but ``NodeDriver``, ``NodeOptimizer``, ``fit_node_transforms`` and ``fit_dynamic_scene``, through the
rasterizer they are given.

    nodes = grid_nodes(bounds, spacing)                  # or farthest_nodes(points, m)
    r.bind_skin(nodes, k=4)
    r.deform(transforms_from_positions(nodes, moved_nodes))       # on the host; or, with the positions on the device:
    driver = NodeDriver(r, nodes); driver.drive(moved_nodes)      # one HIP kernel in front of deform, nothing read back

The other way round -- the node transforms from pictures -- is ``fit_node_transforms``: an optimiser around
``Rasterizer.render_backward`` and ``Rasterizer.deform_backward``, with ``rigidity`` as its regulariser; its twist update runs on the host
in float64 numpy, or (``optimizer="device"``) on the GPU through ``NodeOptimizer``, two HIP kernels on float64 state.  ``fit_dynamic_scene`` fits the
REST scene (and, if asked, the transforms too) from pictures of the object in several bends: ``Rasterizer.deform_backward_rest`` sums the
time steps' gradients, ``Rasterizer.adam_step(rest=True)`` applies them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from ._picture_fit import adam_scalars, device_level, pyramid_level, squared_colour_pass, twist_adam

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


def _fit_positions64(rest_nodes, moved_nodes, neighbours: int = 6, table=None) -> np.ndarray:
    """``transforms_from_positions`` before its rounding to float32: ``[M,3,4]`` float64."""
    a = np.asarray(rest_nodes, np.float64).reshape(-1, 3)
    b = np.asarray(moved_nodes, np.float64).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"rest_nodes {a.shape} and moved_nodes {b.shape} differ in shape")
    M = a.shape[0]
    out = np.zeros((M, 3, 4), np.float64)
    if table is not None:
        nbs = np.asarray(table)
        if nbs.ndim != 2 or nbs.shape[0] != M or nbs.dtype.kind not in "iu":
            raise ValueError(f"transforms_from_positions: table must be an integer array [{M},k], got {nbs.dtype} {list(nbs.shape)}")
        nbs = nbs.astype(np.int64)
        for i in range(M):
            nb = np.concatenate([[i], nbs[i][(nbs[i] >= 0) & (nbs[i] < M)]])
            R = kabsch(a[nb], b[nb])[0] if nb.size >= 2 else np.eye(3)
            out[i, :, :3] = R
            out[i, :, 3] = b[i] - R @ a[i]
        return out
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
    return out


def transforms_from_positions(rest_nodes, moved_nodes, neighbours: int = 6, table=None) -> np.ndarray:
    """Per-node rigid transforms ``[M,3,4]`` float32, rest -> current, from node POSITIONS alone: node i's ``[R | t]`` is the Kabsch fit
    (float64) of itself and its ``neighbours`` nearest rest nodes onto their moved positions, re-centred so that it carries the node
    exactly onto its moved position (``t = moved_i - R rest_i``).  A neighbourhood that does not span a plane and a line off it -- fewer
    than three nodes, or all collinear -- leaves the rotation about its axis undetermined: the fit here then maps the rest line onto the
    moved one, but its twist about that line is whatever the SVD chose, not the least rotation (on drawn collinear neighbourhoods its angle
    exceeds the least one by a median of 42 degrees); ``NodeDriver`` returns the least one.
    This is the bridge from a physics engine's moving vertices to ``Rasterizer.deform``, on the host: an ``[M,M,3]`` table and ``M`` SVDs
    per call.  ``NodeDriver`` is the same bridge on the device.

    ``table [M,k]`` (integers; an entry outside ``[0, M)`` names no neighbour) takes the place of the neighbour search, ``neighbours`` is
    then ignored: node i's members are itself and its live entries in slot order, as ``rigidity(table=)`` takes them (see there on how
    ``Rasterizer.knn_points``' table can differ from the search here at equal distances)."""
    return np.ascontiguousarray(_fit_positions64(rest_nodes, moved_nodes, neighbours, table).astype(np.float32))


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


# ---- node transforms from pictures: how is the cloth bent ("Deformation": the adjoint) -----------------------------------------
def _neighbour_table(nodes, neighbours: int) -> np.ndarray:
    """``[M,k]`` indices of every node's ``k = min(neighbours, M - 1)`` nearest OTHER rest nodes, taken as ``transforms_from_positions`` takes
    them (squared distances in float64, a stable sort: ties to the lower index)."""
    a = np.asarray(nodes, np.float64).reshape(-1, 3)
    M = a.shape[0]
    k = int(min(max(neighbours, 0), M - 1))
    if k <= 0:
        return np.zeros((M, 0), np.int64)
    d2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k + 1]
    out = np.zeros((M, k), np.int64)
    for i in range(M):
        out[i] = [j for j in order[i] if j != i][:k]
    return out


def reverse_table(table) -> Tuple[np.ndarray, np.ndarray]:
    """The reverse of a neighbour table ``[M,k]``: ``(rev_start [M+1], rev_edge [M*k])`` int32.  ``rev_edge[rev_start[j] : rev_start[j+1]]``
    lists the edge numbers ``i * k + slot`` with ``table[i, slot] == j`` in ascending order (a stable sort of the edges by their target);
    entries outside ``[0, M)`` name no node and are left out, and ``rev_edge`` is padded with -1 behind its ``rev_start[M]`` edges.  What
    ``Rasterizer.node_rigidity`` takes beside the table."""
    nb = np.asarray(table)
    if nb.ndim != 2 or nb.dtype.kind not in "iu":
        raise ValueError(f"reverse_table: table must be an integer array [M,k], got {nb.dtype} {list(nb.shape)}")
    M = nb.shape[0]
    flat = nb.reshape(-1).astype(np.int64)
    edges = np.nonzero((flat >= 0) & (flat < M))[0]
    order = np.argsort(flat[edges], kind="stable")
    rev_edge = np.full(flat.size, -1, np.int32)
    rev_edge[:edges.size] = edges[order]
    rev_start = np.zeros(M + 1, np.int32)
    rev_start[1:] = np.cumsum(np.bincount(flat[edges], minlength=M))
    return rev_start, rev_edge


def rigidity(nodes, transforms, neighbours: int = 6, table=None):
    """The embedded-deformation consistency term and its gradient: ``sum_i sum_{j in N(i)} |T_i(g_j) - T_j(g_j)|^2 / (M k)`` with ``g`` the
    rest ``nodes [M,3]``, ``T_i(x) = R_i x + t_i`` the rows of ``transforms [M,3,4]`` and ``N(i)`` node i's ``k = min(neighbours, M - 1)``
    nearest other nodes, taken as ``transforms_from_positions`` takes them: neighbouring nodes should agree on where each other goes.  Zero
    for one rigid motion of all nodes.  Returns ``(value, d_transforms [M,3,4])``, float64, the gradient analytic, the twelve entries of
    every node independent.

    ``table [M,k]`` (integers; an entry outside ``[0, M)`` names no neighbour) takes the place of that neighbour search, ``neighbours``
    is then ignored: ``NodeOptimizer`` regularises over ``Rasterizer.knn_points``' table.  The two searches differ in one respect: the
    search here orders by squared distances in float64, ``knn_points`` by squared distances in float32.  On a grid whose spacing is not
    representable in binary32 (1/7, say) neighbours at EQUAL distance can therefore be chosen differently, and the host and the device
    optimiser then regularise over slightly different edge sets; each is held to its own table.  On a grid with a representable spacing
    (0.5) the two tables are identical."""
    g = np.asarray(nodes, np.float64).reshape(-1, 3)
    T = np.asarray(transforms, np.float64).reshape(-1, 3, 4)
    if T.shape[0] != g.shape[0]:
        raise ValueError(f"rigidity: {g.shape[0]} nodes but {T.shape[0]} transforms")
    M = g.shape[0]
    live = None
    if table is None:
        nb = _neighbour_table(g, neighbours)
    else:
        nb = np.asarray(table)
        if nb.ndim != 2 or nb.shape[0] != M or nb.dtype.kind not in "iu":
            raise ValueError(f"rigidity: table must be an integer array [{M},k], got {nb.dtype} {list(nb.shape)}")
        nb = nb.astype(np.int64)
        live = (nb >= 0) & (nb < M)
        nb = np.where(live, nb, 0)
    d = np.zeros_like(T)
    k = nb.shape[1]
    if k == 0:
        return 0.0, d
    R, t = T[:, :, :3], T[:, :, 3]
    gj = g[nb]                                                                      # [M,k,3]
    res = (np.einsum("mab,mkb->mka", R, gj) + t[:, None, :]) - (np.einsum("mkab,mkb->mka", R[nb], gj) + t[nb])
    if live is not None and not live.all():
        res = np.where(live[:, :, None], res, 0.0)
    scale = 1.0 / (M * k)
    value = float((res * res).sum() * scale)
    dres = 2.0 * scale * res
    d[:, :, :3] = np.einsum("mka,mkb->mab", dres, gj)
    d[:, :, 3] = dres.sum(axis=1)
    np.subtract.at(d[:, :, :3], nb.reshape(-1), np.einsum("mka,mkb->mkab", dres, gj).reshape(-1, 3, 3))
    np.subtract.at(d[:, :, 3], nb.reshape(-1), dres.reshape(-1, 3))
    return value, d


def se3_exp_batch(xi) -> np.ndarray:
    """``register.se3_exp`` of ``xi [M,6]`` twists ``(omega, v)`` at once: ``[M,4,4]`` float64."""
    xi = np.asarray(xi, np.float64).reshape(-1, 6)
    w, v = xi[:, :3], xi[:, 3:]
    th = np.linalg.norm(w, axis=1)
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th * th / 6.0, np.sin(ths) / ths)
    B = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    C = np.where(small, 1.0 / 6.0 - th * th / 120.0, (ths - np.sin(ths)) / ths ** 3)
    Wx = np.zeros((xi.shape[0], 3, 3))
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    W2 = Wx @ Wx
    T = np.tile(np.eye(4), (xi.shape[0], 1, 1))
    T[:, :3, :3] = np.eye(3) + A[:, None, None] * Wx + B[:, None, None] * W2
    T[:, :3, 3] = np.einsum("mab,mb->ma", np.eye(3) + B[:, None, None] * Wx + C[:, None, None] * W2, v)
    return T


def twist_gradient_batch(d_transforms, transforms, pivots=None) -> np.ndarray:
    """``register.twist_gradient`` of ``[M,3,4]`` gradients and transforms at once: the gradient ``[M,6]`` with respect to a twist at 0 that
    left-multiplies each transform; with ``pivots [M,3]`` the twist turns about that point instead of the origin."""
    G = np.asarray(d_transforms, np.float64).reshape(-1, 3, 4)
    A = np.asarray(transforms, np.float64).reshape(-1, 3, 4)
    out = np.zeros((G.shape[0], 6))
    out[:, :3] = np.cross(A.transpose(0, 2, 1), G.transpose(0, 2, 1)).sum(axis=1)   # e_k . sum_c A[:, c] x G[:, c]
    out[:, 3:] = G[:, :, 3]
    if pivots is not None:
        out[:, :3] += np.cross(out[:, 3:], np.asarray(pivots, np.float64).reshape(-1, 3))
    return out


def _twist_step(T, dT, g, m1, m2, it: int, per: int, step):
    """One Adam step (0-based ``it`` of ``per``) of every node's se(3) twist about the node's current position, the step falling to a
    twentieth over ``per`` steps: ``(T, m1, m2)`` after it.  ``T``, ``dT [M,3,4]``, ``g [M,3]`` the rest nodes, ``m1``, ``m2 [M,6]``."""
    piv = np.einsum("mab,mb->ma", T[:, :, :3], g) + T[:, :, 3]   # where every node is now
    xi, m1, m2 = twist_adam(twist_gradient_batch(dT, T, piv), m1, m2, it, per, step)
    E = se3_exp_batch(xi)
    # about the pivot: x -> E (x - p) + p
    Rn = E[:, :3, :3] @ T[:, :, :3]
    tn = np.einsum("mab,mb->ma", E[:, :3, :3], T[:, :, 3] - piv) + E[:, :3, 3] + piv
    return np.concatenate([Rn, tn[:, :, None]], axis=2), m1, m2


class NodeOptimizer:
    """``rigidity`` + ``_twist_step`` on the device (sas_nodes_rigidity, sas_nodes_twist_step; DESIGN.md 3, "Deformation"): the node
    transforms of a skin bound to rasterizer ``r``, their Adam moments and the neighbour graph live there, and a step only enqueues.
    Device tensors it owns: ``nodes [M,3]`` float32, ``table [M,k]`` int32 with its reverse ``rev_start [M+1]`` / ``rev_edge [M*k]``,
    ``transforms64 [M,3,4]``, ``m1``, ``m2 [M,6]`` float64 and ``transforms [M,3,4]`` float32 -- ``transforms64`` rounded once, the
    tensor ``r.deform`` reads where it is.

    The table is ``r.knn_points(nodes, k=min(neighbours, M - 1))``: squared distances in float32, ties to the lower index, the node
    itself left out by index (see ``rigidity`` on how that differs from the host's search); ``neighbours`` is 0..8.  The reverse table
    is built once, on the host, from one read-back of it.  ``transforms [M,3,4]``: where to begin (None: the identity).  ``graph``:
    another NodeOptimizer over the same nodes whose nodes and tables are shared (one graph for the time steps of a dynamic fit).
    Only the constructor and ``read()`` wait for the device."""

    def __init__(self, r, nodes, neighbours: int = 6, transforms=None, graph: Optional["NodeOptimizer"] = None):
        import torch
        from . import _capi
        from .rasterizer import _host
        self.r = r
        if graph is not None:
            self.nodes, self.table, self.rev_start, self.rev_edge = graph.nodes, graph.table, graph.rev_start, graph.rev_edge
        else:
            g = np.ascontiguousarray(np.asarray(_host(nodes), np.float32))
            if g.ndim != 2 or g.shape[1] != 3 or not 1 <= g.shape[0] <= _capi.SAS_KNN_CROSS_MAX_NODES:
                raise ValueError(f"NodeOptimizer: nodes must be [M,3] with 1 <= M <= {_capi.SAS_KNN_CROSS_MAX_NODES}, got {list(g.shape)}")
            if not np.isfinite(g).all():
                raise ValueError("NodeOptimizer: nodes holds non-finite entries")
            if not 0 <= int(neighbours) <= _capi.SAS_NODES_MAX_K:
                raise ValueError(f"NodeOptimizer: neighbours={neighbours} out of [0, {_capi.SAS_NODES_MAX_K}]")
            self.nodes = torch.from_numpy(g).to(r.device)
            k = int(min(int(neighbours), g.shape[0] - 1))
            self.table = self.rev_start = self.rev_edge = None
            if k > 0:
                self.table = r.knn_points(self.nodes, k)["index"]
                rs, re = reverse_table(self.table.cpu().numpy())   # (the one read-back of the set-up)
                self.rev_start, self.rev_edge = torch.from_numpy(rs).to(r.device), torch.from_numpy(re).to(r.device)
        M = int(self.nodes.shape[0])
        dev = r.device
        self.transforms64 = torch.zeros((M, 3, 4), dtype=torch.float64, device=dev)
        self.transforms = torch.zeros((M, 3, 4), dtype=torch.float32, device=dev)
        self.m1 = torch.zeros((M, 6), dtype=torch.float64, device=dev)
        self.m2 = torch.zeros((M, 6), dtype=torch.float64, device=dev)
        self._d_reg = torch.empty((M, 3, 4), dtype=torch.float64, device=dev)
        self._zero = torch.zeros((), dtype=torch.float64, device=dev)
        if transforms is None:
            transforms = np.tile(np.eye(3, 4), (M, 1, 1))
        self.set_transforms(transforms)

    @property
    def m(self) -> int:
        return int(self.nodes.shape[0])

    @property
    def k(self) -> int:
        return 0 if self.table is None else int(self.table.shape[1])

    def set_transforms(self, T) -> None:
        """Replace the transforms (the moments stay: ``reset_moments``).  ``T [M,3,4]``: a device tensor is converted where it is,
        unchecked, as ``Rasterizer.deform`` takes it; anything else is checked for shape and finite entries and copied."""
        import torch
        M = self.m
        if isinstance(T, torch.Tensor) and T.is_cuda:
            if tuple(T.shape) != (M, 3, 4):
                raise ValueError(f"NodeOptimizer: transforms must be [{M},3,4], got {list(T.shape)}")
            self.transforms64.copy_(T.detach())
        else:
            a = np.ascontiguousarray(np.asarray(T.detach().numpy() if isinstance(T, torch.Tensor) else T, np.float64))
            if a.shape != (M, 3, 4) or not np.isfinite(a).all():
                raise ValueError(f"NodeOptimizer: transforms must be finite and [{M},3,4], got {list(a.shape)}")
            self.transforms64.copy_(torch.from_numpy(a))
        self.transforms.copy_(self.transforms64)   # (rounded once)

    def reset_moments(self) -> None:
        self.m1.zero_()
        self.m2.zero_()

    def rigidity(self):
        """``(value, d_transforms [M,3,4])`` of the rigidity term at the current transforms: float64 device tensors, fresh ones."""
        res = self.r.node_rigidity(self.nodes, self.transforms64, self.table, self.rev_start, self.rev_edge)
        return res["value"], res["d_transforms"]

    def step(self, d_transforms, it: int, per: int, step: Tuple[float, float] = (0.01, 0.01), rigidity_weight: Optional[float] = None):
        """One step of ``fit_node_transforms``' update (0-based ``it`` of ``per``) from ``d_transforms [M,3,4]``, the float32 device
        tensor ``Rasterizer.deform_backward`` returns (None: the rigidity term alone), plus ``rigidity_weight`` (None:
        ``RIGIDITY_WEIGHT``) times the rigidity gradient.  Returns the rigidity VALUE at the transforms the step started from, a
        float64 device scalar (exact 0 with a weight of 0 or without neighbours).  Two kernels, enqueued on the current stream."""
        w = RIGIDITY_WEIGHT if rigidity_weight is None else float(rigidity_weight)
        if not w >= 0.0:
            raise ValueError(f"NodeOptimizer.step: rigidity_weight must be >= 0, got {rigidity_weight}")
        it, per = int(it), int(per)
        value, d_reg = self._zero, None
        if w > 0.0 and self.k > 0:
            value = self.r.node_rigidity(self.nodes, self.transforms64, self.table, self.rev_start, self.rev_edge, out=self._d_reg)["value"]
            d_reg = self._d_reg
        if d_transforms is None and d_reg is None:
            raise ValueError("NodeOptimizer.step: no gradient: d_transforms is None and the rigidity term is off")
        decay, c1, c2 = adam_scalars(it, per)   # (the doubles of _twist_step's rule)
        self.r.node_twist_step(self.nodes, self.transforms64, self.m1, self.m2, self.transforms, d_transforms, d_reg, w,
                               lr=(step[0] * decay, step[1] * decay), c1=c1, c2=c2)
        return value

    def read(self) -> np.ndarray:
        """The transforms as float64 numpy ``[M,3,4]``.  Blocking."""
        return self.transforms64.cpu().numpy()


class NodeDriver:
    """``transforms_from_positions`` on the device, in front of ``Rasterizer.deform`` (sas_nodes_fit_rigid; DESIGN.md 3, "Deformation"): the
    bridge from the node positions a simulator holds on the GPU to the deformed scene, without the host in between.  Device tensors it
    owns: ``nodes [M,3]`` float32, ``table [M,k]`` int32 (None without neighbours) and ``transforms [M,3,4]`` float32, written by every
    ``drive`` and read by ``r.deform`` where it is.

    The table is ``r.knn_points(nodes, k=min(neighbours, M - 1))``, as ``NodeOptimizer``'s (``neighbours`` is 0..8).  ``graph``: a
    ``NodeOptimizer`` or ``NodeDriver`` over the same nodes of the same rasterizer whose ``nodes`` and ``table`` are shared: ``knn_points``
    runs once for both; ``neighbours`` is then the graph's, and ``nodes`` is only checked for its shape (None: not at all).
    Every node's rotation is the best rigid fit of itself and its neighbours; a collinear neighbourhood (two nodes, a rope) gets the
    LEAST rotation of all best ones, coincident members the identity.  A node whose moved position is not finite keeps ``[I | 0]`` and is
    left out of its neighbours' fits.

    Not provided: per-member weights; a simulator mesh with more vertices than nodes (index it before the call); a batch of environments
    with different deformations; pinned nodes; stretch and shear."""

    def __init__(self, r, nodes, neighbours: int = 6, graph=None):
        import torch
        from . import _capi
        from .rasterizer import _host
        self.r = r
        if graph is not None:   # (``neighbours`` is the graph's then)
            if graph.r is not r:
                raise ValueError("NodeDriver: graph belongs to another rasterizer")
            if nodes is not None and tuple(np.shape(_host(nodes))) != tuple(graph.nodes.shape):
                raise ValueError(f"NodeDriver: graph is over {list(graph.nodes.shape)} nodes, nodes is {list(np.shape(_host(nodes)))}")
            self.nodes, self.table = graph.nodes, graph.table
        else:
            g = np.ascontiguousarray(np.asarray(_host(nodes), np.float32))
            if g.ndim != 2 or g.shape[1] != 3 or not 1 <= g.shape[0] <= _capi.SAS_KNN_CROSS_MAX_NODES:
                raise ValueError(f"NodeDriver: nodes must be [M,3] with 1 <= M <= {_capi.SAS_KNN_CROSS_MAX_NODES}, got {list(g.shape)}")
            if not np.isfinite(g).all():
                raise ValueError("NodeDriver: nodes holds non-finite entries")
            if not 0 <= int(neighbours) <= _capi.SAS_NODES_MAX_K:
                raise ValueError(f"NodeDriver: neighbours={neighbours} out of [0, {_capi.SAS_NODES_MAX_K}]")
            self.nodes = torch.from_numpy(g).to(r.device)
            k = int(min(int(neighbours), g.shape[0] - 1))
            self.table = r.knn_points(self.nodes, k)["index"] if k > 0 else None
        M = int(self.nodes.shape[0])
        self.transforms = torch.zeros((M, 3, 4), dtype=torch.float32, device=r.device)
        self.transforms[:, 0, 0] = self.transforms[:, 1, 1] = self.transforms[:, 2, 2] = 1.0

    @property
    def m(self) -> int:
        return int(self.nodes.shape[0])

    @property
    def k(self) -> int:
        return 0 if self.table is None else int(self.table.shape[1])

    def _moved(self, moved, steps_allowed: bool):
        """``moved`` as a float32 device tensor: one on the device as it is, anything else checked for its shape and copied."""
        import torch
        M = self.m
        if isinstance(moved, torch.Tensor) and moved.is_cuda:
            return moved.detach()
        a = np.ascontiguousarray(np.asarray(moved.detach().numpy() if isinstance(moved, torch.Tensor) else moved, np.float32))
        if not (a.shape == (M, 3) or (steps_allowed and a.ndim == 3 and a.shape[0] >= 1 and a.shape[1:] == (M, 3))):
            raise ValueError(f"NodeDriver: moved must be [{M},3]" + (f" or [S,{M},3]" if steps_allowed else "") + f", got {list(a.shape)}")
        return torch.from_numpy(a).to(self.r.device)

    def fit(self, moved):
        """The transforms of ``moved [M,3]`` or ``[S,M,3]`` (``S`` time steps, one launch) without deforming anything: ``{"transforms",
        "transforms64"}``, fresh float32 / float64 device tensors ``[M,3,4]`` or ``[S,M,3,4]``.  Only enqueues."""
        return self.r.node_fit_rigid(self.nodes, self._moved(moved, True), self.table)

    def drive(self, moved):
        """Deform the skin bound to the rasterizer by the node positions ``moved [M,3]``: a float32 device tensor is read where it is,
        unchecked; anything else is checked for its shape and copied (non-finite rows are allowed: the kernel's rule).  The fit goes into
        ``self.transforms`` (reused, returned), then ``r.deform(self.transforms)``.  Two kernels enqueued on the current stream; nothing
        blocks."""
        self.r.node_fit_rigid(self.nodes, self._moved(moved, False), self.table, out=self.transforms, want64=False)
        self.r.deform(self.transforms)
        return self.transforms


class _HostNodes:
    """``NodeOptimizer``'s members on the host, for the fitting loops: the node transforms ``transforms64 [M,3,4]`` and their Adam moments
    as float64 numpy, a step ``rigidity`` + ``_twist_step``.  The rigidity term runs over the host's own neighbour search, made once."""

    def __init__(self, nodes, transforms):
        self.nodes = np.asarray(nodes, np.float64).reshape(-1, 3)
        self.table = _neighbour_table(self.nodes, 6)
        self.transforms64 = np.asarray(transforms, np.float64)
        self.reset_moments()

    @property
    def transforms(self) -> np.ndarray:
        """What ``Rasterizer.deform`` takes: contiguous float32, checked there."""
        return np.ascontiguousarray(self.transforms64.astype(np.float32))

    def reset_moments(self) -> None:
        self.m1, self.m2 = np.zeros((self.nodes.shape[0], 6)), np.zeros((self.nodes.shape[0], 6))

    def rigidity(self):
        return rigidity(self.nodes, self.transforms64, table=self.table)

    def step(self, d_transforms, it: int, per: int, step, rigidity_weight: float):
        """``NodeOptimizer.step`` from ``d_transforms [M,3,4]``, read back where it is a device tensor: returns the rigidity value at the
        transforms the step started from, a float (exact 0 with a weight of 0)."""
        import torch
        dT = torch.as_tensor(d_transforms).double().cpu().numpy().reshape(self.transforms64.shape)
        value = 0.0
        if rigidity_weight > 0.0:
            value, d_reg = self.rigidity()
            dT = dT + rigidity_weight * d_reg
        self.transforms64, self.m1, self.m2 = _twist_step(self.transforms64, dT, self.nodes, self.m1, self.m2, it, per, step)
        return value

    def read(self) -> np.ndarray:
        return self.transforms64


@dataclass
class NodeFit:
    transforms: np.ndarray              # [M,3,4] float64, rows [R | t] of every node, rest -> current
    loss: float                         # the last evaluation at full size: mean squared colour difference over the views + rigidity_weight * rigidity
    history: List[Tuple[int, float]] = field(default_factory=list)   # (downsampling factor, loss) of every evaluation


# Chosen on the CPU recovery case of tests/tools/skin_grad_ref.py (a 3x3 node grid under a bent sheet, two 64x48 views, 60 iterations): the run's
# end error over the weights 0, 0.003, 0.01, 0.03 and 0.1 is tabulated there (RECOVER_TABLE); this is the weight with the smallest.
RIGIDITY_WEIGHT = 0.01


def fit_node_transforms(r, images, viewmats, Ks, W: int, H: int, nodes, iters: int = 200, masks=None, start=None,
                        step: Tuple[float, float] = (0.01, 0.01), factors: Sequence[int] = (2, 1), rigidity_weight: float = RIGIDITY_WEIGHT,
                        background=(0.0, 0.0, 0.0), loss_and_grad: Optional[Callable] = None, optimizer: str = "host") -> NodeFit:
    """Fit the node transforms of the skin bound to rasterizer ``r`` so that its frames look like ``images [C,H,W,3]`` (float, 0..1) seen
    from ``viewmats [C,4,4]`` (world -> camera) with ``Ks [C,3,3]``: given pictures of the cloth as it lies now, how is it bent.  ``nodes
    [M,3]``: the rest positions the skin was bound with.  ``register.refine_group_poses``' scheme per node: Adam on an se(3) twist that
    left-multiplies the node's transform about the node's CURRENT position ``R_i g_i + t_i``, coarse to fine over ``factors`` with the step
    (``step``: radians, scene units) falling to a twentieth over each level.  The loss is the mean squared colour difference over ``masks
    [C,H,W]`` averaged over the views, plus ``rigidity_weight * rigidity(nodes, T)``.  Every step is ``r.deform(T)``, one ``render`` +
    ``prechain`` + ``render_backward(out=acc)`` per view into one reused accumulator, ONE ``deform_backward(acc)`` and the stepper's
    ``step``; the losses stay device scalars and come back as one stack at the end.  ``start [M,3,4]``: where to begin (None: the
    identity, the rest pose).  ``r`` is left deformed at the result.  ``loss_and_grad(T [M,3,4], V, K, w, h, target, mask) -> (loss, d_T
    [M,3,4])`` replaces the renderer for one view (tests run the same optimiser on a CPU reference; ``r`` may then be None).

    ``rigidity_weight``: the default was chosen on the CPU recovery case of the tests (a bent sheet under a 3x3 node grid, two views): of
    the weights 0, 0.003, 0.01, 0.03 and 0.1 tried there it ends closest to the true deformed means (0.29 of the start after 60 iterations,
    against 0.34 without the term and 0.39 at 0.1).  The colour loss starts at 2e-3 there: scale the weight with the loss of your scene.

    ``optimizer`` chooses the stepper of that one loop.  ``"host"``: one ``[M,12]`` read-back per step, then ``rigidity`` and the twist
    update in float64 numpy, vectorised over the nodes -- meant for node counts in the hundreds, not for tens of thousands.  ``"device"``:
    a ``NodeOptimizer`` -- the two are HIP kernels on float64 state and ``deform`` reads the transforms where they are, so nothing is read
    back between the first iteration and the last.  Its rigidity term runs over ``Rasterizer.knn_points``' neighbour table (see
    ``rigidity``).  ``"device"`` with ``loss_and_grad`` is refused: that is the CPU reference's door.

    Not fitted: skin weights, node positions; stretch and shear (the twist keeps every transform rigid).  The rest parameters are
    ``fit_dynamic_scene``'s."""
    import torch
    from .rasterizer import _host
    if optimizer not in ("host", "device"):
        raise ValueError(f"fit_node_transforms: optimizer must be 'host' or 'device', got {optimizer!r}")
    if optimizer == "device" and loss_and_grad is not None:
        raise ValueError("fit_node_transforms: optimizer='device' runs the rasterizer's kernels: not with loss_and_grad")
    g = np.asarray(_host(nodes), np.float64).reshape(-1, 3)
    M = g.shape[0]
    Vs = np.asarray(_host(viewmats), np.float64).reshape(-1, 4, 4)
    C = Vs.shape[0]
    K0s = np.asarray(_host(Ks), np.float64).reshape(-1, 3, 3)
    if K0s.shape[0] == 1 and C > 1:
        K0s = np.repeat(K0s, C, axis=0)
    if M < 1 or C < 1 or K0s.shape[0] != C:
        raise ValueError(f"fit_node_transforms: need nodes [M,3], viewmats [C,4,4] and Ks [C,3,3], got {M} nodes, {C} views, {K0s.shape[0]} Ks")
    imgs = torch.as_tensor(np.asarray(_host(images), np.float32)).reshape(C, H, W, 3)
    ms = torch.ones((C, H, W), dtype=torch.float32) if masks is None else (torch.as_tensor(np.asarray(_host(masks))) != 0).to(torch.float32).reshape(C, H, W)
    if start is None:
        T = np.zeros((M, 3, 4))
        T[:, 0, 0] = T[:, 1, 1] = T[:, 2, 2] = 1.0
    else:
        T = np.asarray(_host(start), np.float64).copy()
        if T.shape != (M, 3, 4):
            raise ValueError(f"fit_node_transforms: start must be [{M},3,4], got {list(T.shape)}")
    if not float(rigidity_weight) >= 0.0:
        raise ValueError(f"fit_node_transforms: rigidity_weight must be >= 0, got {rigidity_weight}")
    if loss_and_grad is None and not getattr(r, "has_skin", False):
        raise ValueError("fit_node_transforms: no skin is bound to the rasterizer: bind_skin(nodes) first")
    key = None if loss_and_grad is not None else ("quats" if r.covariance_form == "quats" else "covariances")
    per = max(1, int(iters) // max(1, len(factors)))
    opt = NodeOptimizer(r, g, transforms=T) if optimizer == "device" else _HostNodes(g, T)
    acc, losses, levels = {}, [], []   # the views' summed gradients (made by the first pass, reused), the losses as they come, their levels
    level = (lambda f: pyramid_level(imgs, ms, K0s, W, H, f)) if loss_and_grad is not None else (lambda f: device_level(imgs, ms, Vs, K0s, W, H, f, r.device))

    def evaluate(lv, grad=True):
        """(colour loss averaged over the views, d_T [M,3,4]) at the stepper's transforms and one ``level``; with the renderer both stay on the device."""
        if loss_and_grad is not None:
            w, h, targets, tms, Kcs = lv
            parts = [loss_and_grad(opt.transforms64, Vs[v], Kcs[v], w, h, targets[v], tms[v]) for v in range(C)]
            return sum(p[0] for p in parts) / C, sum(np.asarray(p[1], np.float64).reshape(M, 3, 4) for p in parts) / C
        r.deform(opt.transforms)
        colour = squared_colour_pass(r, *lv, background, acc, want=("means", key))
        return colour, r.deform_backward(acc) if grad else None

    for f in factors:
        lv = level(f)
        opt.reset_moments()
        for it in range(per):
            colour, dT = evaluate(lv)
            reg = opt.step(dT, it, per, step, rigidity_weight)
            losses.append(colour + rigidity_weight * reg)
            levels.append(int(f))
    colour = evaluate(level(1), grad=False)[0]   # (leaves r deformed at the result)
    losses.append(colour + rigidity_weight * opt.rigidity()[0] if rigidity_weight > 0.0 else colour)
    levels.append(1)
    history = torch.stack([torch.as_tensor(x, dtype=torch.float64) for x in losses]).cpu().tolist()   # (the one read-back of the losses)
    return NodeFit(opt.read(), history[-1], list(zip(levels, history)))


# ---- the rest scene from pictures of its motion ("Deformation": the adjoint to the rest arrays) -------------------------------
@dataclass
class DynamicFit:
    history: List[float]                # the loss of every iteration: the views' mean per time step, averaged over the time steps (+ the rigidity terms)
    transforms: np.ndarray              # [S,M,3,4] float64: the node transforms of every time step, as given or as fitted
    steps: int = 0


def fit_dynamic_scene(r, frames, nodes, what: Sequence[str] = ("means", "colors"), transforms=None, fit_transforms: bool = False,
                      iters: int = 100, lrs=None, loss: Optional[str] = None, lambda_dssim: float = 0.2, loss_and_grad: Optional[Callable] = None,
                      rigidity_weight: float = RIGIDITY_WEIGHT, step: Tuple[float, float] = (0.01, 0.01), background=(0.0, 0.0, 0.0),
                      extent: Optional[float] = None, visible_only: bool = True, bound_only: bool = False, renderer=None, optimizer: str = "host") -> DynamicFit:
    """Fit the REST scene of the skin bound to rasterizer ``r`` from pictures of the object in several bends.  ``frames``: one dict per
    time step with ``images [C,H,W,3]`` (float, 0..1), ``viewmats [C,4,4]``, ``Ks [C,3,3]`` and optionally ``masks [C,H,W]``; all images
    have one size.  ``transforms [S,M,3,4]``: the node transforms of every time step, known (from a simulator) or a start value; None:
    the identity.  ``nodes [M,3]``: the rest positions the skin was bound with.  ``what``, ``lrs``, ``extent``, ``loss`` / ``lambda_dssim``
    / ``loss_and_grad`` and ``visible_only`` are ``fit.fit_scene``'s (``what`` names variable groups of the REST scene).

    Per iteration and time step t: ``deform(T_t)``; per view a frame, the loss (a view counts ``1 / C_t``) and
    ``render_backward(out=acc_t)``; then ``deform_backward_rest(acc_t, out=rest_acc)`` for the ``means`` / ``quats`` gradients -- the
    ``opacities``, ``colors`` and ``scales`` gradients are the rest scene's as they are and sum over the time steps by themselves -- and,
    with ``fit_transforms``, ``deform_backward(acc_t)``.  After all time steps ONE ``adam_step(..., rest=True)``, then
    ``fit_node_transforms``' twist update per time step (``step``, ``rigidity_weight``; the step falls to a twentieth over the run).
    With ``fit_transforms`` time step 0 is the anchor: its transforms stay as given, which takes the freedom between rest pose and
    transforms away.  ``bound_only``: only the Gaussians the skin binds (a live entry under ``M`` nodes) are fitted -- ``deform_backward_rest``
    adds nothing for the others, and their ``opacities``, ``colors`` and ``scales`` gradients are zeroed before the step, which with
    ``visible_only`` skips them whole: the static rest of a scene keeps its bits.

    ``r`` is left deformed at the last time step; ``r.clear_skin()`` then ``r.read_scene()`` is the fitted rest scene.  ``renderer``: an
    object with the rasterizer's methods used here, in ``r``'s place (tests run the loop on a CPU reference).  Moments left by an earlier
    fit are dropped first.  Not fitted: skin weights, node positions, stretch and shear.

    ``optimizer`` (with ``fit_transforms``): ``"host"`` reads every time step's ``deform_backward`` back and steps it in float64 numpy.
    ``"device"`` holds one ``NodeOptimizer`` per time step t > 0, all over one neighbour graph: the rigidity term and the twist update
    are kernels, ``deform`` reads their transforms where they are, and nothing is read back before the run ends.  It needs the
    rasterizer's own kernels: refused with ``renderer=``."""
    import torch
    from . import fit as _fit
    from .rasterizer import _host
    R = r if renderer is None else renderer
    who = "fit_dynamic_scene"
    if optimizer not in ("host", "device"):
        raise ValueError(f"{who}: optimizer must be 'host' or 'device', got {optimizer!r}")
    if optimizer == "device" and renderer is not None:
        raise ValueError(f"{who}: optimizer='device' runs the rasterizer's kernels: not with renderer=")
    _fit._check_loss(who, loss, loss_and_grad, lambda_dssim)
    what = tuple(what)
    if not what or any(k not in _fit._WHAT for k in what):
        raise ValueError(f"{who}: what must name some of {_fit._WHAT}, got {what}")
    if not getattr(R, "has_skin", False):
        raise ValueError(f"{who}: no skin is bound to the rasterizer: bind_skin(nodes) first")
    frames = list(frames)
    S = len(frames)
    if S < 1:
        raise ValueError(f"{who}: frames is empty")
    g = np.asarray(_host(nodes), np.float64).reshape(-1, 3)
    M = g.shape[0]
    if transforms is None:
        T = np.zeros((S, M, 3, 4))
        T[:, :, 0, 0] = T[:, :, 1, 1] = T[:, :, 2, 2] = 1.0
    else:
        T = np.asarray(_host(transforms), np.float64).copy()
        if T.shape != (S, M, 3, 4):
            raise ValueError(f"{who}: transforms must be [{S},{M},3,4] (time steps, nodes), got {list(T.shape)}")
    if not float(rigidity_weight) >= 0.0:
        raise ValueError(f"{who}: rigidity_weight must be >= 0, got {rigidity_weight}")
    views, H, W = [], None, None
    for t, f in enumerate(frames):
        img = np.asarray(_host(f["images"]), np.float32)
        if img.ndim != 4 or img.shape[3] != 3 or (H is not None and img.shape[1:3] != (H, W)):
            raise ValueError(f"{who}: frames[{t}]['images'] must be [C,H,W,3], one size for all time steps, got {list(img.shape)}")
        H, W = int(img.shape[1]), int(img.shape[2])
        V, K = _fit._pack_views(f"{who}: frames[{t}]", f["viewmats"], f["Ks"], img, f.get("masks"))
        views.append([V, K, img, f.get("masks"), {}])
    quat_scene = getattr(R, "covariance_form", "quats") == "quats"
    orient = "quats" if quat_scene else "covariances"
    moved = tuple(k for k in ("means", "quats") if k in what)                    # what the deformation moves, of the variables
    passed = tuple(k for k in what if k not in moved)
    want = what + tuple(k for k in ("means", orient) if fit_transforms and k not in what)
    rates = dict(_fit.DEFAULT_LRS, **(lrs or {}))
    bg = tuple(float(v) for v in background)
    lg = _fit.l1_loss_and_grad if loss_and_grad is None else loss_and_grad
    if hasattr(R, "adam_reset"):
        R.adam_reset()
    if extent is None:
        extent = 1.0
        if "means" in what:   # (of the scene as it stands: a bend does not change the scale of things)
            m = R.read_scene()["means"]
            extent = float((m - m.mean(dim=0)).norm(dim=1).max()) if m.shape[0] else 1.0
    n_iters = int(iters)
    bound = None
    if bound_only and passed:
        sk = R.read_skin()
        bound = ((sk["indices"] >= 0) & (sk["indices"] < M) & (sk["weights"] > 0)).any(dim=1)
    opts, held = {}, {}   # the steppers of the time steps that move, and the float32 transforms of those that do not
    for t in range(S):
        if fit_transforms and t > 0:
            opts[t] = NodeOptimizer(R, g, transforms=T[t], graph=opts.get(1)) if optimizer == "device" else _HostNodes(g, T[t])
        else:
            held[t] = np.ascontiguousarray(T[t].astype(np.float32))
            if optimizer == "device":
                held[t] = torch.from_numpy(check_node_transforms(held[t])).to(R.device)
    losses = []
    for it in range(1, n_iters + 1):
        rest_acc, shared, total, dTs = {}, {}, None, {}
        for t, (V, K, img, masks, cache) in enumerate(views):
            R.deform(opts[t].transforms if t in opts else held[t])
            acc_t = dict(shared)
            C = V.shape[0]
            for v in range(C):
                value, acc_t, _ = _fit._view_pass(R, V[v], K[v], W, H, bg, cache, v, img, masks, loss, lg, lambda_dssim, C, out=acc_t, want=want)
                value = torch.as_tensor(value).detach().reshape(()) / (C * S)
                total = value if total is None else total + value
            shared = {k: acc_t[k] for k in passed}
            if moved:
                rest_acc = R.deform_backward_rest({k: acc_t[k] for k in moved}, out=rest_acc, bound_only=bound_only)
            if t in opts:
                dTs[t] = R.deform_backward({k: acc_t[k] for k in ("means", orient)})
        if bound is not None:
            for k, a in shared.items():
                a.mul_(bound.reshape((-1,) + (1,) * (a.dim() - 1)).to(a.dtype))
        R.adam_step(dict(shared, **rest_acc), _fit.step_rates(rates, what, extent, it, n_iters), it, visible_only=visible_only, rest=True)
        for t, d in dTs.items():   # (the host's read-backs wait for the step's work once, here)
            total = total + rigidity_weight * opts[t].step(d, it - 1, n_iters, step, rigidity_weight) / S
        losses.append(total)
    for t, opt in opts.items():
        T[t] = opt.read()
    R.deform(np.ascontiguousarray(T[S - 1].astype(np.float32)))
    history = torch.stack([torch.as_tensor(x, dtype=torch.float64) for x in losses]).cpu().tolist() if losses else []   # (the one read-back of the losses)
    return DynamicFit(history=history, transforms=T, steps=len(history))
