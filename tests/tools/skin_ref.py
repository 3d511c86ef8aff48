"""The numpy restatement of the deformable splats ("Deformation"; csrc/sas_skin.hip), and the scenes, node sets and transforms
the CPU and GPU tests share, every one from a fixed seed.

``knn_cross_ref`` is exact binary32 as knn_ref.py does it: ``d = node - point``, ``d2 = (dx*dx + dy*dy) + dz*dz`` with every operation rounded,
keys ``bits(d2) << 32 | j``, the k smallest ascending; a NaN or +inf ``d2`` never counts, neither does ``d2 > max_distance^2`` (binary32, the
square formed once); nothing is left out by index; missing neighbours read ``+inf`` / ``-1``.

``weights_ref(dtype)`` and ``deform_ref(dtype)`` follow the kernels' and ``bind_skin``'s expression order in ``dtype``: float32 restates the
device's arithmetic (up to its division and square root), float64 is the yardstick.  The tests' bound on the device is four times the
float32 restatement's own error against float64, in the measure ``rel_err``.
"""
from __future__ import annotations

import numpy as np

from knn_ref import NONE_KEY

N = 777          # not a multiple of 256: the n_pad tail is exercised
GROUPS = 2
LDS_NODES = 256  # SAS_SKIN_LDS_BYTES / 64: node records k_deform stages in LDS at most
CHUNK = 256      # SAS_KNN_CHUNK: nodes k_knn_cross stages in LDS at a time


def knn_cross_ref(points, nodes, k: int = 4, max_distance: float = np.inf, chunk: int = 1024):
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    q = np.ascontiguousarray(np.asarray(nodes, dtype=np.float32)).reshape(-1, 3)
    n, m = p.shape[0], q.shape[0]
    dist2 = np.full((n, k), np.inf, np.float32)
    index = np.full((n, k), -1, np.int32)
    j = np.arange(m, dtype=np.uint64)[None, :]
    with np.errstate(all="ignore"):
        md2 = np.float32(max_distance) * np.float32(max_distance)
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            dx = q[None, :, 0] - p[a:b, None, 0]
            dy = q[None, :, 1] - p[a:b, None, 1]
            dz = q[None, :, 2] - p[a:b, None, 2]
            d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j
            key[~((d2 < np.float32(np.inf)) & (d2 <= md2))] = NONE_KEY
            kk = min(k, m)
            part = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
            found = part != NONE_KEY
            dist2[a:b, :kk] = np.where(found, (part >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
            index[a:b, :kk] = np.where(found, (part & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    return dist2, index


def default_sigma(nodes) -> float:
    """bind_skin's default: the mean distance of a node to its nearest OTHER node (knn_ref's float32 d2, the root and the mean in float64);
    1 where no node has a neighbour."""
    from knn_ref import knn_ref
    d2 = knn_ref(nodes, 1, indices=False).astype(np.float64).reshape(-1)
    d2 = d2[np.isfinite(d2)]
    return float(np.mean(np.sqrt(d2))) if d2.size else 1.0


def weights_ref(dist2, index, sigma: float, dtype=np.float64, keep=None):
    """w_j = exp(-(d2_j - d2_0) / (2 sigma^2)); 0 (and index -1) for a missing neighbour and outside ``keep``."""
    d2 = np.asarray(dist2, np.float32).astype(dtype)
    idx = np.asarray(index, np.int32).copy()
    with np.errstate(all="ignore"):
        w = np.exp(-(d2 - d2[:, :1]) / dtype(2.0 * sigma * sigma)).astype(dtype)
    off = idx < 0
    if keep is not None:
        off = off | ~np.asarray(keep, bool)[:, None]
    w[off] = 0
    idx[off] = -1
    return idx, w


def node_quats(R, dtype=np.float64):
    """[m,3,3] -> unit wxyz [m,4] by the branch of the largest of (trace, R00, R11, R22), each branch's terms as k_skin_nodes forms them."""
    R = np.asarray(R, np.float32).astype(dtype)
    one = dtype(1.0)
    r = lambda i, j: R[:, i, j]
    tr = (r(0, 0) + r(1, 1)) + r(2, 2)
    b0 = (tr >= r(0, 0)) & (tr >= r(1, 1)) & (tr >= r(2, 2))
    b1 = ~b0 & (r(0, 0) >= r(1, 1)) & (r(0, 0) >= r(2, 2))
    b2 = ~b0 & ~b1 & (r(1, 1) >= r(2, 2))
    q0 = np.stack([one + tr, r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1)], axis=1)
    q1 = np.stack([r(2, 1) - r(1, 2), ((one + r(0, 0)) - r(1, 1)) - r(2, 2), r(0, 1) + r(1, 0), r(0, 2) + r(2, 0)], axis=1)
    q2 = np.stack([r(0, 2) - r(2, 0), r(0, 1) + r(1, 0), ((one + r(1, 1)) - r(0, 0)) - r(2, 2), r(1, 2) + r(2, 1)], axis=1)
    q3 = np.stack([r(1, 0) - r(0, 1), r(0, 2) + r(2, 0), r(1, 2) + r(2, 1), ((one + r(2, 2)) - r(0, 0)) - r(1, 1)], axis=1)
    q = np.where(b0[:, None], q0, np.where(b1[:, None], q1, np.where(b2[:, None], q2, q3))).astype(dtype)
    inv = one / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    return (q * inv[:, None]).astype(dtype)


def deform_ref(rest, indices, weights, node_Rt, dtype=np.float64):
    """``rest``: dict of float32 ``means [N,3]`` and ``quats [N,4]`` or ``covariances [N,6]``.  Returns the deformed arrays under the same keys,
    in ``dtype``.  Entries are live when 0 <= index < m and weight > 0; a Gaussian without one keeps the rest values exactly."""
    G = np.asarray(node_Rt, np.float32).reshape(-1, 3, 4)
    m = G.shape[0]
    R, t = G[:, :, :3].astype(dtype), G[:, :, 3].astype(dtype)
    Q = node_quats(G[:, :, :3], dtype)
    mean = np.asarray(rest["means"], np.float32).astype(dtype)
    idx = np.asarray(indices).astype(np.int64)
    wts = np.asarray(weights, np.float32).astype(dtype)
    n, k = idx.shape
    zero, one, two = dtype(0.0), dtype(1.0), dtype(2.0)
    acc = np.zeros((n, 3), dtype)
    W = np.zeros(n, dtype)
    aq = np.zeros((n, 4), dtype)
    f = np.zeros((n, 4), dtype)
    any_ = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for e in range(k):
            live = (idx[:, e] >= 0) & (idx[:, e] < m) & (wts[:, e] > 0)
            ic = np.where(live, idx[:, e], 0)
            we = wts[:, e]
            Rj, tj, qj = R[ic], t[ic], Q[ic]
            y = ((Rj[:, :, 0] * mean[:, None, 0] + Rj[:, :, 1] * mean[:, None, 1]) + Rj[:, :, 2] * mean[:, None, 2]) + tj
            acc = np.where(live[:, None], acc + we[:, None] * (y - mean), acc)
            W = np.where(live, W + we, W)
            f = np.where((live & ~any_)[:, None], qj, f)
            any_ = any_ | live
            dot = ((qj[:, 0] * f[:, 0] + qj[:, 1] * f[:, 1]) + qj[:, 2] * f[:, 2]) + qj[:, 3] * f[:, 3]
            sw = np.where(dot < 0, -we, we)
            aq = np.where(live[:, None], aq + sw[:, None] * qj, aq)
        out = {"means": np.where(any_[:, None], mean + acc / W[:, None], mean).astype(dtype)}
        n2 = ((aq[:, 0] * aq[:, 0] + aq[:, 1] * aq[:, 1]) + aq[:, 2] * aq[:, 2]) + aq[:, 3] * aq[:, 3]
        ok = (n2 > 0) & np.isfinite(n2)
        qb = np.where(ok[:, None], aq * (one / np.sqrt(n2))[:, None], f).astype(dtype)
    bw, bx, by, bz = qb[:, 0], qb[:, 1], qb[:, 2], qb[:, 3]
    if rest.get("quats") is not None:
        r = np.asarray(rest["quats"], np.float32).astype(dtype)
        rw, rx, ry, rz = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
        q = np.stack([((bw * rw - bx * rx) - by * ry) - bz * rz, ((bw * rx + bx * rw) + by * rz) - bz * ry,
                      ((bw * ry - bx * rz) + by * rw) + bz * rx, ((bw * rz + bx * ry) - by * rx) + bz * rw], axis=1)
        out["quats"] = np.where(any_[:, None], q, r).astype(dtype)
    else:
        c = np.asarray(rest["covariances"], np.float32).astype(dtype)
        Rb = np.stack([np.stack([one - two * (by * by + bz * bz), two * (bx * by - bw * bz), two * (bx * bz + bw * by)], axis=1),
                       np.stack([two * (bx * by + bw * bz), one - two * (bx * bx + bz * bz), two * (by * bz - bw * bx)], axis=1),
                       np.stack([two * (bx * bz - bw * by), two * (by * bz + bw * bx), one - two * (bx * bx + by * by)], axis=1)], axis=1)
        S = np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], axis=1), np.stack([c[:, 1], c[:, 3], c[:, 4]], axis=1),
                      np.stack([c[:, 2], c[:, 4], c[:, 5]], axis=1)], axis=1)
        T = np.stack([np.stack([(Rb[:, i, 0] * S[:, 0, j] + Rb[:, i, 1] * S[:, 1, j]) + Rb[:, i, 2] * S[:, 2, j] for j in range(3)], axis=1)
                      for i in range(3)], axis=1)
        o = lambda i, j: (T[:, i, 0] * Rb[:, j, 0] + T[:, i, 1] * Rb[:, j, 1]) + T[:, i, 2] * Rb[:, j, 2]
        cov = np.stack([o(0, 0), o(0, 1), o(0, 2), o(1, 1), o(1, 2), o(2, 2)], axis=1)
        out["covariances"] = np.where(any_[:, None], cov, c).astype(dtype)
    return out


def rel_err(x, ref) -> float:
    """max |x - ref| / max |ref|: the measure of the four-times rule."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max()) if ref.size else 0.0


# ---- the scenes, node sets and transforms of the tests ---------------------------------------------------------------------------------------
def quat_to_matrix(q):
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=-1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=-1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)], axis=-2)


def scene(form: str = "quats", n: int = N, seed: int = 40):
    """N Gaussians in GROUPS splat groups around the origin, as ``Rasterizer.upload``'s keyword arguments (plain colours)."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 0.4, (n, 3)).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    scales = rng.uniform(0.03, 0.1, (n, 3)).astype(np.float32)
    kw = dict(means=means, opacities=rng.uniform(0.2, 0.95, n).astype(np.float32), colors=rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32),
              sh_degree=-1, group_id=(np.arange(n) % GROUPS).astype(np.uint8), n_groups=GROUPS)
    if form == "quats":
        kw.update(quats=quats, scales=scales)
    else:
        M = quat_to_matrix(quats) * scales.astype(np.float64)[:, None, :]
        S = M @ np.swapaxes(M, 1, 2)
        kw.update(covariances=np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32))
    return kw


def rest_of(kw):
    """A scene's arrays as deform_ref takes them."""
    return {k: kw[k] for k in ("means", "quats", "covariances") if k in kw}


def cloud(n: int = N, seed: int = 41) -> np.ndarray:
    return np.random.default_rng(seed + n).normal(0.0, 0.4, (n, 3)).astype(np.float32)


def nodes(name: str) -> np.ndarray:
    """A node set by name: ``m<M>`` (M uniform nodes in the scene's box), ``dup`` (40 nodes, each twice, shuffled), ``non_finite`` (70 with NaN
    and inf entries, and one whose d2 overflows)."""
    if name == "dup":
        q = np.random.default_rng(50).uniform(-0.8, 0.8, (40, 3)).astype(np.float32)
        return np.ascontiguousarray(np.tile(q, (2, 1))[np.random.default_rng(51).permutation(80)])
    if name == "non_finite":
        q = np.random.default_rng(52).uniform(-0.8, 0.8, (70, 3)).astype(np.float32)
        q[3, 0] = np.nan
        q[10] = np.nan
        q[20, 2] = np.inf
        q[21, 1] = -np.inf
        q[40] = (1e30, 0.0, 0.0)
        return q
    m = int(name[1:])
    return np.random.default_rng(60 + m).uniform(-0.8, 0.8, (m, 3)).astype(np.float32)


def non_finite_cloud() -> np.ndarray:
    p = cloud(300, 70)
    p[5, 0] = np.nan
    p[17] = np.nan
    p[100, 2] = np.inf
    p[101, 1] = -np.inf
    p[200] = (-1e30, 1e30, 1e30)
    return p


def transforms(node_xyz, seed: int = 80, angle: float = 0.7, shift: float = 0.08) -> np.ndarray:
    """Rigid [m,3,4] float32: node i turns by up to ``angle`` about a random axis THROUGH ITSELF and moves by up to ``shift`` per axis."""
    c = np.asarray(node_xyz, np.float64).reshape(-1, 3)
    m = c.shape[0]
    rng = np.random.default_rng(seed + m)
    axis = rng.normal(size=(m, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = 0.5 * rng.uniform(-angle, angle, m)
    R = quat_to_matrix(np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * axis], axis=1))
    t = c + rng.uniform(-shift, shift, (m, 3)) - np.einsum("mij,mj->mi", R, c)
    return np.ascontiguousarray(np.concatenate([R, t[:, :, None]], axis=2).astype(np.float32))


def identity_transforms(m: int) -> np.ndarray:
    G = np.zeros((m, 3, 4), np.float32)
    G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
    return G
