"""The numpy restatement of sas_knn_points ("Scene from points"), and the clouds the CPU and GPU tests share.

``knn_ref(points, k)`` is chunked brute force in ``np.float32`` with the kernel's expression order:

    d = q - p   (q the candidate, p the point);   d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded to binary32

Candidates are compared by the uint64 key ``bits(d2) << 32 | j``; the k smallest keys win, in ascending order, so equal distances go to
the lower index.  The point itself is left out by index.  A candidate whose d2 is NaN or +inf never counts.  Missing neighbours read
``dist2 = +inf``, ``index = -1``.
"""
from __future__ import annotations

import numpy as np

NONE_KEY = np.uint64((0x7f800000 << 32) | 0xffffffff)


def knn_ref(points, k: int = 3, chunk: int = 1024, indices: bool = True):
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    n = p.shape[0]
    dist2 = np.full((n, k), np.inf, np.float32)
    index = np.full((n, k), -1, np.int32)
    j = np.arange(n, dtype=np.uint64)[None, :]
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            dx = p[None, :, 0] - p[a:b, None, 0]
            dy = p[None, :, 1] - p[a:b, None, 1]
            dz = p[None, :, 2] - p[a:b, None, 2]
            d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j
            bad = ~(d2 < np.float32(np.inf))                       # NaN and +inf
            bad[np.arange(b - a), np.arange(a, b)] = True          # the point itself, by index
            key[bad] = NONE_KEY
            kk = min(k, n)
            part = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1) if n else key[:, :0]
            found = part != NONE_KEY
            dist2[a:b, :kk] = np.where(found, (part >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
            index[a:b, :kk] = np.where(found, (part & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    return (dist2, index) if indices else dist2


def knn_f64(points, k: int = 3):
    """Brute force in float64 (exact products of float32 inputs up to the last sum): the yardstick for inputs without near-ties."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    d = p[None, :, :] - p[:, None, :]
    d2 = (d * d).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    index = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, index, axis=1), index.astype(np.int32)


# ---- the clouds of the tests: name -> float32 [N,3], every one from its own seeded generator -------------------------------------------------
UNIFORM_SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 257, 4099)


def uniform_cube(n: int) -> np.ndarray:
    return np.random.default_rng(1000 + n).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def planar() -> np.ndarray:
    p = np.random.default_rng(11).uniform(-2.0, 2.0, (1500, 3)).astype(np.float32)
    p[:, 1] = np.float32(0.75)   # one axis of zero extent
    return p


def identical() -> np.ndarray:
    return np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (300, 1))


def tenfold() -> np.ndarray:
    p = np.random.default_rng(12).uniform(0.0, 1.0, (120, 3)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(p, 10, axis=0)[np.random.default_rng(13).permutation(1200)])


def lattice() -> np.ndarray:
    g = np.arange(9, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(14).permutation(p.shape[0])])


def clusters_and_outliers() -> np.ndarray:
    rng = np.random.default_rng(15)
    a = rng.normal(0.0, 0.05, (400, 3)) + np.array([1.0, 2.0, 3.0])
    b = rng.normal(0.0, 0.05, (400, 3)) + np.array([-2.0, 1.0, 0.5])
    far = np.array([[1e4, 0.0, 0.0], [0.0, -1e4, 50.0], [30.0, 20.0, 1e4]])
    p = np.concatenate([a, far[:1], b, far[1:]], axis=0).astype(np.float32)
    return p


def non_finite() -> np.ndarray:
    rng = np.random.default_rng(16)
    p = rng.uniform(-1.0, 1.0, (700, 3)).astype(np.float32)
    p[5, 0] = np.nan
    p[17] = np.nan
    p[100, 2] = np.inf
    p[101, 1] = -np.inf
    p[333] = (np.inf, -np.inf, np.nan)
    p[400, 0] = 1e30
    p[401] = (-1e30, 1e30, 1e30)
    p[699, 2] = np.nan
    return p


def sphere() -> np.ndarray:
    v = np.random.default_rng(17).normal(0.0, 1.0, (8229, 3))
    return (2.5 * v / np.linalg.norm(v, axis=1, keepdims=True) + np.array([0.5, -1.0, 2.0])).astype(np.float32)


DISTRIBUTIONS = dict(planar=planar, identical=identical, tenfold=tenfold, lattice=lattice, clusters=clusters_and_outliers,
                     non_finite=non_finite, sphere=sphere)


def cloud(name: str) -> np.ndarray:
    """A cloud by name: ``uniform<N>`` or a key of DISTRIBUTIONS."""
    if name.startswith("uniform"):
        return uniform_cube(int(name[len("uniform"):]))
    return DISTRIBUTIONS[name]()


ALL_CLOUDS = tuple(f"uniform{n}" for n in UNIFORM_SIZES) + tuple(DISTRIBUTIONS)


def init_formulas(points, dist2, colors=None, sh_degree: int = 3, init_opacity: float = 0.1, init_scale: float = 1.0, min_dist2: float = 1e-7):
    """fit.init_scene's arrays in numpy float32 from given neighbour distances ``dist2 [N,3]``."""
    p = np.asarray(points, np.float32)
    n = p.shape[0]
    d = np.asarray(dist2, np.float32)
    m = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)
    s = np.float32(init_scale) * np.sqrt(np.maximum(m, np.float32(min_dist2)))
    if colors is None:
        rgb = np.full((n, 3), 0.5, np.float32)
    else:
        c = np.asarray(colors)
        rgb = c.astype(np.float32) / np.float32(255.0) if c.dtype == np.uint8 else c.astype(np.float32)
    sh = np.zeros((n, (sh_degree + 1) ** 2, 3), np.float32)
    sh[:, 0, :] = (rgb - np.float32(0.5)) / np.float32(0.28209479177387814)
    quats = np.zeros((n, 4), np.float32)
    quats[:, 0] = 1.0
    return dict(means=p, opacities=np.full(n, init_opacity, np.float32), colors=sh, quats=quats,
                scales=np.repeat(s.astype(np.float32)[:, None], 3, axis=1))
