"""Cases of the point-cloud tests (tests/test_cloud_cpu.py, tests/test_gpu_p_cloud.py): drawn depth images with holes and undefined
values, label and colour images, cameras, similarity frames, and DYADIC cases on which float32 arithmetic is exact.  Everything is
drawn from a seed; nothing here knows the code under test."""
import numpy as np


def intrinsics(W, H, f, cx=None, cy=None):
    """[3,3] float32, square pixels, the principal point at the image centre unless given."""
    return np.array([[f, 0, 0.5 * W if cx is None else cx], [0, f, 0.5 * H if cy is None else cy], [0, 0, 1]], np.float32)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def viewmat(axis=(0, 0, 1), degrees=0.0, t=(0, 0, 0)):
    """World-to-camera [4,4] float32."""
    V = np.eye(4)
    V[:3, :3] = rotation(axis, degrees)
    V[:3, 3] = t
    return V.astype(np.float32)


def similarity(scale, axis, degrees, t):
    """4x4 float64 x -> s R x + t: a frame that folds a similarity in (the inverse of an ICP registration, say)."""
    F = np.eye(4)
    F[:3, :3] = scale * rotation(axis, degrees)
    F[:3, 3] = t
    return F


def drawn_views(C, H, W, seed, holes=0.2):
    """depth [C,H,W] float32 in about 0.6..1.8 (a tilted plane plus noise) with a share ``holes`` of zeros, rgb8 [C,H,W,3] and labels
    [C,H,W] uint8 (labels 0..3 in blobs, 255 here and there), view matrices [C,4,4] and intrinsics [C,3,3]."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.stack([1.2 + 0.3 * (u / W - 0.5) * rng.uniform(-1, 1) + 0.3 * (v / H - 0.5) * rng.uniform(-1, 1) + rng.uniform(-0.3, 0.3, (H, W))
                      for _ in range(C)]).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < holes] = 0.0
    rgb8 = rng.integers(0, 256, (C, H, W, 3), dtype=np.uint8)
    labels = ((u // max(1, W // 3) + 2 * (v // max(1, H // 2))) % 4).astype(np.uint8)[None].repeat(C, axis=0).copy()
    labels[rng.uniform(size=labels.shape) < 0.05] = 255
    Vs = np.stack([viewmat(rng.normal(size=3), rng.uniform(-40, 40), rng.uniform(-0.2, 0.2, 3)) for _ in range(C)])
    Ks = np.stack([intrinsics(W, H, rng.uniform(0.8, 1.4) * W) for _ in range(C)])
    return dict(depth=depth, rgb8=rgb8, labels=labels, viewmats=Vs, Ks=Ks, W=W, H=H, C=C)


def with_undefined(depth, seed):
    """A copy with NaN, +Inf, -Inf, 0, -0 and negative depths at drawn pixels; returns (depth, the flat indices touched)."""
    rng = np.random.default_rng(seed)
    d = depth.copy()
    flat = d.reshape(-1)
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, -1e-30], np.float32)
    where = rng.choice(flat.size, size=4 * len(bad), replace=False)
    flat[where] = np.tile(bad, 4)
    return d, where


def exact_count(M, seed, C=2, H=32, W=33):
    """Views of which exactly M pixels carry a depth (the others are holes), at drawn places: M survivors without crop or grid."""
    c = drawn_views(C, H, W, seed, holes=0.0)
    rng = np.random.default_rng(seed + 1)
    assert M <= C * H * W
    flat = c["depth"].reshape(-1)
    keep = np.zeros(flat.size, bool)
    keep[rng.choice(flat.size, size=M, replace=False)] = True
    flat[~keep] = 0.0
    return c


# ---- dyadic cases: float32 arithmetic is exact -------------------------------------------------------------------------------------------
# Depths are integers 1..4 (0: a hole), fx = fy = 8, the principal point an integer, W x H = 16 x 12: (u - cx) d / fx is a multiple of
# 1/8 below 8; transform entries are in {0, +-1, +-0.5} and t is a multiple of 1/4, so every w is a multiple of 1/16 below 32 (9 bits),
# a difference has 10 bits, a square 20, the sum of three 22: nothing is rounded in float32, nor in float64.
DYADIC_T = (
    np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32),
    np.array([[0, -1, 0, 0.25], [1, 0, 0, -0.5], [0, 0, 1, 1.0]], np.float32),
    np.array([[0.5, 0, 0.5, 1.5], [0, -0.5, 0, 0.25], [-0.5, 0, 1, -2.0]], np.float32),
    np.array([[0, 0, -1, 3.0], [0.5, 0.5, 0, 0], [1, -1, 0.5, 0.75]], np.float32),
)


def dyadic(seed, C=2):
    rng = np.random.default_rng(seed)
    H, W = 12, 16
    depth = rng.integers(0, 5, (C, H, W)).astype(np.float32)
    Ks = np.stack([intrinsics(W, H, 8.0, cx=float(rng.integers(4, 12)), cy=float(rng.integers(3, 9))) for _ in range(C)])
    T = np.stack([DYADIC_T[int(rng.integers(0, len(DYADIC_T)))] for _ in range(C)]).reshape(C, 12)
    rgb8 = rng.integers(0, 256, (C, H, W, 3), dtype=np.uint8)
    labels = rng.integers(0, 4, (C, H, W)).astype(np.uint8)
    return dict(depth=depth, Ks=Ks, transform=T, rgb8=rgb8, labels=labels, W=W, H=H, C=C,
                bounds=np.array([[-4.0, -4.0, -4.0], [6.0, 6.0, 6.0]], np.float32), voxel=0.5)
