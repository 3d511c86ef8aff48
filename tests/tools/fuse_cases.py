"""Cases of the depth-fusion tests (tests/test_fuse_cpu.py, tests/test_gpu_r_fuse.py): analytic sphere and box geometry, DYADIC cases on
which float32 arithmetic is exact up to the first division, an EDGE volume whose voxels sit exactly on the contract's thresholds, and
drawn views (cloud_cases.drawn_views) with a volume in front of them.  Everything is computed from its arguments or drawn from a seed;
nothing here knows the code under test."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from cloud_cases import DYADIC_T, drawn_views, intrinsics, viewmat, with_undefined  # noqa: E402,F401


# ---- analytic sphere -------------------------------------------------------------------------------------------------------------------
def sphere_tsdf(n=16, r=0.3, trunc_voxels=3.0):
    """(tsdf, weight, lo, voxel) of an n^3 volume over [-0.5,0.5]^3: tsdf = clip((|x| - r) / (trunc_voxels voxel), -1, 1) at the voxel
    centres, every voxel observed once."""
    voxel = 1.0 / n
    lo = np.full(3, -0.5)
    c = lo[0] + (np.arange(n) + 0.5) * voxel
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    d = np.sqrt(x * x + y * y + z * z)
    return np.clip((d - r) / (trunc_voxels * voxel), -1.0, 1.0).astype(np.float32), np.ones((n, n, n), np.float32), lo, voxel


def axis_viewmats(distance=1.5):
    """World-to-camera [6,4,4] float32 of six cameras on the +-x, +-y, +-z axes at ``distance`` that look at the origin (OpenCV axes: +z
    forward).  Rotations are signed permutations: exact in float32."""
    out = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            zc = np.zeros(3)
            zc[axis] = -sign                              # forward: towards the origin
            xc = np.zeros(3)
            xc[(axis + 1) % 3] = 1.0
            yc = np.cross(zc, xc)
            R = np.stack([xc, yc, zc])                       # world -> camera rows
            V = np.eye(4)
            V[:3, :3] = R
            V[:3, 3] = -R @ (sign * distance * np.eye(3)[axis])
            out.append(V)
    return np.stack(out).astype(np.float32)


def sphere_depths(viewmats, K, W, H, r=0.3, fill=4.0):
    """Depth images [C,H,W] float32 of the sphere |x| = r about the origin: the camera-frame z of the first intersection of the ray
    through the pixel's centre (u + 0.5, v + 0.5), ``fill`` where the ray misses."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    K = np.asarray(K, np.float64)
    d = np.stack([(u + 0.5 - K[0, 2]) / K[0, 0], (v + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(u, dtype=np.float64)], axis=-1)   # z = 1 rays
    out = []
    for V in np.asarray(viewmats, np.float64):
        o = V[:3, 3]                                         # the origin of the world in the camera frame: the sphere's centre
        a = (d * d).sum(-1)
        b = (d * o).sum(-1)
        disc = b * b - a * ((o * o).sum() - r * r)
        t = (b - np.sqrt(np.maximum(disc, 0.0))) / a         # the nearer root of |t d - o|^2 = r^2: the depth, since d_z = 1
        out.append(np.where(disc > 0, t, fill))
    return np.stack(out).astype(np.float32)


def sphere_case(fill=4.0, n=16, r=0.3, W=48, H=40, f=60.0, distance=1.5):
    V = axis_viewmats(distance)
    K = intrinsics(W, H, f)
    voxel = 1.0 / n
    return dict(depth=sphere_depths(V, K, W, H, r, fill), viewmats=V, Ks=np.stack([K] * 6), W=W, H=H, C=6, lo=np.full(3, -0.5, np.float32),
                voxel=voxel, dims=(n, n, n), trunc=3.0 * voxel, r=r)


# ---- mesh checks (closedness, Euler number, volume) -------------------------------------------------------------------------------------
def mesh_topology(vertices, faces):
    """dict(closed, euler, volume): ``closed`` iff every undirected edge lies in exactly two triangles that run through it in opposite
    directions; Euler number V - E + F over the vertices the faces use; the signed volume (positive: outward normals)."""
    f = np.asarray(faces, np.int64)
    v = np.asarray(vertices, np.float64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(e, axis=1)
    key, inv, counts = np.unique(und, axis=0, return_inverse=True, return_counts=True)
    direction = np.where(e[:, 0] < e[:, 1], 1, -1)
    balance = np.zeros(len(key), np.int64)
    np.add.at(balance, np.asarray(inv).reshape(-1), direction)
    closed = bool(len(f) > 0 and (counts == 2).all() and (balance == 0).all())
    tri = v[f]
    volume = float((tri[:, 0] * np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0)
    return dict(closed=closed, euler=int(len(np.unique(f)) - len(key) + len(f)), volume=volume, edges=len(key))


def box_distance(p, lo, hi):
    """Unsigned distance of points [n,3] to the SURFACE of the axis-aligned box [lo, hi]."""
    p, lo, hi = np.asarray(p, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    outside = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
    inside = np.minimum(p - lo, hi - p).min(axis=1)
    return np.where(outside > 0, outside, np.maximum(inside, 0.0))


def box_mesh(lo, hi):
    """(vertices [8,3], faces [12,3]) of the box, outward normals."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (c >> k) & 1 else lo)[k] for k in range(3)] for c in range(8)])
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]])
    return v, f


# ---- dyadic cases: float32 arithmetic is exact up to the first division ----------------------------------------------------------------------
# voxel = 1/4 and lo a multiple of 1/8: a voxel centre is a multiple of 1/8 below 4 (5 bits).  DYADIC_T entries are in {0, +-1, +-0.5} and
# its t a multiple of 1/4: every product is a multiple of 1/16, every q a multiple of 1/16 below 16 (8 bits): nothing is rounded in
# float32, nor in float64.  Depths are integers 1..4 (0: a hole): sdf = d - q_z is a multiple of 1/16 below 32, exact; trunc is a power of
# two: sdf / trunc is exact.  The first operation that rounds is q_x / q_z.
def dyadic(seed, C=3, pixel_centre=0.5):
    rng = np.random.default_rng(seed)
    H, W = 12, 16
    depth = rng.integers(0, 5, (C, H, W)).astype(np.float32)
    Ks = np.stack([intrinsics(W, H, 8.0, cx=float(rng.integers(4, 12)), cy=float(rng.integers(3, 9))) for _ in range(C)])
    T = np.stack([DYADIC_T[int(rng.integers(0, len(DYADIC_T)))] for _ in range(C)]).reshape(C, 12)
    return dict(depth=depth, Ks=Ks, transform=T, rgb8=rng.integers(0, 256, (C, H, W, 3), dtype=np.uint8), labels=rng.integers(0, 4, (C, H, W)).astype(np.uint8),
                W=W, H=H, C=C, lo=np.array([-1.0, -0.875, 0.5], np.float32), voxel=0.25, dims=(9, 7, 11), trunc=float(2.0 ** int(rng.integers(-2, 1))),
                pixel_centre=pixel_centre)


# ---- the edge volume: voxels exactly on the thresholds ------------------------------------------------------------------------------------
# 3 x 3 x 3 voxels of 1/4 with centres x, y in {-1/4, 0, 1/4} and z in {3/4, 1, 5/4}, seen by ONE identity camera with fx = fy = 8 in an
# 8 x 8 image of constant depth.  In the layer z = 1: q_x / q_z = x exactly, fx x = -2, 0, 2; uf = ((fx x + cx) - pixel_centre) + 0.5.
#   cx = 2 (pixel_centre 0.5): the column x = -1/4 has uf = 0 exactly (in); with cx one float lower it is out
#   cx = 6: the column x = 1/4 has uf = 8 = W exactly (out); with cx one float lower it is in (cy and vf likewise)
#   near = 1: the layer z = 1 is in front (q_z >= near); with near one float higher it is not
#   depth 1/2, trunc 1/2: the layer has sdf = -trunc exactly (updated, val -1); with trunc one float lower it is skipped
#   depth 3/2, trunc 1/2, carving pixels: the layer has sdf = trunc exactly (updated, val 1); with trunc one float higher it is skipped
# (a threshold is approached through cx, near and trunc, which enter one comparison each: a depth one float off 1/2 gives the same sdf,
# d - 1 rounds back onto -1/2)
def edge_volume(depth=1.0, cx=4.0, cy=4.0, label=0):
    W = H = 8
    return dict(depth=np.full((1, H, W), depth, np.float32), Ks=intrinsics(W, H, 8.0, cx=cx, cy=cy)[None], transform=DYADIC_T[0].reshape(1, 12),
                rgb8=np.full((1, H, W, 3), 200, np.uint8), labels=np.full((1, H, W), label, np.uint8), W=W, H=H, C=1,
                lo=np.array([-0.375, -0.375, 0.625], np.float32), voxel=0.25, dims=(3, 3, 3), trunc=0.5)


def around(x):
    """(the float32 below x, x, the float32 above x)"""
    x = np.float32(x)
    return float(np.nextafter(x, np.float32(-np.inf))), float(x), float(np.nextafter(x, np.float32(np.inf)))


# ---- drawn cases -------------------------------------------------------------------------------------------------------------------------
def drawn(C, H, W, seed, dims, voxel=None, centre=(0.0, 0.0, 1.2), holes=0.2):
    """cloud_cases.drawn_views (depths about 0.6 .. 1.8 in front of cameras that look roughly down +z from near the origin) with a volume
    of ``dims`` voxels around ``centre``, where the depths are: its longest side 1.6 unless ``voxel`` is given.  trunc = 0.2."""
    c = drawn_views(C, H, W, seed, holes=holes)
    dims = tuple(int(d) for d in dims)
    voxel = 1.6 / max(dims) if voxel is None else float(voxel)
    lo = (np.asarray(centre, np.float64) - 0.5 * voxel * np.asarray(dims)).astype(np.float32)
    c.update(lo=lo, voxel=voxel, dims=dims, trunc=0.2)
    return c
