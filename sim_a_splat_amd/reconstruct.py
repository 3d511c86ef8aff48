"""Geometry from the splat: a triangle mesh of what the scene shows, by TSDF fusion of rendered depth and surface nets.

    python -m sim_a_splat_amd.reconstruct --splat SCENE --bounds x0 y0 z0 x1 y1 z1 --voxel 0.004 --out mesh.obj [--masks-dir DIR --rows link3 ...]

An object that exists only as Gaussians -- a mug, the table, the T-block as it was captured -- gets its collision and visual mesh here:
label frames from an orbit of cameras (``SplatScene.fuse_views``) are integrated on the GPU into a truncated-signed-distance volume
(``Rasterizer.fuse_depth``, sas_fuse_depth; DESIGN.md 3, "Depth fusion"), and ``surface_nets`` extracts the zero level on the host, once
per reconstruction.  The result goes to ``upload_meshes``, ``query_meshes``, ``register_robot`` or, through ``mesh_io.save_obj``, to a
file the physics side loads.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .poses import matrix_to_quat_wxyz

MAX_DIM = 1024        # voxels along an axis (sas_fuse_depth)
MAX_VOXELS = 2 ** 27


def volume_dims(lo, hi, voxel_size: float) -> Tuple[int, int, int]:
    """``(nx, ny, nz)`` of the smallest grid of ``voxel_size`` cubes from ``lo`` that covers ``hi``; ValueError when it is not a volume
    ``sas_fuse_depth`` takes."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    v = float(voxel_size)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(v) and v > 0 and (hi > lo).all()):
        raise ValueError(f"a volume needs finite lo < hi and a voxel size > 0, got {lo.tolist()}, {hi.tolist()}, {v}")
    n = np.ceil((hi - lo) / v - 1e-9)
    if n.max() > MAX_DIM or n.prod() > MAX_VOXELS:
        raise ValueError(f"{n.astype(np.int64).tolist()} voxels: at most {MAX_DIM} along an axis and 2^27 in all")
    return tuple(int(max(1, x)) for x in n)


class TsdfVolume:
    """A TSDF volume on a rasterizer's device: ``tsdf`` (ones: free space) and ``weight`` (zeros: nothing observed) ``[nz,ny,nx]``
    float32 and, with ``color``, ``color [nz,ny,nx,3]`` float32 (0..255).  Voxel ``(i,j,k)`` has its centre at
    ``lo + (i + 0.5, j + 0.5, k + 0.5) voxel_size``.  Give ``dims = (nx, ny, nz)`` or ``hi``."""

    def __init__(self, rasterizer, lo, voxel_size: float, dims: Optional[Sequence[int]] = None, hi=None, color: bool = True):
        import torch
        if (dims is None) == (hi is None):
            raise ValueError("give dims or hi")
        self.rasterizer = rasterizer
        self.lo = np.asarray(lo, np.float32).reshape(3).copy()
        self.voxel_size = float(voxel_size)
        self.dims = volume_dims(lo, hi, voxel_size) if dims is None else tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1 or max(self.dims) > MAX_DIM or int(np.prod(self.dims, dtype=np.int64)) > MAX_VOXELS:
            raise ValueError(f"dims {self.dims}: three sizes in [1,{MAX_DIM}], at most 2^27 voxels in all")
        nx, ny, nz = self.dims
        dev = rasterizer.device
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=dev)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
        self.color = torch.zeros((nz, ny, nx, 3), dtype=torch.float32, device=dev) if color else None

    def reset(self) -> None:
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def integrate(self, depth, viewmats, Ks, width: int, height: int, **kw) -> None:
        """``Rasterizer.fuse_depth`` into this volume."""
        self.rasterizer.fuse_depth(self, depth, viewmats, Ks, width, height, **kw)

    def extract_mesh(self, min_weight: float = 1.0):
        """``surface_nets`` of the volume as it stands (copied to the host): ``(vertices, faces, colors)``."""
        return surface_nets(self.tsdf.cpu().numpy(), self.weight.cpu().numpy(), self.lo, self.voxel_size,
                            color=None if self.color is None else self.color.cpu().numpy(), min_weight=min_weight)


# corner c of a cell has offsets (c & 1, c >> 1 & 1, c >> 2 & 1) along (x, y, z); its 12 edges, four per axis
_CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])
_EDGES = [(a, a | (1 << axis)) for axis in range(3) for a in range(8) if not a & (1 << axis)]


def surface_nets(tsdf, weight, lo, voxel: float, color=None, min_weight: float = 1.0):
    """Naive surface nets of a sampled signed distance, in float64, table-free and deterministic.

    ``tsdf``, ``weight [nz,ny,nx]``: samples at the voxel centres ``lo + (i + 0.5, j + 0.5, k + 0.5) voxel``.  A voxel is observed iff
    ``weight >= min_weight`` (and its tsdf is not a NaN), inside iff ``tsdf < 0``.  Cell ``(i,j,k)``, ``i < nx - 1`` and likewise, is active
    iff its 8 corner voxels are all observed and not all of one sign; its vertex is the mean of the crossing points ``p0 + (f0 / (f0 -
    f1)) (p1 - p0)`` on those of its 12 edges whose ends differ in sign, its colour the mean of the 8 corners' ``color [nz,ny,nx,3]``.
    Vertices are ordered by ascending cell index ``(k (ny - 1) + j) (nx - 1) + i``.  Every grid edge between a voxel and its +x, +y or
    +z neighbour whose ends differ in sign and whose four surrounding cells all exist and are active makes one quad of those cells'
    vertices, split into two triangles along the same diagonal and wound so that the normal points from the inside end to the
    outside end; faces are ordered by axis, then by the edge's (lower voxel's) flat index.

    Returns ``vertices [V,3]`` float64, ``faces [F,3]`` int32 and ``colors [V,3]`` uint8 (None without ``color``)."""
    f = np.asarray(tsdf, np.float64)
    w = np.asarray(weight, np.float64)
    if f.ndim != 3 or w.shape != f.shape:
        raise ValueError(f"tsdf and weight must be [nz,ny,nx], got {list(f.shape)} and {list(w.shape)}")
    nz, ny, nx = f.shape
    lo = np.asarray(lo, np.float64).reshape(3)
    voxel = float(voxel)
    empty = (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32), None if color is None else np.zeros((0, 3), np.uint8))
    if min(nx, ny, nz) < 2:
        return empty
    observed = (w >= min_weight) & ~np.isnan(f)
    inside = f < 0

    def corner(a, c):   # the [nz-1,ny-1,nx-1] view of `a` at the cells' corner c
        ox, oy, oz = _CORNERS[c]
        return a[oz:nz - 1 + oz, oy:ny - 1 + oy, ox:nx - 1 + ox]

    all_obs = np.ones((nz - 1, ny - 1, nx - 1), bool)
    n_in = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        all_obs &= corner(observed, c)
        n_in += corner(inside, c)
    active = all_obs & (n_in > 0) & (n_in < 8)
    ck, cj, ci = np.nonzero(active)                          # (C order: ascending cell index)
    V = len(ci)
    if V == 0:
        return empty
    base = np.stack([ci, cj, ck], axis=1)
    fc = np.stack([f[ck + o[2], cj + o[1], ci + o[0]] for o in _CORNERS], axis=1)        # [V,8]
    sc = fc < 0
    acc, cnt = np.zeros((V, 3)), np.zeros(V)
    for a, b in _EDGES:
        cross = sc[:, a] != sc[:, b]
        f0, f1 = fc[:, a], fc[:, b]
        t = np.where(cross, f0 / np.where(cross, f0 - f1, 1.0), 0.0)
        p0 = lo + (base + _CORNERS[a] + 0.5) * voxel
        p1 = lo + (base + _CORNERS[b] + 0.5) * voxel
        acc += np.where(cross[:, None], p0 + t[:, None] * (p1 - p0), 0.0)
        cnt += cross
    vertices = acc / cnt[:, None]
    colors = None
    if color is not None:
        col = np.asarray(color, np.float64).reshape(nz, ny, nx, 3)
        mean = sum(col[ck + o[2], cj + o[1], ci + o[0]] for o in _CORNERS) / 8.0
        colors = np.clip(np.rint(mean), 0, 255).astype(np.uint8)
    vid = np.full((nz - 1, ny - 1, nx - 1), -1, np.int64)
    vid[ck, cj, ci] = np.arange(V)
    faces = []
    for axis in range(3):
        # voxels (i,j,k) with a neighbour along `axis` and, across the other two axes, cells on both sides
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3               # (axis, a1, a2) is a right-handed triple
        n = (nx, ny, nz)
        rng = [None, None, None]
        rng[axis] = np.arange(0, n[axis] - 1)
        rng[a1] = np.arange(1, n[a1] - 1)
        rng[a2] = np.arange(1, n[a2] - 1)
        if min(len(r) for r in rng) == 0:
            continue
        K, J, I = np.meshgrid(rng[2], rng[1], rng[0], indexing="ij")
        idx = [I.reshape(-1), J.reshape(-1), K.reshape(-1)]   # ascending flat voxel index
        nb = [x.copy() for x in idx]
        nb[axis] = nb[axis] + 1
        s0, s1 = inside[idx[2], idx[1], idx[0]], inside[nb[2], nb[1], nb[0]]
        cells = []
        for d1, d2 in ((-1, -1), (0, -1), (0, 0), (-1, 0)):   # around the edge, from a1 towards a2: the normal is +axis
            c = [x.copy() for x in idx]
            c[a1] = c[a1] + d1
            c[a2] = c[a2] + d2
            cells.append(vid[c[2], c[1], c[0]])
        q = np.stack(cells, axis=1)
        use = (s0 != s1) & (q >= 0).all(axis=1)
        q, out_plus = q[use], s0[use]                          # inside end first: the normal points along +axis
        q = np.where(out_plus[:, None], q, q[:, [0, 3, 2, 1]])
        faces.append(np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3))
    faces = np.concatenate(faces).astype(np.int32) if faces else np.zeros((0, 3), np.int32)
    return vertices, faces, colors


def orbit_cameras(center, radius: float, n_azimuth: int, elevations_deg: Sequence[float], up=(0.0, 0.0, 1.0)) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Cameras on rings around ``center`` that look at it: for every elevation (degrees above the plane normal to ``up``) ``n_azimuth``
    positions at ``radius``, as ``[(wxyz, position), ...]`` (camera-to-world, OpenCV axes: +z forward, +y down) -- the form
    ``SplatScene``'s camera calls take.  Elevations within 0.5 degrees of the poles are refused (the image's up is undefined there)."""
    c = np.asarray(center, np.float64).reshape(3)
    u = np.asarray(up, np.float64).reshape(3)
    if not np.linalg.norm(u) > 0 or not radius > 0 or n_azimuth < 1:
        raise ValueError("orbit_cameras needs an up vector, a radius > 0 and n_azimuth >= 1")
    u = u / np.linalg.norm(u)
    e1 = np.cross(u, [1.0, 0.0, 0.0] if abs(u[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    cams = []
    for el in elevations_deg:
        if abs(float(el)) > 89.5:
            raise ValueError(f"elevation {el}: must be within +-89.5 degrees")
        e = np.deg2rad(float(el))
        for a in range(int(n_azimuth)):
            az = 2.0 * np.pi * a / int(n_azimuth)
            d = np.cos(e) * (np.cos(az) * e1 + np.sin(az) * e2) + np.sin(e) * u   # centre -> camera
            z = -d                                               # forward
            x = np.cross(z, u)
            x /= np.linalg.norm(x)                               # right
            y = np.cross(z, x)                                   # down
            cams.append((matrix_to_quat_wxyz(np.stack([x, y, z], axis=1)), c + float(radius) * d))
    return cams


def orbit_radius(half_diagonal: float, fov: float, height: int, width: int, margin: float = 1.2) -> float:
    """The distance from which a sphere of ``half_diagonal`` fits the narrower of a camera's two fields of view (``fov``: vertical,
    square pixels), times ``margin``."""
    half = min(0.5 * fov, float(np.arctan(np.tan(0.5 * fov) * width / height)))
    return margin * float(half_diagonal) / float(np.sin(half))


def cli_plan(argv: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The command line as what the run needs: the parsed arguments plus ``lo``, ``hi`` and ``dims``.  Raises SystemExit (argparse) or
    ValueError on arguments no volume can be made from, before anything touches a GPU."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m sim_a_splat_amd.reconstruct", description=__doc__.split("\n\n")[0])
    ap.add_argument("--splat", required=True, help="scene: .npz / .json scene, splatfacto config.yml, run directory or .ckpt")
    ap.add_argument("--bounds", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="the volume, scene frame")
    ap.add_argument("--voxel", type=float, required=True, help="voxel size")
    ap.add_argument("--out", required=True, help="mesh.obj to write")
    ap.add_argument("--masks-dir", help="masks directory (link_masks_global_dict.npz): the links become rows of their own")
    ap.add_argument("--rows", nargs="*", help="with --masks-dir: the rows to reconstruct (link names, 'scene' for the rest); default: everything")
    ap.add_argument("--azimuths", type=int, default=12)
    ap.add_argument("--elevations", type=float, nargs="+", default=[20.0, 50.0, 80.0])
    ap.add_argument("--radius", type=float, help="camera distance from the volume's centre (default: the volume fits the view)")
    ap.add_argument("--render-size", type=int, nargs=2, default=[240, 320], metavar=("H", "W"))
    ap.add_argument("--trunc", type=float, help="truncation distance (default: 4 voxels)")
    ap.add_argument("--min-weight", type=float, default=1.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.rows and not a.masks_dir:
        raise ValueError("--rows needs --masks-dir: without masks the scene is one row")
    if min(a.render_size) < 1 or a.azimuths < 1:
        raise ValueError("--render-size and --azimuths must be positive")
    lo, hi = np.array(a.bounds[:3]), np.array(a.bounds[3:])
    return dict(args=a, lo=lo, hi=hi, dims=volume_dims(lo, hi, a.voxel))


def split_rows(n: int, masks: Optional[Dict[str, np.ndarray]], rows: Optional[Sequence[str]]):
    """The Gaussians of a scene as named rows: ``[(name, boolean mask [n]), ...]`` -- every link mask, then ``scene`` (the rest) -- and
    the names to keep (None: all).  ValueError on a mask of the wrong length or a row that does not exist."""
    groups, rest = [], np.ones(n, bool)
    for name, m in (masks or {}).items():
        m = np.asarray(m, bool).reshape(-1)
        if m.shape[0] != n:
            raise ValueError(f"mask {name}: {m.shape[0]} entries for {n} Gaussians")
        groups.append((name, m))
        rest &= ~m
    groups.append(("scene", rest))
    names = [g[0] for g in groups]
    for r in rows or ():
        if r not in names:
            raise ValueError(f"no row named {r!r} (rows: {names})")
    return groups, (list(rows) if rows else None)


def main(argv: Optional[Sequence[str]] = None) -> int:
    import time
    from . import io, mesh_io
    from .covariance import GSplatLoader
    from .scene import SplatScene
    plan = cli_plan(argv)
    a, lo, hi = plan["args"], plan["lo"], plan["hi"]
    L = GSplatLoader.from_path(Path(a.splat))
    means = L.means.cpu().numpy()
    masks = None
    if a.masks_dir:
        d = Path(a.masks_dir)
        mfile = d / "link_masks_global_dict.npz"
        masks = io.load_link_masks(mfile if mfile.exists() else d / "link_masks_global_dict.npy")
    groups, keep = split_rows(len(means), masks, a.rows)
    scene = SplatScene(a.device)
    try:
        arr = lambda t, m: t.cpu().numpy()[m]
        for name, m in groups:
            if m.any():
                scene.add_gaussian_splats(name, arr(L.means, m), arr(L.covs, m), np.clip(arr(L.colors, m), 0, 1), arr(L.opacities, m))
        H, W = a.render_size
        radius = a.radius or orbit_radius(0.5 * float(np.linalg.norm(hi - lo)), scene.camera.fov, H, W)
        cams = orbit_cameras(0.5 * (lo + hi), radius, a.azimuths, a.elevations)
        vol = TsdfVolume(scene._raster, lo, a.voxel, dims=plan["dims"])
        t0 = time.perf_counter()
        scene.fuse_views(vol, H, W, cams, keep=keep, trunc=a.trunc)
        v, f, c = vol.extract_mesh(a.min_weight)
        dt = time.perf_counter() - t0
    finally:
        scene.close()
    mesh_io.save_obj(a.out, v, f, c)
    print(f"{len(cams)} views of {H}x{W} into {plan['dims']} voxels: {len(v)} vertices, {len(f)} faces in {dt:.2f} s")
    print(f"-> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
