"""Per-link masks from the robot's URDF meshes: the segmentation step of the reference (match_splat.py:131-284) without open3d.

The reference poses the URDF visuals at the mask-time joint configuration, moves them by the ICP similarity, crops the Gaussian
centres to a polygon volume and asks of every cropped centre and every link mesh "inside, or within 0.015 of it?"
(``RaycastingScene.compute_occupancy / compute_distance``, :240-251).  Here the question is ``Rasterizer.query_meshes`` (a HIP
kernel; DESIGN.md 3, "Mesh queries"), the crop is ``polygon_volume_mask`` and the result is a mask over ALL Gaussians in the
caller's order -- what ``io.save_link_masks`` writes and ``SplatHandler`` reads.  The ICP registration itself is an input
(``sim_a_splat_amd.register`` makes it).

    python -m sim_a_splat_amd.segment --splat SCENE --urdf ROBOT.urdf --joint-config joint_config.npy \\
        --icp icp_transformation.npy --robot-description-dir DIR --package-name NAME --out MASKS_DIR \\
        [--polygon polygon_bounds.npy --axis-min -0.3 --axis-max 0.1 --axis Z] [--distance 0.015] [--links 7]
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np

from .rasterizer import _host

AXES = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}   # (u, v, w): the polygon's plane and the prism's axis


def polygon_volume_mask(points, polygon_xy, axis_min: float, axis_max: float, axis: str = "Z") -> np.ndarray:
    """The reference's crop volume (open3d ``SelectionPolygonVolume``, match_splat.py:138-168): bool [N], the points inside the
    prism over a polygon in the plane orthogonal to ``axis``, between ``axis_min`` and ``axis_max`` (both inclusive) along it.
    ``polygon_xy``: ``[K,2]`` in-plane coordinates, or ``[K,3]`` points as ``polygon_bounds.npy`` stores them (their in-plane
    columns are used).  Inside is even-odd: a point is in when a ray from it along +u crosses the outline an odd number of times."""
    u, v, w = AXES[axis.upper()]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    poly = np.asarray(polygon_xy, np.float64)
    poly = poly.reshape(-1, poly.shape[-1])
    if poly.shape[1] == 3:
        poly = poly[:, [u, v]]
    if poly.shape[1] != 2 or poly.shape[0] < 3:
        raise ValueError(f"polygon must be [K>=3,2] or [K,3], got {list(poly.shape)}")
    x, y = p[:, u], p[:, v]
    inside = np.zeros(len(p), bool)
    for (x0, y0), (x1, y1) in zip(poly, np.roll(poly, -1, axis=0)):
        if y0 == y1:
            continue                                    # a ray along +u never crosses an edge parallel to it
        straddles = (y0 > y) != (y1 > y)
        with np.errstate(invalid="ignore", over="ignore"):
            xc = x0 + (y - y0) * (x1 - x0) / (y1 - y0)
        inside ^= straddles & (x < xc)
    return inside & (p[:, w] >= axis_min) & (p[:, w] <= axis_max)


def transform_vertices(vertices, T) -> np.ndarray:
    """``vertices [V,3]`` under the 4x4 ``T`` (may carry scale), float64."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    return v @ T[:3, :3].T + T[:3, 3]


def link_masks_from_meshes(means, meshes, transforms, *, distance: float = 0.015, crop=None, rasterizer=None) -> Dict[str, np.ndarray]:
    """``{"link0": bool[N], ...}``: Gaussian ``i`` belongs to link k when it is in the crop and inside mesh k or closer to it than
    ``distance`` -- ``crop & ((winding_k > 0.5) | (distance_k < distance))``, match_splat.py:250.

    ``meshes``: ``[(vertices [V,3], faces [F,3]), ...]``, closed and outward-oriented for the inside test; mesh k is moved by
    ``transforms[k]`` (4x4 float64, may carry scale: ICP . FK) in float64 and rounded once.  ``means [N,3]`` and ``distance`` are in
    the moved meshes' frame and units (the splat's).  ``crop``: bool [N] (``polygon_volume_mask``) or None.  Masks of different
    links may overlap, as the reference's do.  ``rasterizer``: the ``Rasterizer`` to query with (anything with its
    ``query_meshes``); None makes one on device 0 for the call."""
    pts = np.ascontiguousarray(_host(means), dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    if len(meshes) != len(transforms):
        raise ValueError(f"{len(meshes)} meshes, {len(transforms)} transforms")
    keep = np.ones(n, bool) if crop is None else np.asarray(_host(crop), bool).reshape(-1)
    if keep.shape[0] != n:
        raise ValueError(f"crop must be bool [{n}], got {keep.shape[0]}")
    moved = [(transform_vertices(v, T), np.asarray(f, np.int64).reshape(-1, 3)) for (v, f), T in zip(meshes, transforms)]
    masks = {f"link{k}": np.zeros(n, bool) for k in range(len(moved))}
    idx = np.flatnonzero(keep)
    if len(idx) == 0 or not moved:
        return masks
    own = rasterizer is None
    if own:
        from .rasterizer import Rasterizer
        rasterizer = Rasterizer(0)
    try:
        res = rasterizer.query_meshes(pts[idx], moved, max_distance=float(distance))
        d, w = _host(res["distance"]), _host(res["winding"])
    finally:
        if own:
            rasterizer.close()
    for k in range(len(moved)):
        masks[f"link{k}"][idx] = (w[k] > 0.5) | (d[k] < distance)
    return masks


def robot_link_meshes(urdf_path, joint_config, icp_transformation, robot_description_dir: str, package_name: str, n_links: int = 7):
    """(meshes, transforms) of the robot's first ``n_links`` visual meshes (match_splat.py:64-85, :235-236): meshes as
    ``handler.robot_visual_meshes`` reads them (links in URDF order), welded; transforms = ICP . FK of each visual at
    ``joint_config`` (``urdf_fk.visual_mesh_fk``, matched to the meshes visual by visual)."""
    from . import mesh_io, urdf_fk
    from .handler import robot_visual_meshes
    robot = urdf_fk.load(urdf_path)
    fk = urdf_fk.visual_mesh_fk(robot, joint_config)
    with_mesh = lambda links: [(l, k) for l in links for k, v in enumerate(robot.visuals[l]) if v.mesh]
    by_visual = dict(zip(with_mesh(robot.fk_link_order or robot.links), fk))
    icp = np.asarray(icp_transformation, np.float64).reshape(4, 4)
    transforms = [icp @ by_visual[key] for key in with_mesh(robot.links)][:n_links]
    vis = robot_visual_meshes(robot, robot_description_dir, package_name, Path(str(urdf_path)).parent)[:n_links]
    return [mesh_io.weld(v, f) for v, f, _ in vis], transforms


def segment_robot(means, urdf_path, joint_config, icp_transformation, robot_description_dir: str, package_name: str,
                  n_links: int = 7, **kw) -> Dict[str, np.ndarray]:
    """The per-link masks of a splat (``means [N,3]``) from the robot's URDF: ``link_masks_from_meshes`` (whose keywords ``kw``
    are) of ``robot_link_meshes``."""
    meshes, transforms = robot_link_meshes(urdf_path, joint_config, icp_transformation, robot_description_dir, package_name, n_links)
    return link_masks_from_meshes(means, meshes, transforms, **kw)


def masks_from_votes(votes, seen, names: Sequence[str], *, min_share: float = 0.5, min_seen: int = 0) -> Dict[str, np.ndarray]:
    """``{name: bool[N]}`` from the sums of ``Rasterizer.lift_labels``: ``votes [N,G]`` and ``seen [N]`` (int64; arrays or tensors),
    ``names [G]``.  Gaussian ``i`` belongs to label ``g`` when ``g`` is the lowest index that reaches ``max_k votes[i,k]`` and
    ``votes[i,g] >= min_share * seen[i]``, ``seen[i] > min_seen`` and ``votes[i,g] > 0``: a Gaussian no labelled pixel showed, or
    one seen mostly through unlabelled pixels, belongs to nobody.  The masks are disjoint by construction and are what
    ``io.save_link_masks``, ``write_masks_dir`` and ``SplatHandler.from_arrays(link_masks=...)`` take.  For objects without a mesh
    (the masks of ``segment_robot`` need one): label a few images, lift them, threshold here."""
    v = np.asarray(_host(votes), np.int64)
    s = np.asarray(_host(seen), np.int64).reshape(-1)
    names = list(names)
    if v.ndim != 2 or v.shape[0] != s.shape[0] or v.shape[1] != len(names):
        raise ValueError(f"votes must be [N,{len(names)}] beside seen [N], got {list(v.shape)} and {list(s.shape)}")
    if len(set(names)) != len(names):
        raise ValueError("label names must be distinct")
    if not names:
        return {}
    arg = v.argmax(axis=1)   # (the first index of the maximum: ties go to the lowest label)
    top = v[np.arange(len(s)), arg]
    own = (top > 0) & (s > int(min_seen)) & (top >= float(min_share) * s)
    return {name: own & (arg == g) for g, name in enumerate(names)}


def lift_label_views(rasterizer, viewmats, Ks, W: int, H: int, label_images, n_labels: int, views_per_call: int = 8):
    """``Rasterizer.lift_labels`` over a long list of views, ``views_per_call`` at a time, into ONE pair of buffers: returns
    ``{"votes": int64 [N,n_labels], "seen": int64 [N]}`` (device tensors).  ``viewmats [C,4,4]``, ``Ks [C,3,3]``,
    ``label_images [C,H,W]`` uint8 (an array, a tensor, or a sequence of ``[H,W]`` images).  Integer sums: the result does not
    depend on ``views_per_call``."""
    V = np.asarray(_host(viewmats), np.float32).reshape(-1, 4, 4)
    K = np.asarray(_host(Ks), np.float32).reshape(-1, 3, 3)
    C = V.shape[0]
    if K.shape[0] != C or len(label_images) != C:
        raise ValueError(f"{C} view matrices, {K.shape[0]} intrinsics, {len(label_images)} label images")
    if C == 0 or views_per_call < 1:
        raise ValueError("lift_label_views needs at least one view and views_per_call >= 1")
    out = None
    for a in range(0, C, int(views_per_call)):
        b = min(C, a + int(views_per_call))
        lab = label_images[a:b]
        if not hasattr(lab, "shape"):   # a sequence of images
            lab = np.stack([np.asarray(_host(x), np.uint8) for x in lab])
        out = rasterizer.lift_labels(V[a:b], K[a:b], W, H, lab, n_labels, **(out or {}))
    return out


def load_means(path) -> np.ndarray:
    """Gaussian centres [N,3] of a scene file: an ``.npy`` of centres, or whatever ``GSplatLoader.from_path`` reads."""
    p = Path(path)
    if p.suffix == ".npy":
        return np.asarray(np.load(p, allow_pickle=False), np.float32).reshape(-1, 3)
    from .covariance import GSplatLoader
    return GSplatLoader.from_path(p).means.cpu().numpy()


def write_masks_dir(out_dir, masks: Dict[str, np.ndarray], joint_config, icp_transformation) -> Path:
    """The masks directory ``SplatHandler``'s path constructor reads: ``link_masks_global_dict.npz``, ``joint_config.npy`` and
    ``icp_transformation.npy``."""
    from . import io
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    io.save_link_masks(d / "link_masks_global_dict.npz", masks)
    np.save(d / "joint_config.npy", np.asarray(joint_config, np.float64).reshape(-1))
    np.save(d / "icp_transformation.npy", np.asarray(icp_transformation, np.float64).reshape(4, 4))
    return d


def main(argv: Optional[Sequence[str]] = None) -> int:
    import argparse
    from . import io
    ap = argparse.ArgumentParser(prog="python -m sim_a_splat_amd.segment", description=__doc__.split("\n\n")[0])
    ap.add_argument("--splat", required=True, help="scene: .npy of centres, .npz / .json scene, splatfacto config.yml, run directory or .ckpt")
    ap.add_argument("--urdf", required=True)
    ap.add_argument("--joint-config", required=True, help=".npy, or comma-separated joint positions")
    ap.add_argument("--icp", required=True, help="icp_transformation.npy (4x4 similarity)")
    ap.add_argument("--robot-description-dir", required=True, help="what package://NAME in the URDF's mesh filenames stands for")
    ap.add_argument("--package-name", required=True)
    ap.add_argument("--out", required=True, help="masks directory to write")
    ap.add_argument("--links", type=int, default=7)
    ap.add_argument("--distance", type=float, default=0.015)
    ap.add_argument("--polygon", help="polygon_bounds.npy of the crop volume (default: no crop)")
    ap.add_argument("--axis", default="Z")
    ap.add_argument("--axis-min", type=float, default=-np.inf)
    ap.add_argument("--axis-max", type=float, default=np.inf)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    means = load_means(a.splat)
    jc = io.load_joint_config(a.joint_config) if Path(a.joint_config).exists() else np.array([float(x) for x in a.joint_config.split(",")])
    icp = io.load_icp_transformation(a.icp)
    crop = polygon_volume_mask(means, np.load(a.polygon, allow_pickle=False), a.axis_min, a.axis_max, a.axis) if a.polygon else None
    from .rasterizer import Rasterizer
    r = Rasterizer(a.device)
    try:
        masks = segment_robot(means, a.urdf, jc, icp, a.robot_description_dir, a.package_name, a.links, distance=a.distance,
                              crop=crop, rasterizer=r)
    finally:
        r.close()
    d = write_masks_dir(a.out, masks, jc, icp)
    for k, m in masks.items():
        print(f"{k}: {int(m.sum())} of {len(m)} Gaussians")
    print(f"-> {d}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
