#!/usr/bin/env python3
"""Per-link masks made here instead of read: a fabricated splat holds the pushT T-block (tests/golden/tblock_paper.obj) and the
xarm6 base link (tests/golden/xarm6_base.stl) as clouds of Gaussians in front of a background; `link_masks_from_meshes` asks the
GPU which Gaussians lie inside a mesh or within 0.015 of it, the masks build a `SplatHandler`, and one label image shows the result.

    python examples/demo_segment_links.py [--out-dir .]

Writes `link_masks_global_dict.npz` (what `SplatHandler`'s path constructor reads from a masks directory) and `segmentation.ppm`
(one colour per link, grey for the rest of the scene, black where nothing shows).  With a real robot the meshes and transforms come
from the URDF: `sim_a_splat_amd.segment.segment_robot`, or `python -m sim_a_splat_amd.segment`.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from sim_a_splat_amd import io, mesh_io, segment  # noqa: E402
from sim_a_splat_amd.handler import SplatHandler  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
PALETTE = np.array([[230, 60, 60], [60, 110, 230], [120, 120, 120]], np.uint8)   # link0, link1, the rest


def around(vertices, faces, n, sigma, rng):
    """n points on randomly drawn triangles plus normal(0, sigma)."""
    tri = vertices[faces[rng.integers(0, len(faces), n)]]
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    return (tri * b[:, :, None]).sum(axis=1) + rng.normal(0.0, sigma, (n, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=".")
    a = ap.parse_args()
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(1)
    icp = np.load(GOLDEN / "scene_assets_xarm6_1.npz")["icp_transformation"].astype(np.float64)   # robot frame -> splat frame, scale 0.55
    beside = np.eye(4)
    beside[:3, 3] = (0.35, 0.0, 0.0)                                   # the block lies 0.35 m beside the base, in the robot's frame
    meshes = [mesh_io.load_obj(GOLDEN / "tblock_paper.obj"), mesh_io.weld(*mesh_io.load_stl(GOLDEN / "xarm6_base.stl"))]
    transforms = [icp @ beside, icp]
    placed = [segment.transform_vertices(v, T) for (v, _), T in zip(meshes, transforms)]
    lo, hi = np.minimum(*[p.min(0) for p in placed]) - 0.3, np.maximum(*[p.max(0) for p in placed]) + 0.3
    lo[2] = hi[2] - 0.2                                                  # a wall behind both (+z)
    means = np.concatenate([around(placed[0], meshes[0][1], 4000, 0.006, rng), around(placed[1], meshes[1][1], 8000, 0.006, rng),
                            rng.uniform(lo, hi, (8000, 3))]).astype(np.float32)
    n = len(means)
    masks = segment.link_masks_from_meshes(means, meshes, transforms, distance=0.015)
    for k, m in masks.items():
        print(f"{k}: {int(m.sum())} of {n} Gaussians")
    io.save_link_masks(out / "link_masks_global_dict.npz", masks)
    covs = np.tile(np.eye(3, dtype=np.float32) * 4e-5, (n, 1, 1))
    colors = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
    h = SplatHandler.from_arrays(means, covs, colors, np.full(n, 0.9, np.float32), masks, icp, [np.eye(4)] * len(masks), device=0)
    centre = 0.5 * (placed[0].mean(0) + placed[1].mean(0))
    cam = (np.array([1.0, 0.0, 0.0, 0.0]), centre + np.array([0.0, 0.0, -0.5]))   # camera-to-world, OpenCV axes: looking along +z
    labels, = h.render_segmentation(h.scene, [cam], [[240, 320]])
    names = h.scene.row_names()
    for row in np.unique(labels):
        print(f"label {row:3d} {'(none)' if row == 255 else names[row]:28s} {100 * (labels == row).mean():5.1f} % of the frame")
    img = np.zeros(labels.shape + (3,), np.uint8)
    for row in range(len(names)):
        img[labels == row] = PALETTE[min(row, len(PALETTE) - 1)]
    with open(out / "segmentation.ppm", "wb") as fh:
        fh.write(f"P6\n{img.shape[1]} {img.shape[0]}\n255\n".encode() + img.tobytes())
    print(f"-> {out / 'link_masks_global_dict.npz'}, {out / 'segmentation.ppm'}")
    h.scene.close()


if __name__ == "__main__":
    main()
