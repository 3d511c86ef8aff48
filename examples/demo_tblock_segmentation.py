#!/usr/bin/env python3
"""A label image and a point cloud of a scene that holds the pushT T-block as a triangle mesh (tests/golden/tblock_paper.obj):
two splat groups and the block on pose rows of their own, through the viser-style `SplatScene`.

    python examples/demo_tblock_segmentation.py [--out-dir .]

Writes `labels.npy` (uint8 [H,W]: the pose row each pixel shows, 255 for none; the names are printed) and `cloud.ply` (ASCII:
camera-frame points with colours).  The depth comes from `get_render_float(..., mesh_surface=True)`: without the flag the depth
of a pixel that shows the block is that of the splats in front of it, and the cloud has a hole where the block is.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from sim_a_splat_amd.covariance import compute_cov, sh2rgb  # noqa: E402
from sim_a_splat_amd.mesh_io import load_obj  # noqa: E402
from sim_a_splat_amd.scene import SplatScene  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=".")
    a = ap.parse_args()
    out = Path(a.out_dir)
    H, W = 240, 320
    s = make_scene(20000, seed=3, log_scale_mean=float(np.log(0.03)))
    covs = compute_cov(torch.from_numpy(s.quats), torch.from_numpy(s.scales)).numpy()
    cols = np.clip(sh2rgb(torch.from_numpy(s.sh[:, 0])).numpy(), 0, 1)
    arm = s.means[:, 0] > 0.3                                          # a stand-in for a link's mask
    scene = SplatScene(device=0)
    scene.add_gaussian_splats("arm", s.means[arm], covs[arm], cols[arm], s.opacities[arm])
    scene.add_gaussian_splats("table", s.means[~arm], covs[~arm], cols[~arm], s.opacities[~arm])
    v, f = load_obj(ROOT / "tests" / "golden" / "tblock_paper.obj")
    scene.add_mesh_simple("tblock", v, f, color=(0.45, 0.5, 0.55), scale=8.0, position=(-0.3, 0.2, -1.2))
    wxyz, pos = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, -3.0])   # camera-to-world, OpenCV axes: looking along +z
    seg = scene.get_segmentation(H, W, wxyz, pos)
    labels = seg["labels"].cpu().numpy()
    names = scene.row_names()
    for row in np.unique(labels):
        print(f"label {row:3d} {'(none)' if row == 255 else names[row]:8s} {100 * (labels == row).mean():5.1f} % of the frame")
    np.save(out / "labels.npy", labels)
    fr = scene.get_render_float(H, W, wxyz, pos, mesh_surface=True)
    depth, alpha, rgb = fr["depth"].cpu().numpy()[..., 0], fr["alpha"].cpu().numpy()[..., 0], fr["rgb"].cpu().numpy()
    # get_render's camera: vertical field of view, square pixels, principal point at the image centre
    focal = 0.5 * H / np.tan(0.5 * scene.camera.fov)
    ys, xs = np.mgrid[0:H, 0:W]
    keep = alpha > 0.5
    pts = np.stack([(xs - 0.5 * W) * depth / focal, (ys - 0.5 * H) * depth / focal, depth], -1)[keep]
    c8 = np.round(rgb[keep] * 255).astype(np.uint8)
    with open(out / "cloud.ply", "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        for p, c in zip(pts, c8):
            fh.write(f"{p[0]:.5f} {p[1]:.5f} {p[2]:.5f} {c[0]} {c[1]} {c[2]}\n")
    print(f"{len(pts)} points, {int((labels[keep] == names.index('tblock')).sum())} of them on the block -> {out / 'cloud.ply'}, {out / 'labels.npy'}")
    scene.close()


if __name__ == "__main__":
    main()
