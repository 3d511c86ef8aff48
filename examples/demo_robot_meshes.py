#!/usr/bin/env python3
"""The robot's visual meshes in the Gym cameras, flat against smooth: a stand-in scene, three procedural links handed to
`SplatHandler.from_arrays(meshes={"robot": [...]})` and posed by a draw message, two 240x320 cameras.

    python examples/demo_robot_meshes.py [--out-dir .]

Writes `robot_meshes.npy` (uint8 [2 H, 2 W, 3]: the two cameras side by side, the handler's smooth-shaded links above, the same
meshes flat-shaded below) and, when Pillow is installed, `robot_meshes.png`.  A handler draws the links smooth, as the
reference hands viser vertex normals; the flat row is the same scene with its vertex attributes cleared.
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
from sim_a_splat_amd.handler import SplatHandler  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402


def link(r, length, nu=24, nv=16):
    """An ellipsoid about the z axis as a triangle soup (three private vertices per facet, as an STL stores a mesh)."""
    th = np.pi * np.arange(nv + 1) / nv
    ph = 2.0 * np.pi * np.arange(nu + 1) / nu
    p = np.stack([r * np.outer(np.sin(th), np.cos(ph)), r * np.outer(np.sin(th), np.sin(ph)), 0.5 * length * np.outer(np.cos(th), np.ones(nu + 1))], -1)
    quads = [(p[i, j], p[i + 1, j], p[i + 1, j + 1], p[i, j + 1]) for i in range(nv) for j in range(nu)]
    v = np.array([c for a, b, c_, d in quads for c in (a, b, c_, a, c_, d)])
    return v, np.arange(len(v)).reshape(-1, 3)


class Msg:
    def __init__(self, robot_num, quaternion, position):
        self.num_links, self.robot_num, self.quaternion, self.position = len(robot_num), robot_num, quaternion, position


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=".")
    a = ap.parse_args()
    H, W = 240, 320
    s = make_scene(2500, seed=3, log_scale_mean=float(np.log(0.015)))
    covs = compute_cov(torch.from_numpy(s.quats), torch.from_numpy(s.scales)).numpy()
    cols = np.clip(sh2rgb(torch.from_numpy(s.sh[:, 0])).numpy(), 0, 1)
    masks = {"link0": s.means[:, 0] < -0.6, "link1": s.means[:, 0] > 0.6, "link2": np.abs(s.means[:, 1]) > 0.8}
    masks["link2"] &= ~(masks["link0"] | masks["link1"])
    links = [(*link(0.22, 0.9), (0.75, 0.75, 0.78)), (*link(0.17, 1.0), (0.9, 0.35, 0.2)), (*link(0.13, 0.8), (0.2, 0.45, 0.85))]
    h = SplatHandler.from_arrays(s.means, covs, cols, s.opacities, masks, np.eye(4), [np.eye(4)] * 3, device=0, meshes={"robot": links})
    tilt = lambda ang: np.array([np.cos(ang / 2), np.sin(ang / 2), 0.0, 0.0])
    h.draw_handler(Msg([3, 3, 3], [tilt(0.3), tilt(1.2), tilt(2.0)], [(-0.7, 0.0, -1.0), (0.0, 0.1, -0.6), (0.7, 0.0, -0.2)]))
    cams = [(np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, -2.2])), (tilt(-0.35), np.array([0.2, -0.8, -2.0]))]
    smooth = np.concatenate(h.render(h.scene, cams, [[H, W]] * 2), axis=1)
    h.scene._raster.upload_mesh_vertex_attributes(None, None)          # the same meshes, one shade per triangle
    flat = np.concatenate(h.render(h.scene, cams, [[H, W]] * 2), axis=1)
    h.scene.close()
    img = np.concatenate([smooth, flat], axis=0)
    out = Path(a.out_dir)
    np.save(out / "robot_meshes.npy", img)
    try:
        from PIL import Image
        Image.fromarray(img).save(out / "robot_meshes.png")
    except ImportError:
        pass
    diff = np.abs(smooth.astype(int) - flat.astype(int))
    print(f"{h.scene.row_names()[4:]}: {int((diff.max(-1) > 0).sum())} pixels differ between smooth and flat, by at most {int(diff.max())} / 255")


if __name__ == "__main__":
    main()
