#!/usr/bin/env python3
"""A sheet of Gaussians that bends: a deformable splat group beside a static scene, driven as a physics engine would drive it -- by the
moving positions of a few control nodes ("Deformation").

    python examples/demo_deform_cloth.py [--steps 200] [--sheet 40000] [--scene 100000] [--driver host|device] [--save frame.png]

The sheet (a 1 x 1 square of flat Gaussians in its own group) is bound to an 8 x 8 node grid; every step a travelling wave moves the nodes,
``deform.transforms_from_positions`` turns the positions into rigid per-node transforms, ``SplatScene.deform`` moves the resident Gaussians
in place, and a frame comes through the Door-B path (``get_render``).  Printed: the step time (transforms on the host + deform + frame),
and the largest distance between the deformed means and the analytic wave surface -- a measurement of THIS scene: 64 nodes and a blend of
four of them follow a wave of this length that closely, no more.

``--driver device``: the node positions are formed on the GPU (as a simulator that keeps its state there would hand them over) and
``SplatScene.deform_positions`` -- ``deform.NodeDriver``, one HIP kernel -- takes the place of the host's fits: nothing is read back."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sim_a_splat_amd import deform  # noqa: E402
from sim_a_splat_amd.scene import SplatScene  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402

AMPLITUDE, WAVELENGTH, SPEED = 0.08, 1.2, 0.02


def wave(x, step):
    return AMPLITUDE * np.sin(2.0 * np.pi * (x / WAVELENGTH - SPEED * step))


def static_group(n, seed=3):
    """A stand-in scene behind the sheet, as ``add_gaussian_splats`` takes it (covariances, plain colours)."""
    s = make_scene(n, seed=seed, log_scale_mean=float(np.log(0.012)))
    q = s.quats / np.linalg.norm(s.quats, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    M = R * s.scales[:, None, :]
    rgb = np.clip(0.5 + 0.2820947917738781 * s.sh[:, 0, :], 0.0, 1.0)
    return s.means * np.float32(0.6) - np.array([0.0, 0.0, 1.0], np.float32), M @ M.transpose(0, 2, 1), rgb, s.opacities


def sheet_group(n, seed=4):
    """n flat Gaussians on the square [-0.5, 0.5]^2 of the plane z = 0 (the sheet's local frame)."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 3), np.float32)
    c[:, :2] = rng.uniform(-0.5, 0.5, (n, 2))
    side = 1.5 / np.sqrt(n)
    cov = np.tile(np.diag([side * side, side * side, (0.1 * side) ** 2]).astype(np.float32), (n, 1, 1))
    stripes = 0.5 + 0.5 * np.sign(np.sin(20.0 * c[:, 0]) * np.sin(20.0 * c[:, 1]))
    rgb = np.stack([0.9 * stripes + 0.1, 0.3 + 0.0 * stripes, 0.9 - 0.8 * stripes], axis=1).astype(np.float32)
    return c, cov, rgb, np.full(n, 0.9, np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sheet", type=int, default=40_000)
    ap.add_argument("--scene", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--driver", choices=("host", "device"), default="host", help="where the node positions become transforms")
    ap.add_argument("--save", default="", help="write the last frame as a PNG (needs PIL)")
    a = ap.parse_args()

    scene = SplatScene(0, background=(0.05, 0.05, 0.08))
    scene.add_gaussian_splats("scene", *static_group(a.scene))
    cloth = scene.add_gaussian_splats("cloth", *sheet_group(a.sheet), wxyz=(np.cos(0.5), -np.sin(0.5), 0.0, 0.0), position=(0.0, 0.0, 0.3))
    nodes = deform.grid_nodes(((-0.5, -0.5, 0.0), (0.5, 0.5, 0.0)), 1.0 / 7.0)
    assert nodes.shape == (64, 3)
    bound = scene.bind_deformable(cloth, nodes, k=4)
    print(f"{a.scene} static + {a.sheet} deformable Gaussians, {nodes.shape[0]} nodes, k = 4, sigma = {bound['sigma']:.4f}")
    cam = dict(wxyz=(0.0, 1.0, 0.0, 0.0), position=(0.0, 0.0, 2.2))
    rest = scene._raster.read_scene()["means"].cpu().numpy()[a.scene:]
    times, worst = [], 0.0
    frame = None
    if a.driver == "device":
        import torch
        nodes_dev = torch.from_numpy(nodes).to(scene._raster.device)
    for step in range(a.steps):
        t0 = time.perf_counter()
        if a.driver == "device":
            moved = nodes_dev.clone()
            moved[:, 2] = AMPLITUDE * torch.sin(2.0 * np.pi * (nodes_dev[:, 0] / WAVELENGTH - SPEED * step))
            scene.deform_positions(moved)
        else:
            moved = nodes.astype(np.float64)
            moved[:, 2] = wave(moved[:, 0], step)
            scene.deform(deform.transforms_from_positions(nodes, moved, neighbours=6))
        frame = scene.get_render(a.height, a.width, **cam)
        times.append((time.perf_counter() - t0) * 1e3)
        if step % 25 == 0 or step == a.steps - 1:   # the measurement reads the scene back: outside the timed part
            now = scene._raster.read_scene()["means"].cpu().numpy()[a.scene:]
            # distance to the wave surface z = wave(x), along z at the deformed x (the surface's slope is at most 0.42)
            worst = max(worst, float(np.abs(now[:, 2] - wave(now[:, 0], step)).max()))
    t = np.array(times[min(10, len(times) - 1):])
    print(f"step (transforms on the {a.driver} + deform + {a.width} x {a.height} frame): median {np.median(t):.3f} ms, [{t.min():.3f}..{t.max():.3f}] over {t.size} steps")
    print(f"largest |z - wave(x)| of a deformed mean over the sampled steps: {worst:.4f} (amplitude {AMPLITUDE}, wavelength {WAVELENGTH}, node spacing {1 / 7:.3f}; "
          f"the sheet's means at rest spread {float(np.abs(rest[:, 2]).max()):.4f} from their plane)")
    if a.save:
        from PIL import Image
        Image.fromarray(frame).save(a.save)
        print(f"wrote {a.save}")
    scene.close()


if __name__ == "__main__":
    main()
