#!/usr/bin/env python3
"""The rest scene of a deformable splat group from pictures of its motion ("Deformation": the adjoint to the rest arrays).

    python examples/demo_fit_dynamic.py [--iters 100] [--sheet 20000] [--views 3] [--poses 3] [--noise 0.02]

demo_deform_cloth.py's sheet (a 1 x 1 square of flat Gaussians bound to an 8 x 8 node grid) is seen in a few poses of its travelling wave, each
from a few cameras: those frames are the targets, and the poses' node transforms are known, as a simulator knows them.  (The sheet's colours
get a speckle per Gaussian on top of the demo's checks: inside a patch of one colour no picture says where a Gaussian lies.)  Then the
sheet's REST means are perturbed by noise -- a smooth random field in the sheet's plane, which neighbours share -- and its colours tinted, and ``SplatScene.fit_dynamic`` fits them back from the pictures of the bent sheet alone --
per iteration and pose a ``deform``, a ``render`` + ``render_backward`` per view and one ``deform_backward_rest``, then ONE
``adam_step(rest=True)``.  Printed: the mean distance of the rest means to the TRUE rest means and the mean colour error, before and after,
and the time per iteration -- a measurement of THIS scene, not a guarantee: how far a fit gets depends on the texture, the views, the
bends and on how much of the sheet lies under its own Gaussians."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from demo_deform_cloth import sheet_group, wave  # noqa: E402
from demo_fit_deformation import look_at  # noqa: E402
from sim_a_splat_amd import deform  # noqa: E402
from sim_a_splat_amd.scene import SplatScene  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--sheet", type=int, default=20_000)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--poses", type=int, default=3, help="poses of the wave the sheet is seen in")
    ap.add_argument("--noise", type=float, default=0.02, help="amplitude of the noise on the rest means, per axis in the sheet's plane")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    a = ap.parse_args()

    centers, cov, rgb, opac = sheet_group(a.sheet)
    rng = np.random.default_rng(8)
    rgb = np.clip(rgb + rng.uniform(-0.25, 0.25, rgb.shape), 0.0, 1.0).astype(np.float32)
    nodes = deform.grid_nodes(((-0.5, -0.5, 0.0), (0.5, 0.5, 0.0)), 1.0 / 7.0)
    cams = [look_at((1.2 * np.sin(t), -1.2 * np.cos(t), 1.6)) for t in np.linspace(0.0, 2.0 * np.pi, a.views, endpoint=False)]
    transforms = []
    for step in np.linspace(0, 90, a.poses).astype(int):
        moved = nodes.astype(np.float64)
        moved[:, 2] = wave(moved[:, 0], int(step))
        transforms.append(deform.transforms_from_positions(nodes, moved, neighbours=6))
    transforms = np.stack(transforms)

    # the targets: the TRUE sheet in every pose
    true = SplatScene(0, background=(0.05, 0.05, 0.08))
    true.bind_deformable(true.add_gaussian_splats("cloth", centers, cov, rgb, opac), nodes, k=4)
    frames = []
    for T in transforms:
        true.deform(T)
        frames.append(dict(images=true.get_renders(a.height, a.width, cams).copy(), cam_poses=cams))
    true.close()

    # the start: rest means perturbed in the sheet's plane, colours tinted
    start = centers.copy()
    for axis in range(2):
        for _ in range(2):
            start[:, axis] += a.noise * np.sin(centers[:, :2] @ rng.normal(0.0, 4.0, 2) + rng.uniform(0.0, 6.28)).astype(np.float32) / 2.0 ** 0.5
    tinted = np.clip(0.7 * rgb + np.array([0.2, -0.1, 0.1], np.float32), 0.0, 1.0).astype(np.float32)
    scene = SplatScene(0, background=(0.05, 0.05, 0.08))
    scene.bind_deformable(scene.add_gaussian_splats("cloth", start, cov, tinted, opac), nodes, k=4)
    t0 = time.perf_counter()
    res = scene.fit_dynamic(frames, a.height, a.width, what=("means", "colors"), transforms=transforms, iters=a.iters,
                            lrs=dict(means=1e-3, sh_dc=2e-2), extent=1.0)
    ms = (time.perf_counter() - t0) * 1e3 / max(1, res.steps)
    fitted, colours = scene._groups[0]["centers"], scene._groups[0]["rgbs"]
    e0, e1 = np.linalg.norm(start - centers, axis=1).mean(), np.linalg.norm(fitted - centers, axis=1).mean()
    c0, c1 = np.abs(tinted - rgb).mean(), np.abs(colours - rgb).mean()
    print(f"{a.sheet} Gaussians, {nodes.shape[0]} nodes, {a.poses} poses x {a.views} views of {a.width} x {a.height}, {a.iters} iterations")
    print(f"a measurement of that scene: mean distance of the rest means to the true ones {e0:.5f} -> {e1:.5f} ({e1 / e0:.3f} of the start); "
          f"mean colour error {c0:.4f} -> {c1:.4f}; loss {res.history[0]:.3e} -> {res.history[-1]:.3e}")
    print(f"time per iteration ({a.poses} x (deform, {a.views} x (frame + backward), deform_backward_rest), one adam_step(rest=True)): {ms:.2f} ms")
    scene.close()


if __name__ == "__main__":
    main()
