#!/usr/bin/env python3
"""How is the sheet bent, given pictures of it: the node transforms of a deformable splat group fitted to camera frames (DESIGN.md 3,
"Deformation": the adjoint).

    python examples/demo_fit_deformation.py [--iters 200] [--sheet 20000] [--views 4] [--step 60] [--optimizer host|device]

demo_deform_cloth.py's sheet (a 1 x 1 square of flat Gaussians bound to an 8 x 8 node grid) is put into ONE pose of its travelling wave and
rendered from a few cameras: those frames are the targets.  The sheet goes back to rest, and ``SplatScene.fit_deformation`` recovers the node
transforms from the pictures alone -- every step is a ``deform``, a ``render`` + ``render_backward`` per view, one ``deform_backward`` and a
twist update of the 64 nodes on the host.  Printed: the mean distance of the deformed means to the TRUE deformed means before and after,
and the time per step -- a measurement of THIS scene, not a guarantee: how far a fit gets depends on the texture, the views and the bend.
``--optimizer device`` keeps the twist update on the GPU (``deform.NodeOptimizer``): the rigidity term and the update are two kernels, and
nothing is read back between the first step and the last."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from demo_deform_cloth import sheet_group, wave  # noqa: E402
from sim_a_splat_amd import deform  # noqa: E402
from sim_a_splat_amd.poses import matrix_to_quat_wxyz  # noqa: E402
from sim_a_splat_amd.scene import SplatScene  # noqa: E402


def look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(wxyz, position) of a camera at ``position`` looking at ``target``: camera-to-world, OpenCV axes."""
    p = np.asarray(position, np.float64)
    z = np.asarray(target, np.float64) - p
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return tuple(matrix_to_quat_wxyz(np.stack([x, np.cross(z, x), z], axis=1))), tuple(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sheet", type=int, default=20_000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--step", type=int, default=60, help="the wave's step whose pose is the truth")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--optimizer", choices=("host", "device"), default="host", help="where the nodes' twist update runs")
    a = ap.parse_args()

    scene = SplatScene(0, background=(0.05, 0.05, 0.08))
    cloth = scene.add_gaussian_splats("cloth", *sheet_group(a.sheet))
    nodes = deform.grid_nodes(((-0.5, -0.5, 0.0), (0.5, 0.5, 0.0)), 1.0 / 7.0)
    scene.bind_deformable(cloth, nodes, k=4)
    cams = [look_at((1.2 * np.sin(t), -1.2 * np.cos(t), 1.6)) for t in np.linspace(0.0, 2.0 * np.pi, a.views, endpoint=False)]
    moved = nodes.astype(np.float64)
    moved[:, 2] = wave(moved[:, 0], a.step)
    scene.deform(deform.transforms_from_positions(nodes, moved, neighbours=6))
    images = scene.get_renders(a.height, a.width, cams).copy()
    truth = scene._raster.read_scene()["means"].cpu().numpy()
    scene.deform(deform.transforms_from_positions(nodes, nodes))
    rest = scene._raster.read_scene()["means"].cpu().numpy()
    t0 = time.perf_counter()
    res = scene.fit_deformation(images, a.height, a.width, cams, iters=a.iters, **({} if a.optimizer == "host" else {"optimizer": a.optimizer}))
    ms = (time.perf_counter() - t0) * 1e3 / max(1, len(res.history))
    after = scene._raster.read_scene()["means"].cpu().numpy()
    e0, e1 = np.linalg.norm(rest - truth, axis=1).mean(), np.linalg.norm(after - truth, axis=1).mean()
    print(f"{a.sheet} Gaussians, {nodes.shape[0]} nodes, {a.views} views of {a.width} x {a.height}, {a.iters} iterations")
    print(f"mean distance of the deformed means to the true ones: {e0:.5f} at rest -> {e1:.5f} fitted ({e1 / e0:.3f} of the start); "
          f"loss {res.history[0][1]:.3e} -> {res.loss:.3e}")
    update = "host update" if a.optimizer == "host" else "rigidity + twist step on the device"
    print(f"time per step (deform, {a.views} x (frame + backward), deform_backward, {update}): {ms:.2f} ms")
    scene.close()


if __name__ == "__main__":
    main()
