#!/usr/bin/env python3
"""A mesh from the splat: a synthetic capture -- an ellipsoidal object of 6 000 Gaussians standing on a table of 20 000 -- whose object
group is reconstructed as a triangle mesh: label frames from an orbit of 36 cameras, TSDF fusion of their depth on the GPU, surface nets on
the host ("Depth fusion").  The table's pixels and the background only carve.  Prints the vertex and face counts, the time,
and how far the vertices lie from the ellipsoid the Gaussians were drawn on; then hands the mesh back to the library (a winding-number
query: which Gaussians does the mesh contain?).

    python examples/demo_reconstruct_mesh.py [--voxel 0.004] [--save mesh.obj]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sim_a_splat_amd import mesh_io  # noqa: E402
from sim_a_splat_amd.handler import SplatHandler  # noqa: E402

CENTRE, AXES = np.array([0.1, 0.0, 0.1]), np.array([0.12, 0.08, 0.10])


def capture(seed=0, n_object=6000, n_table=20000, sigma=0.004):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_object, 3))
    obj = CENTRE + AXES * d / np.linalg.norm(d, axis=1, keepdims=True)
    table = np.stack([rng.uniform(-0.6, 0.6, n_table), rng.uniform(-0.6, 0.6, n_table), np.zeros(n_table)], axis=1)
    means = np.concatenate([obj, table]).astype(np.float32)
    n = len(means)
    covs = np.broadcast_to((sigma ** 2 * np.eye(3)).astype(np.float32), (n, 3, 3)).copy()
    colors = np.where((np.arange(n) < n_object)[:, None], [0.8, 0.3, 0.2], [0.5, 0.5, 0.55]).astype(np.float32)
    return means, covs, colors, np.full(n, 0.95, np.float32), {"link0": np.arange(n) < n_object}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--save", type=str, default="")
    a = ap.parse_args()
    means, covs, colors, opacities, masks = capture()
    handler = SplatHandler.from_arrays(means, covs, colors, opacities, masks, np.eye(4), [np.eye(4)], device=0)
    row = "robot/splat_robot/link0"
    bounds = (CENTRE - AXES - 0.03, CENTRE + AXES + 0.03)
    handler.reconstruct_mesh([row], bounds, a.voxel, n_azimuth=4, elevations=(30,), render_size=(120, 160))      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = handler.reconstruct_mesh([row], bounds, a.voxel)
    dt = time.perf_counter() - t0
    v, f, c = m["vertices"], m["faces"], m["colors"]
    print(f"{row}: {int(masks['link0'].sum())} of {len(means)} Gaussians, bounds {np.round(bounds, 3).tolist()}, voxel {a.voxel}")
    print(f"mesh: {len(v)} vertices, {len(f)} faces in {1e3 * dt:.1f} ms (36 views of 240x320: label frames, fusion, extraction)")
    if len(f):
        r = np.linalg.norm((v - CENTRE) / AXES, axis=1)
        err = np.abs(r - 1.0) * AXES.mean() / a.voxel
        print(f"  vertices against the ellipsoid: median {np.median(err):.2f} voxel, 95 % within {np.percentile(err, 95):.2f} voxel; "
              f"mean colour {c.mean(0).round(1).tolist()}")
        q = handler.scene._raster.query_meshes(means, [(v, f)], max_distance=0.02)
        inside = (q["winding"][0].cpu().numpy() > 0.5)
        print(f"  winding number against the mesh: {int(inside[masks['link0']].sum())} object and {int(inside[~masks['link0']].sum())} table Gaussians inside")
    if a.save:
        mesh_io.save_obj(a.save, v, f, c)
        print(f"-> {a.save}")
    handler.scene.close()


if __name__ == "__main__":
    main()
