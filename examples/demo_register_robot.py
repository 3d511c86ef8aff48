"""Register a robot to a splat, then segment it: the whole of the reference's match_splat.py on the committed meshes.

Two "links" -- the xarm6 base (tests/golden/xarm6_base.stl) and the T block (tests/golden/tblock_paper.obj) beside it -- stand in a
synthetic splat under a known similarity: Gaussian centres scattered around both placed meshes plus a background.  The robot's
surface is sampled (mesh_io.sample_surface), registered from a perturbed guess (register.register_similarity: every iteration's
nearest-neighbour search is Rasterizer.match_points on the GPU), and the recovered similarity makes the per-link masks
(segment.link_masks_from_meshes) a SplatHandler is built from.

    python examples/demo_register_robot.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from sim_a_splat_amd import mesh_io, poses, register, segment  # noqa: E402
from sim_a_splat_amd.handler import SplatHandler  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def main():
    rng = np.random.default_rng(0)
    base = mesh_io.weld(*mesh_io.load_stl(GOLDEN / "xarm6_base.stl"))
    block = mesh_io.load_obj(GOLDEN / "tblock_paper.obj")
    shift = np.eye(4)
    shift[:3, 3] = (0.3, 0.0, 0.0)                                   # the block stands beside the base (robot frame)
    meshes, local = [base, block], [np.eye(4), shift]
    truth = np.eye(4)
    truth[:3, :3] = 0.93 * rotation((0.3, -0.5, 0.8), 12.0)
    truth[:3, 3] = (0.21, -0.13, 0.34)

    # the robot as one surface, and the splat: centres around the placed links, and a background behind them
    verts = np.concatenate([segment.transform_vertices(v, S) for (v, _), S in zip(meshes, local)])
    faces = np.concatenate([base[1], block[1] + len(base[0])])
    on = segment.transform_vertices(mesh_io.sample_surface(verts, faces, 6000, seed=1), truth) + rng.normal(0, 0.004, (6000, 3))
    back = rng.uniform(on.min(0) - 0.5, on.max(0) + 0.5, (6000, 3))
    back = back[np.linalg.norm(back - on.mean(0), axis=1) > 0.45]
    means = np.concatenate([on, back]).astype(np.float32)

    source = mesh_io.sample_surface(verts, faces, 4000, seed=0)
    guess = register.initial_guess(source, on, scale=0.9)            # the centres of the two clouds, and a first scale
    r = Rasterizer(0)
    try:
        res = register.register_similarity(source, means, guess, max_correspondence_distance=0.2, max_iteration=80, rasterizer=r)
        T = res.transformation
        s, R, t = poses.decompose_icp(T)
        s0, R0, t0 = poses.decompose_icp(truth)
        angle = np.degrees(np.arccos(np.clip((np.trace(R @ R0.T) - 1) / 2, -1, 1)))
        print(f"registered in {res.iterations} iterations: fitness {res.fitness:.4f}, inlier rmse {res.inlier_rmse:.5f}")
        print(f"recovered scale {s:.5f} (truth {s0:.5f}), angle error {angle:.4f} deg, translation error {np.linalg.norm(t - t0):.5f}")
        masks = segment.link_masks_from_meshes(means, meshes, [T @ S for S in local], distance=0.015, rasterizer=r)
    finally:
        r.close()
    for k, m in masks.items():
        print(f"{k}: {int(m.sum())} of {len(m)} Gaussians")

    n = len(means)
    covs = np.tile(np.eye(3, dtype=np.float32) * 1e-4, (n, 1, 1))
    colors = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
    h = SplatHandler.from_arrays(means, covs, colors, np.full(n, 0.9, np.float32), masks, T, [np.eye(4)] * 2, device=0)
    try:
        centre = on.mean(0)
        cam = (np.array([1.0, 0.0, 0.0, 0.0]), centre + np.array([0.0, 0.0, -0.6]))      # looks along +z at both links
        labels, = h.render_segmentation(h.scene, [cam], [[120, 160]])
        names = h.scene.row_names()
        print("label image rows:", sorted(names[r] for r in np.unique(labels) if r != 255))
    finally:
        h.scene.close()


if __name__ == "__main__":
    main()
