#!/usr/bin/env python3
"""A fixed-size point cloud in the observation: the synthetic env of examples/demo_synthetic_env.py with
``obs_modes=("rgb", "pointcloud")`` -- two 240x320 cameras, every step one cloud of 1024 points (xyz in the robot's frame, rgb in 0..1)
cropped to a workspace box, thinned on a 5 mm grid and cut by farthest-point sampling, all on the GPU ("Point clouds").
Prints the counts and bounds of a step's cloud.

    python examples/demo_point_cloud_obs.py [--steps 50] [--points 1024] [--save cloud.npy]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from demo_synthetic_env import N_LINKS, SwingingArmEnv  # noqa: E402
from sim_a_splat_amd.covariance import GSplatLoader  # noqa: E402
from sim_a_splat_amd.env_wrapper import SplatEnvWrapper  # noqa: E402
from sim_a_splat_amd.handler import SplatHandler  # noqa: E402
from sim_a_splat_amd.poses import SE3  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402

# the workspace, in the robot's frame (the stand-in's ICP is the identity): the part of the scene's front the cameras see from z = 3,
# sized so that the 5 mm grid stays within the contract's 2^24 cells (240 x 240 x 180)
BOUNDS = ([-0.6, -0.6, 0.2], [0.6, 0.6, 1.1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--n", type=int, default=113_831)
    ap.add_argument("--save", type=str, default="")
    a = ap.parse_args()
    sc = make_scene(a.n, seed=2, n_groups=N_LINKS + 1)
    L = GSplatLoader.from_arrays(sc.means, sc.quats, np.log(sc.scales), sc.sh[:, 0], np.log(sc.opacities / (1 - sc.opacities)))
    masks = {f"link{i}": sc.group_id == i + 1 for i in range(N_LINKS)}
    handler = SplatHandler.from_arrays(L.means.numpy(), L.covs.numpy(), np.clip(L.colors.numpy(), 0, 1), L.opacities.numpy(),
                                       masks, np.eye(4), [np.eye(4)] * N_LINKS, device=0)
    env = SplatEnvWrapper(SwingingArmEnv(), splat_handler=handler, obs_modes=("rgb", "pointcloud"),
                          point_cloud=dict(n_points=a.points, bounds=BOUNDS, voxel_size=0.005, stride=1, keep=None, frame="robot"))
    env._configure_cameras({
        0: {"link_name": "world", "local_frame": SE3(wxyz_xyz=np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 3.0])), "type": "viewport",
            "render_size": [240, 320]},
        1: {"link_name": "link6", "local_frame": SE3(wxyz_xyz=np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.2, 2.5])), "type": "moving",
            "render_size": [240, 320]},
    })
    env.reset()
    obs = None
    for _ in range(5):
        obs, *_ = env.step(None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        obs, *_ = env.step(None)
    dt = time.perf_counter() - t0
    pc = obs["point_cloud"]
    cams, sizes = env._render_cameras()
    o = handler.render_point_cloud(env.ch, cams, sizes, a.points, frame="robot", bounds=BOUNDS, voxel_size=0.005)
    M = int(o["count"][0])
    k = min(a.points, M)
    rows = np.unique(o["labels"][0, :k].cpu().numpy())
    names = env.ch.row_names()
    print(f"{a.steps / dt:.0f} env steps/s with obs keys {list(obs)}")
    print(f"point_cloud {pc.shape} {pc.dtype}: {M} survivors behind crop and grid, {k} picked, {a.points - k} padding rows")
    print(f"  xyz min {pc[:k, :3].min(0).round(3).tolist()} max {pc[:k, :3].max(0).round(3).tolist()} (bounds {BOUNDS}); "
          f"rgb mean {pc[:k, 3:].mean(0).round(3).tolist()}")
    print(f"  rows seen: {[names[r] for r in rows if r != 255]}")
    if a.save:
        np.save(a.save, pc)
    env.close()


if __name__ == "__main__":
    main()
