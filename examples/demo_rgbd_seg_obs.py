#!/usr/bin/env python3
"""RGB, depth and segmentation per camera from `step()`: the synthetic env of examples/demo_synthetic_env.py (the
113,831-Gaussian stand-in for `robots-scene-v2`, 7 link groups, two 240x320 cameras) with
`SplatEnvWrapper(..., obs_modes=("rgb", "depth", "segmentation"))`.  All three modalities of both cameras come from one
label-frame call per step (sas_render_batch_labels); the labels index `env.ch.row_names()`, 255 = nothing seen.

    python examples/demo_rgbd_seg_obs.py [--steps 50]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path[:0] = [str(Path(__file__).resolve().parent.parent), str(Path(__file__).resolve().parent)]

from demo_synthetic_env import N_LINKS, SwingingArmEnv  # noqa: E402
from sim_a_splat_amd.covariance import GSplatLoader  # noqa: E402
from sim_a_splat_amd.env_wrapper import SplatEnvWrapper  # noqa: E402
from sim_a_splat_amd.handler import SplatHandler  # noqa: E402
from sim_a_splat_amd.poses import SE3  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402

MODES = ("rgb", "depth", "segmentation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    sc = make_scene(113_831, seed=2, n_groups=N_LINKS + 1)            # group 0 = static scene
    L = GSplatLoader.from_arrays(sc.means, sc.quats, np.log(sc.scales), sc.sh[:, 0], np.log(sc.opacities / (1 - sc.opacities)))
    masks = {f"link{i}": sc.group_id == i + 1 for i in range(N_LINKS)}
    handler = SplatHandler.from_arrays(L.means.numpy(), L.covs.numpy(), np.clip(L.colors.numpy(), 0, 1), L.opacities.numpy(),
                                       masks, np.eye(4), [np.eye(4)] * N_LINKS, device=0)
    env = SplatEnvWrapper(SwingingArmEnv(), splat_handler=handler, obs_modes=MODES)
    env._configure_cameras({
        0: {"link_name": "world", "local_frame": SE3(wxyz_xyz=np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 3.0])), "type": "viewport",
            "render_size": [240, 320]},
        1: {"link_name": "link6", "local_frame": SE3(wxyz_xyz=np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.2, 2.5])), "type": "moving",
            "render_size": [240, 320]},
    })
    env.reset()
    obs, *_ = env.step(None)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        obs, *_ = env.step(None)
    dt = time.perf_counter() - t0
    names = env.ch.row_names()
    print(f"{a.steps / dt:.0f} env steps/s with {MODES}; obs keys {list(obs)}")
    for i in range(2):
        rgb, depth, seg = obs[f"camera_{i}"], obs[f"camera_{i}_depth"], obs[f"camera_{i}_segmentation"]
        print(f"camera_{i}: rgb {rgb.shape} {rgb.dtype}, depth {depth.shape} {depth.dtype} (max {depth.max():.2f}), "
              f"segmentation {seg.shape} {seg.dtype}")
        count = np.bincount(seg.reshape(-1), minlength=256)
        for row in np.nonzero(count)[0]:
            print(f"    {names[row] if row < len(names) else 'nothing':32s} {count[row]:6d} px")
    env.close()


if __name__ == "__main__":
    main()
