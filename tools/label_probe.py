"""What per-pixel group labels cost a vectorised rollout: the Door-B workload -- the stand-in scene (113 831 Gaussians, the static
rest + 7 link groups) with the procedural robot's meshes on the links' pose rows, 2 cameras of 240x320, E = 16 envs with distinct
pose sets: 32 views per step.

    arm A   the earlier path, per view: set_group_poses + render_group_masks (a feature frame [H,W,G] float32, then four torch
            kernels to one byte per pixel); the context drains between views
    arm B   one render_batch_labels(..., pose_sets=...) call: k_blend_labels keeps the argmax, one byte per pixel leaves the kernel

    python tools/label_probe.py [--reps 20] [--envs 16]

Both arms run in this process, alternating, after a warm-up of every shape; a step ends in a device synchronise and is timed on the
host clock; the medians are reported.  The arms' labels are compared on every pixel first.  Prints one JSON line (times in ms, the
bytes of device output a step writes, arm B's mean stage times from a timed pass of its own).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(Path(__file__).resolve().parent)]
from robot_mesh_probe import robot  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, random_group_poses, ring_camera  # noqa: E402

W, H, G = 320, 240, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--n", type=int, default=113_831)
    a = ap.parse_args()
    E = a.envs
    sc = make_scene(a.n, seed=2, n_groups=G)
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=3, group_id=sc.group_id, n_groups=G)
    m = robot()
    r.upload_meshes(m["verts"], m["tris"], (0.7, 0.7, 0.75), groups=m["groups"])
    cams = [ring_camera(W, H, 262.0, yaw_deg=0.0), ring_camera(W, H, 262.0, yaw_deg=60.0, elev=0.5)]
    V = np.stack([np.asarray(c.viewmat, np.float32) for c in cams] * E)
    K = np.stack([np.asarray(c.K, np.float32) for c in cams] * E)
    sets = np.stack([random_group_poses(G, seed=100 + e) for e in range(E)])
    pose_set = np.repeat(np.arange(E), 2).astype(np.int32)
    n_views = 2 * E
    out_b = {"labels": torch.empty((n_views, H, W), dtype=torch.uint8, device=r.device)}

    def arm_a():
        labs = []
        for v in range(n_views):
            r.set_group_poses(sets[pose_set[v]])
            labs.append(r.render_group_masks(V[v], K[v], W, H)["labels"])
        torch.cuda.synchronize()
        return labs

    def arm_b(timing=False):
        o = r.render_batch_labels(V, K, W, H, pose_sets=sets, pose_set=pose_set, out=out_b, timing=timing)["labels"]
        torch.cuda.synchronize()
        return o

    same = all(torch.equal(x, y) for x, y in zip(arm_a(), arm_b()))      # (also the first warm-up of both arms)
    for _ in range(3):
        arm_a()
        arm_b()
    ta, tb = [], []
    for _ in range(a.reps):                                              # alternating: both arms see the same machine
        t0 = time.perf_counter(); arm_a(); t1 = time.perf_counter(); arm_b(); t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    r.stage_time_means(reset=True)
    for _ in range(3):
        arm_b(timing=True)
    stages, frames = r.stage_time_means(reset=True)
    px = n_views * H * W
    row = dict(n=a.n, groups=G, triangles=int(len(m["tris"])), views=n_views, width=W, height=H, reps=a.reps, labels_equal=bool(same),
               a_ms_median=float(np.median(ta)), a_ms_min=float(np.min(ta)), b_ms_median=float(np.median(tb)), b_ms_min=float(np.min(tb)),
               a_over_b=float(np.median(ta) / np.median(tb)),
               a_device_output_bytes=px * (4 * G + 4 + 1), b_device_output_bytes=px,
               b_stage_ms_per_view={k: round(v, 4) for k, v in stages.items()}, b_timed_views=frames)
    r.close()
    print(json.dumps(row))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
