"""What the robot's visual meshes cost a frame: the Door-B stand-in scene (113 831 Gaussians, 8 groups), the two 240x320 Gym cameras
and one 1920x1080 frame, with

    --meshes none     no meshes (the lazy path; the full-sort frame of the same views is timed beside it: k_blend)
    --meshes task     the T-block, flat: the task mesh Door B draws today
    --meshes flat     a procedural robot of about 55 k triangles (seven tessellated links, one pose row each), flat-shaded
    --meshes smooth   the same robot with vertex normals and colours (rule 2b)

    python tools/robot_mesh_probe.py --meshes flat [--reps 30]

Prints one JSON line: the blocking Gym step (poses + both cameras to pinned host memory), the blocking 1080p frame, the mesh
counters.  Kernel times come from a run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/robot_mesh_probe.py --meshes flat
The flat arm uses nothing newer than upload_meshes, so the same file measures an older checkout.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests" / "tools")]
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import NERFSTUDIO_EVAL_BACKGROUND as BG, make_scene, random_group_poses, ring_camera  # noqa: E402


def link(r, length, nu, nv):
    """A capsule-like link about the z axis: a UV sphere of radius r stretched to `length`; 2 nu (nv - 1) triangles, shared vertices,
    unit normals of the stretched surface."""
    th = np.pi * np.arange(1, nv) / nv
    ph = 2.0 * np.pi * np.arange(nu) / nu
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nu))], -1)
    n = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    at = lambda i, j: 1 + i * nu + (j % nu)
    south = 1 + nu * (nv - 1)
    tris = [[0, at(0, j), at(0, j + 1)] for j in range(nu)]
    for i in range(nv - 2):
        for j in range(nu):
            tris += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    tris += [[south, at(nv - 2, j + 1), at(nv - 2, j)] for j in range(nu)]
    s = np.array([r, r, 0.5 * length])
    nn = n / s                                                   # normal of an ellipsoid: gradient of the quadric
    return n * s, np.asarray(tris, np.int64), nn / np.linalg.norm(nn, axis=1, keepdims=True)


def robot(n_links=7, nu=64, nv=62):
    """Seven links on pose rows 1..7 along an arm through the cloud: 7 * 2 * 64 * 61 = 54 656 triangles."""
    vs, fs, ns, gs, off = [], [], [], [], 0
    for k in range(n_links):
        v, f, n = link(0.09 - 0.006 * k, 0.34, nu, nv)
        vs.append((v + np.array([0.0, 0.0, 0.3 * k - 0.9]))[:, ::-1])     # the arm lies along x, across both cameras' frames
        fs.append(f + off)
        ns.append(n[:, ::-1])
        gs.append(np.full(len(f), k + 1))
        off += len(v)
    v = np.concatenate(vs).astype(np.float32)
    rng = np.random.default_rng(4)
    return dict(verts=v, tris=np.concatenate(fs).astype(np.int32), groups=np.concatenate(gs).astype(np.uint8),
                normals=np.concatenate(ns).astype(np.float32), vcols=rng.uniform(0.3, 1.0, v.shape).astype(np.float32))


def timed_host(fn, reps):
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us)), float(np.min(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", choices=("none", "task", "flat", "smooth"), default="flat")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", choices=("both", "gym", "hd"), default="both", help="under the kernel tracer: one frame size per run")
    a = ap.parse_args()
    sc = make_scene(113_831, seed=2, n_groups=8)
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=3, group_id=sc.group_id, n_groups=8)
    row = dict(meshes=a.meshes, n=113_831, triangles=0)
    if a.meshes == "task":
        from sim_a_splat_amd.mesh_io import load_obj
        v, f = load_obj(ROOT / "tests" / "golden" / "tblock_paper.obj")
        r.upload_meshes((v * 6.0).astype(np.float32), f, (0.956, 0.396, 0.365), groups=np.full(len(f), 1, np.uint8))
        row["triangles"] = int(len(f))
    elif a.meshes != "none":
        m = robot()
        kw = dict(vertex_normals=m["normals"], vertex_colors=m["vcols"]) if a.meshes == "smooth" else {}
        r.upload_meshes(m["verts"], m["tris"], (0.7, 0.7, 0.75), groups=m["groups"], **kw)
        row["triangles"] = int(len(m["tris"]))
    cams = [ring_camera(320, 240, 262.0, yaw_deg=0.0), ring_camera(320, 240, 262.0, yaw_deg=60.0, elev=0.5)]
    V, K = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])
    poses = [random_group_poses(8, seed=s) for s in range(a.reps + 5)]
    host = torch.empty((2, 240, 320, 3), dtype=torch.uint8).pin_memory()
    step = iter(range(10 ** 9))

    def gym_step():
        r.set_group_poses(poses[next(step) % len(poses)])
        r.render_batch_host(V, K, 320, 240, BG, out=host)

    big = ring_camera(1920, 1080, 1400.0, yaw_deg=10.0)
    full = a.meshes == "none"      # frames with meshes are full-sort frames: the frame without meshes beside them is one too
    hd = lambda: r.render(big.viewmat, big.K, 1920, 1080, BG, want=("rgb8",), full_sort=full)
    if a.frames != "hd":
        timed_host(gym_step, 5)
        row["gym_step_us"], row["gym_step_min_us"] = timed_host(gym_step, a.reps)
        if full:
            gym_full = lambda: [r.render(c.viewmat, c.K, 320, 240, BG, want=("rgb8",), full_sort=True) for c in cams]
            timed_host(gym_full, 5)
            row["gym_full_sort_views_us"] = timed_host(gym_full, a.reps)[0]
    if a.frames != "gym":
        timed_host(hd, 5)
        row["hd_frame_us"], row["hd_frame_min_us"] = timed_host(hd, a.reps)
        row["hd_n_isect"] = int(r.stats()["n_isect"])
    r.close()
    print(json.dumps(row))


if __name__ == "__main__":
    main()
