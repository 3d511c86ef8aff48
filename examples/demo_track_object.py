"""Where is the object: recover the poses of two movable splat groups from two camera pictures, through the HIP backward pass.

A synthetic scene of a static part and two movable groups (Door B: ``SplatScene.add_gaussian_splats``) is pictured by two 240x320 cameras
at the true poses; the two groups are then displaced by a few degrees and centimetres, and ``SplatScene.refine_handle_poses`` brings them
back by descending the gradient of the photometric loss with respect to their poses (``Rasterizer.render_backward(pose_groups=...)``).

    python examples/demo_track_object.py [--gaussians 4000] [--angle-deg 4] [--shift 0.03] [--iters 400]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sim_a_splat_amd.poses import matrix_to_quat_wxyz, quat_wxyz_to_matrix  # noqa: E402
from sim_a_splat_amd.register import se3_exp  # noqa: E402
from sim_a_splat_amd.scene import SplatScene  # noqa: E402
from sim_a_splat_amd.synthetic import ring_camera  # noqa: E402

H, W, FOV = 240, 320, 0.6


def blob(rng, n, centre, spread):
    c = rng.normal(0, spread, (n, 3)) + centre
    A = rng.normal(0, 0.25 * spread, (n, 3, 3))
    return c, A @ A.transpose(0, 2, 1) + (0.05 * spread) ** 2 * np.eye(3), rng.uniform(0, 1, (n, 3)), rng.uniform(0.5, 0.95, n)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=4000, help="per group")
    ap.add_argument("--angle-deg", type=float, default=4.0)
    ap.add_argument("--shift", type=float, default=0.03)
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(7)
    scene = SplatScene(0)
    scene.add_gaussian_splats("static", *blob(rng, a.gaussians, [0.0, 0.35, -0.3], 0.35))
    parts = [blob(rng, a.gaussians, [-0.45, -0.1, 0.1], 0.14), blob(rng, a.gaussians, [0.45, -0.05, 0.15], 0.14)]
    handles = [scene.add_gaussian_splats(f"object{k}", *p) for k, p in enumerate(parts)]
    cams = []
    for yaw, elev in ((0.0, 0.3), (70.0, 0.5)):
        c2w = np.linalg.inv(np.asarray(ring_camera(W, H, 1.0, yaw_deg=yaw, elev=elev).viewmat, np.float64))   # OpenCV axes
        cams.append((matrix_to_quat_wxyz(c2w[:3, :3]), c2w[:3, 3].copy()))
    pictures = scene.get_renders(H, W, cams, fov=FOV)
    centroids = [p[0].mean(axis=0) for p in parts]
    for h, centre in zip(handles, centroids):   # displaced about its own centroid
        w, v = rng.normal(size=3), rng.normal(size=3)
        Tp = np.eye(4)
        Tp[:3, 3] = centre
        M = Tp @ se3_exp(np.concatenate([w * np.deg2rad(a.angle_deg) / np.linalg.norm(w), v * a.shift / np.linalg.norm(v)])) @ np.linalg.inv(Tp)
        h.wxyz, h.position = matrix_to_quat_wxyz(M[:3, :3]), M[:3, 3]

    def errors():
        out = []
        for h, centre in zip(handles, centroids):
            R = quat_wxyz_to_matrix(h.wxyz)
            out.append((np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))), np.linalg.norm(R @ centre + h.position - centre)))
        return out

    before = errors()
    t = time.perf_counter()
    res = scene.refine_handle_poses(handles, pictures, H, W, cams, fov=FOV, iters=a.iters)
    dt = time.perf_counter() - t
    after = errors()
    for h, (a0, d0), (a1, d1) in zip(handles, before, after):
        print(f"{h.name}: {a0:.3f} deg, {d0 * 100:.2f} cm off  ->  {a1:.4f} deg, {d1 * 100:.3f} cm off")
    print(f"loss {res.history[0][1]:.3e} (at 1/{res.history[0][0]} size) -> {res.loss:.3e}   ({a.iters} iterations, two views, {dt:.2f} s)")
    scene.close()
    ok = all(a1 < 0.1 * a0 and d1 < 0.1 * d0 for (a0, d0), (a1, d1) in zip(before, after))
    print("recovered" if ok else "NOT recovered")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
