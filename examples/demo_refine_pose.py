"""Recover a camera pose by render-and-compare through the HIP backward pass.

A camera of the synthetic scene takes a picture; the same camera is then moved by a few centimetres and degrees, and
``register.refine_camera_pose`` brings it back by descending the gradient of the photometric loss with respect to the view matrix
(``Rasterizer.render_backward`` through ``autograd.render_differentiable``).

    python examples/demo_refine_pose.py [--gaussians 20000] [--size 128] [--angle-deg 3] [--shift 0.03] [--iters 300]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.register import refine_camera_pose, se3_exp  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402


def pose_error(A, B):
    D = A @ np.linalg.inv(B)
    centre = lambda M: -M[:3, :3].T @ M[:3, 3]
    return np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1))), np.linalg.norm(centre(A) - centre(B))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--angle-deg", type=float, default=3.0)
    ap.add_argument("--shift", type=float, default=0.03)
    ap.add_argument("--iters", type=int, default=300)
    a = ap.parse_args(argv)
    sc = make_scene(a.gaussians, seed=4, log_scale_mean=float(np.log(0.03)))
    cam = ring_camera(a.size, a.size, 1.1 * a.size, yaw_deg=20.0, elev=0.3)
    V = np.asarray(cam.viewmat, np.float64)
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
    picture = r.render(cam.viewmat, cam.K, a.size, a.size)["rgb"].clone()
    rng = np.random.default_rng(0)
    w, v = rng.normal(size=3), rng.normal(size=3)
    xi = np.concatenate([w * np.deg2rad(a.angle_deg) / np.linalg.norm(w), v * a.shift / np.linalg.norm(v)])
    V0 = se3_exp(xi) @ V
    t = time.perf_counter()
    res = refine_camera_pose(r, picture, V0, cam.K, a.size, a.size, iters=a.iters)
    dt = time.perf_counter() - t
    a0, d0 = pose_error(V0, V)
    a1, d1 = pose_error(res.viewmat, V)
    print(f"start : {a0:.3f} deg, {d0 * 100:.2f} cm off   loss {res.history[0][1]:.3e} (at 1/{res.history[0][0]} size)")
    print(f"end   : {a1:.4f} deg, {d1 * 100:.3f} cm off   loss {res.loss:.3e}   ({a.iters} iterations, {dt:.2f} s)")
    r.close()
    ok = a1 < 0.1 * a0 and d1 < 0.1 * d0
    print("recovered" if ok else "NOT recovered")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
