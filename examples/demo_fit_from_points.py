"""Reconstruct a scene from pictures and a point cloud: the first scene comes from ``fit.init_scene``.

The synthetic stand-in scene of examples/demo_fit_densify.py takes a few pictures of itself, with depth.  ``sample_point_cloud`` turns the
depth frames into a coloured cloud (farthest-point sampling over all views), as an RGB-D rig or a structure-from-motion run would hand over.
``init_scene`` makes the first Gaussians of it -- the points as means, their colours as the SH DC term, opacity 0.1, and as isotropic scale
the RMS distance to the three nearest neighbours, found on the GPU by ``Rasterizer.knn_points`` -- and ``fit_scene`` with density control
takes it from there.  Beside it, the same fit started from as many uniformly random grey points in the scene's bounds with the same scale
rule.  Prints N and the PSNR over all views (``fit.image_metrics``) of both.

    python examples/demo_fit_from_points.py [--gaussians 20000] [--points 2000] [--size 192] [--views 8] [--iters 600]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sim_a_splat_amd.fit import DensifyConfig, fit_scene, image_metrics, init_scene  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

WHAT = ("means", "opacities", "colors", "quats", "scales")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--every", type=int, default=100, help="densify after every this many steps (from the first such step on)")
    ap.add_argument("--grow-grad2d", type=float, default=2e-4)
    a = ap.parse_args(argv)
    sc = make_scene(a.gaussians, seed=4, log_scale_mean=float(np.log(0.03)))
    cams = [ring_camera(a.size, a.size, 1.1 * a.size, yaw_deg=360.0 * k / a.views, elev=0.3) for k in range(a.views)]
    V, K = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
    frames = [{k: v.clone() for k, v in r.render(V[v], K[v], a.size, a.size, want=("rgb", "alpha", "depth", "rgb8")).items()} for v in range(a.views)]
    pictures = torch.stack([f["rgb"] for f in frames])
    # a pixel the scene covers well has a depth; the others are no points
    depth = torch.stack([torch.where(f["alpha"][..., 0] > 0.5, f["depth"][..., 0], torch.zeros_like(f["depth"][..., 0])) for f in frames])
    cloud = r.sample_point_cloud(depth, V, K, a.size, a.size, a.points, rgb8=torch.stack([f["rgb8"] for f in frames]))
    k = min(a.points, int(cloud["count"][0]))
    pts, cols = cloud["points"][0, :k].contiguous(), cloud["colors"][0, :k].contiguous()
    lo, hi = torch.tensor(sc.means.min(axis=0), device=r.device), torch.tensor(sc.means.max(axis=0), device=r.device)
    rnd = lo + (hi - lo) * torch.rand((k, 3), generator=torch.Generator(device=r.device).manual_seed(5), device=r.device)
    t = time.perf_counter()
    d2 = r.knn_points(pts, 3)["dist2"]
    torch.cuda.synchronize()
    print(f"cloud: {int(cloud['count'][0])} pixels with a depth in {a.views} views, {k} sampled; knn_points of them {1e3 * (time.perf_counter() - t):.2f} ms "
          f"(first call), median neighbour distance {float(d2.mean(dim=1).sqrt().median()):.4f}; grid {r.knn_stats()}")
    psnr = lambda: float(image_metrics(r, V, K, a.size, a.size, pictures)["psnr"].mean())
    rows = {}
    for name, (p, c) in (("from the cloud", (pts, cols)), ("random points", (rnd, None))):
        init_scene(r, p, c, sh_degree=sc.sh_degree)
        p0 = psnr()
        cfg = DensifyConfig(start=a.every, every=a.every, reset_every=0, grow_grad2d=a.grow_grad2d, max_gaussians=2 * a.gaussians)
        t = time.perf_counter()
        res = fit_scene(r, V, K, a.size, a.size, pictures, a.iters, what=WHAT, views_per_step=2, loss="dssim", densify=cfg)
        dt = time.perf_counter() - t
        rows[name] = (r.n, psnr())
        print(f"{name:14s}: N {k} -> {r.n}   PSNR {p0:.2f} -> {rows[name][1]:.2f} dB   loss {res.history[0]:.4e} -> {res.history[-1]:.4e}   "
              f"({res.steps} steps of two views, {dt:.2f} s)")
    r.close()
    ok = rows["from the cloud"][1] > rows["random points"][1]
    print("the cloud start ends above the random start" if ok else "the cloud start did NOT end above the random start")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
