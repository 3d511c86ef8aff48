"""Reconstruct a scene from pictures starting from a tenth of its Gaussians, with and without density control.

The synthetic stand-in scene takes a few pictures of itself.  The fit then starts from a random tenth of its Gaussians and descends the
3DGS photometric loss on all five variable groups -- once at fixed N, once with ``densify=fit.DensifyConfig(...)``: the statistics are
gathered after every backward pass, and on the schedule the resident scene is cloned, split and pruned where it lives, the optimiser
moments following the survivors.  Prints N and the PSNR over all views (``fit.image_metrics``) of both.

    python examples/demo_fit_densify.py [--gaussians 20000] [--size 192] [--views 8] [--iters 600]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sim_a_splat_amd.fit import DensifyConfig, fit_scene, image_metrics  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

WHAT = ("means", "opacities", "colors", "quats", "scales")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=20000)
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
    pictures = torch.stack([r.render(V[v], K[v], a.size, a.size)["rgb"].clone() for v in range(a.views)])
    keep = np.sort(np.random.default_rng(5).choice(a.gaussians, a.gaussians // 10, replace=False))
    psnr = lambda: float(image_metrics(r, V, K, a.size, a.size, pictures)["psnr"].mean())
    rows = {}
    for name, cfg in (("fixed N", None), ("densify", DensifyConfig(start=a.every, every=a.every, reset_every=0, grow_grad2d=a.grow_grad2d,
                                                                     max_gaussians=2 * a.gaussians))):
        r.upload(sc.means[keep], sc.opacities[keep], sc.sh[keep], quats=sc.quats[keep], scales=sc.scales[keep], sh_degree=sc.sh_degree)
        p0 = psnr()
        t = time.perf_counter()
        res = fit_scene(r, V, K, a.size, a.size, pictures, a.iters, what=WHAT, views_per_step=2, loss="dssim", densify=cfg)
        dt = time.perf_counter() - t
        rows[name] = (r.n, psnr())
        print(f"{name:8s}: N {len(keep)} -> {r.n}   PSNR {p0:.2f} -> {rows[name][1]:.2f} dB   loss {res.history[0]:.4e} -> {res.history[-1]:.4e}   "
              f"({res.steps} steps of two views, {dt:.2f} s)")
    r.close()
    ok = rows["densify"][0] > rows["fixed N"][0]
    print("N grew" if ok else "N did NOT grow")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
