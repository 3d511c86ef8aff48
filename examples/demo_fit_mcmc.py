"""Reconstruct a scene from pictures under a BUDGET of Gaussians: fixed N, the default density strategy capped, and MCMC density control.

The synthetic stand-in scene takes a few pictures of itself.  Three fits start from the same random tenth of its Gaussians and descend the
3DGS photometric loss on all five variable groups, each allowed at most ``--cap`` Gaussians: at fixed N; with
``densify=fit.DensifyConfig(max_gaussians=cap)``, which stops growing at the cap and never moves capacity; and with
``densify=fit.McmcConfig(cap_max=cap)``, which re-births dead Gaussians on live ones, grows by ``--grow-factor`` a time up to the cap and
perturbs the means with noise after every step.  Prints N, the PSNR over all views (``fit.image_metrics``) and the final loss of each arm:
a measurement of this scene at these settings, not a guarantee for another.

    python examples/demo_fit_mcmc.py [--gaussians 20000] [--cap 6000] [--size 192] [--views 8] [--iters 600]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sim_a_splat_amd.fit import DensifyConfig, McmcConfig, fit_scene, image_metrics  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

WHAT = ("means", "opacities", "colors", "quats", "scales")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--cap", type=int, default=6000, help="the budget of every arm")
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--every", type=int, default=50, help="densify / refine after every this many steps")
    ap.add_argument("--grow-factor", type=float, default=1.25, help="MCMC: growth per refine (gsplat's default is 1.05, over 25 000 steps)")
    a = ap.parse_args(argv)
    sc = make_scene(a.gaussians, seed=4, log_scale_mean=float(np.log(0.03)))
    cams = [ring_camera(a.size, a.size, 1.1 * a.size, yaw_deg=360.0 * k / a.views, elev=0.3) for k in range(a.views)]
    V, K = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
    pictures = torch.stack([r.render(V[v], K[v], a.size, a.size)["rgb"].clone() for v in range(a.views)])
    keep = np.sort(np.random.default_rng(5).choice(a.gaussians, a.gaussians // 10, replace=False))
    psnr = lambda: float(image_metrics(r, V, K, a.size, a.size, pictures)["psnr"].mean())
    arms = (("fixed N", None),
            ("default", DensifyConfig(start=a.every, every=a.every, reset_every=0, max_gaussians=a.cap)),
            ("MCMC", McmcConfig(cap_max=a.cap, start=a.every, every=a.every, grow_factor=a.grow_factor)))
    rows = {}
    for name, cfg in arms:
        r.upload(sc.means[keep], sc.opacities[keep], sc.sh[keep], quats=sc.quats[keep], scales=sc.scales[keep], sh_degree=sc.sh_degree)
        p0 = psnr()
        t = time.perf_counter()
        res = fit_scene(r, V, K, a.size, a.size, pictures, a.iters, what=WHAT, views_per_step=2, loss="dssim", densify=cfg)
        dt = time.perf_counter() - t
        rows[name] = (r.n, psnr(), max(res.n_history, default=r.n))
        print(f"{name:8s}: N {len(keep)} -> {r.n} (most {rows[name][2]}, budget {a.cap})   PSNR {p0:.2f} -> {rows[name][1]:.2f} dB   "
              f"loss {res.history[0]:.4e} -> {res.history[-1]:.4e}   ({res.steps} steps of two views, {dt:.2f} s)")
    r.close()
    ok = all(most <= max(a.cap, len(keep)) for _, _, most in rows.values())
    print("measured on this scene at these settings; every arm stayed within its budget" if ok else "an arm EXCEEDED its budget")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
