"""Adapt a scene's appearance to pictures with the fused optimiser step on the resident scene.

The synthetic stand-in scene takes a few pictures of itself; its colours are then tinted and its opacities scaled (another day's
lighting), and ``fit.fit_scene`` recovers them from the pictures: render, loss, ``Rasterizer.render_backward``, ``Rasterizer.adam_step``
-- the scene is never uploaded again.  Prints the loss and the PSNR over all views before and after.

    python examples/demo_fit_appearance.py [--gaussians 20000] [--size 128] [--views 6] [--iters 200]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sim_a_splat_amd.fit import fit_scene, mean_loss  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402


def psnr(r, V, K, size, pictures):
    mse = [float(((r.render(V[v], K[v], size, size)["rgb"] - pictures[v]) ** 2).mean()) for v in range(len(V))]
    return -10.0 * np.log10(max(float(np.mean(mse)), 1e-12))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--loss", choices=("l1", "dssim"), default="l1", help="dssim: descend 0.8 L1 + 0.2 (1 - SSIM) through Rasterizer.photometric_loss")
    a = ap.parse_args(argv)
    sc = make_scene(a.gaussians, seed=4, log_scale_mean=float(np.log(0.03)))
    cams = [ring_camera(a.size, a.size, 1.1 * a.size, yaw_deg=360.0 * k / a.views, elev=0.3) for k in range(a.views)]
    V, K = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
    pictures = torch.stack([r.render(V[v], K[v], a.size, a.size)["rgb"].clone() for v in range(a.views)])
    tinted = sc.sh * np.float32(0.7)
    tinted[:, 0] += np.array([0.4, -0.3, 0.2], np.float32)
    r.upload(sc.means, sc.opacities * np.float32(0.7), tinted, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
    l0, p0 = mean_loss(r, V, K, a.size, a.size, pictures), psnr(r, V, K, a.size, pictures)
    t = time.perf_counter()
    res = fit_scene(r, V, K, a.size, a.size, pictures, a.iters, what=("colors", "opacities"), lrs=dict(sh_dc=2e-2, sh_rest=1e-3), views_per_step=2,
                    loss=None if a.loss == "l1" else a.loss)
    dt = time.perf_counter() - t
    l1, p1 = mean_loss(r, V, K, a.size, a.size, pictures), psnr(r, V, K, a.size, pictures)
    print(f"start : loss {l0:.4e}  PSNR {p0:.2f} dB")
    print(f"end   : loss {l1:.4e}  PSNR {p1:.2f} dB   ({res.steps} steps of two views, {dt:.2f} s, {1e3 * dt / max(res.steps, 1):.2f} ms per step)")
    r.close()
    ok = l1 < 0.5 * l0
    print("recovered" if ok else "NOT recovered")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
