#!/usr/bin/env python3
"""Per-Gaussian masks from pictures instead of meshes: the synthetic scene with link groups is looked at from a ring of cameras, its
own label frames (`render_batch_labels`) play the labelled images, `lift_labels` pushes them back onto the Gaussians, and
`masks_from_votes` turns the votes into the `{"link": bool[N]}` masks a `SplatHandler` is built from.

    python examples/demo_lift_labels.py [--n 20000] [--groups 4] [--views 16] [--size 320 240]

Prints, per group, the share of its Gaussians with `seen > 0` that came back under their own label, then builds a handler from the
lifted masks and renders one frame.  With real data the label images are hand-painted masks or a 2D segmenter's output, 255 where
nothing is labelled; `GaussianSplat.lift_labels(poses, label_images, n_labels)` is the same call from camera-to-world poses.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from sim_a_splat_amd import segment  # noqa: E402
from sim_a_splat_amd.covariance import compute_cov, sh2rgb  # noqa: E402
from sim_a_splat_amd.handler import SplatHandler  # noqa: E402
from sim_a_splat_amd.rasterizer import LIFT_ONE, Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=(320, 240), metavar=("W", "H"))
    a = ap.parse_args()
    W, H = a.size
    G = a.groups
    sc = make_scene(a.n, seed=7, log_scale_mean=float(np.log(0.02)), n_groups=G)
    # make_scene draws its link members all over the scene; objects are compact: link g is the cap of the cloud beyond 0.55 along a
    # horizontal direction of its own, the rest is the static scene (group 0)
    ang = 2.0 * np.pi * np.arange(1, G) / max(1, G - 1)
    along = sc.means @ np.stack([np.cos(ang), np.zeros_like(ang), np.sin(ang)]).astype(np.float32)      # [N,G-1]
    gid = np.where(along.max(axis=1) > 0.55, 1 + along.argmax(axis=1), 0).astype(np.uint8) if G > 1 else np.zeros(a.n, np.uint8)
    sc.group_id = gid
    cams = [ring_camera(W, H, 0.8 * W, yaw_deg=360.0 * k / a.views, elev=0.3 * (k % 3 - 1)) for k in range(a.views)]
    Vs, Ks = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])

    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    labels = r.render_batch_labels(Vs, Ks, W, H, min_alpha=0.5)["labels"]          # [views,H,W] uint8, 255: nothing shows
    sums = segment.lift_label_views(r, Vs, Ks, W, H, labels, G)
    votes, seen = sums["votes"].cpu().numpy(), sums["seen"].cpu().numpy()
    r.close()
    names = [f"link{g}" for g in range(G)]
    masks = segment.masks_from_votes(votes, seen, names, min_share=0.5)
    print(f"{a.views} views of {W}x{H}, {a.n} Gaussians in {G} groups; {int((seen > 0).sum())} Gaussians seen, "
          f"{seen.sum() / LIFT_ONE:.0f} pixels' worth of weight handed back")
    right = total = 0
    for g, name in enumerate(names):
        mine = (sc.group_id == g) & (seen > 0)
        back = int((masks[name] & mine).sum())
        right, total = right + back, total + int(mine.sum())
        print(f"{name}: {back} of {int(mine.sum())} seen Gaussians came back under their own label "
              f"({100.0 * back / max(1, int(mine.sum())):.1f} %), {int((masks[name] & ~mine).sum())} of others joined")
    print(f"agreement over all groups: {100.0 * right / max(1, total):.1f} %")

    # the lifted masks are link masks: a handler takes them as it takes the ones made from URDF meshes (link0 is the static scene here)
    link_masks = {f"link{g - 1}": masks[f"link{g}"] for g in range(1, G)}
    covs = compute_cov(torch.from_numpy(sc.quats), torch.from_numpy(sc.scales)).numpy()
    rgb = np.clip(sh2rgb(torch.from_numpy(sc.sh[:, 0])).numpy(), 0, 1)
    h = SplatHandler.from_arrays(sc.means, covs, rgb, sc.opacities, link_masks, np.eye(4), [np.eye(4)] * len(link_masks), device=0)
    cam = (np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 3.0]))              # camera-to-world, OpenCV axes: from +z towards the origin
    frame, = h.render(h.scene, [cam], [[H, W]])
    print(f"handler from the lifted masks: {len(link_masks)} links, one frame {frame.shape} rendered, mean {frame.mean():.1f}")
    h.scene.close()


if __name__ == "__main__":
    main()
