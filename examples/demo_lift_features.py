#!/usr/bin/env python3
"""Per-Gaussian embeddings from pictures: the synthetic scene with three caps (demo_lift_labels.py's) carries one known embedding per
group; `render_features` of those embeddings plays the feature maps a 2-D extractor would deliver for a ring of views,
`lift_feature_views` pushes them back onto the Gaussians, `features_from_sums` turns the integer sums into mean embeddings, and LERF's
relevancy against the three caps' embeddings (the static scene's as the negative) gives `{"name": bool[N]}` masks.

    python examples/demo_lift_features.py [--n 20000] [--dim 16] [--views 16] [--size 320 240]

Prints, per cap, the share of its seen Gaussians that came back in its mask -- a measurement of this scene.  With real data the
feature images are DINO / CLIP patch features upsampled to the image (or, with 3 channels, new photographs of a captured object) and
the queries are embeddings of a text encoder that is the caller's; `GaussianSplat.lift_features(poses, feature_images)` is the same
call from camera-to-world poses.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from sim_a_splat_amd import semantics  # noqa: E402
from sim_a_splat_amd.rasterizer import LIFT_FEATURE_ONE, Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=(320, 240), metavar=("W", "H"))
    a = ap.parse_args()
    W, H = a.size
    G = 4   # the static scene and three caps
    sc = make_scene(a.n, seed=7, log_scale_mean=float(np.log(0.02)), n_groups=G)
    # the caps of demo_lift_labels.py: cap g is the part of the cloud beyond 0.55 along a horizontal direction of its own
    ang = 2.0 * np.pi * np.arange(1, G) / (G - 1)
    along = sc.means @ np.stack([np.cos(ang), np.zeros_like(ang), np.sin(ang)]).astype(np.float32)
    gid = np.where(along.max(axis=1) > 0.55, 1 + along.argmax(axis=1), 0).astype(np.uint8)
    rng = np.random.default_rng(11)
    group_embed = rng.normal(size=(G, a.dim)).astype(np.float32)
    group_embed /= np.linalg.norm(group_embed, axis=1, keepdims=True)
    embeds = group_embed[gid]                                                       # the known per-Gaussian embeddings
    cams = [ring_camera(W, H, 0.8 * W, yaw_deg=360.0 * k / a.views, elev=0.3 * (k % 3 - 1)) for k in range(a.views)]
    Vs, Ks = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])

    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
    r.upload_features(embeds)
    images = torch.stack([r.render_features(Vs[v], Ks[v], W, H, want=("features",))["features"] for v in range(a.views)])   # [views,H,W,dim]
    scale = 32767.0 / float(images.abs().max())
    out = semantics.lift_feature_views(r, Vs, Ks, W, H, images, scale)
    r.close()
    feats, seen = semantics.features_from_sums(out["sums"], out["weight"], out["feature_scale"])
    rel = semantics.relevancy(feats, group_embed[1:], group_embed[:1])              # [N,3]: the caps against the static scene
    names = [f"cap{g}" for g in range(1, G)]
    masks = semantics.masks_from_relevancy(rel, names, threshold=0.5, seen=seen)
    seen = seen.cpu().numpy()
    cos = (torch.nn.functional.normalize(feats, dim=1).cpu().numpy() * embeds).sum(axis=1)
    print(f"{a.views} views of {W}x{H}, {a.n} Gaussians, {a.dim} channels; {int(seen.sum())} Gaussians seen, "
          f"{float(out['weight'].sum()) / LIFT_FEATURE_ONE:.0f} pixels' worth of weight handed back, largest weight 2^{np.log2(float(out['weight'].max())):.1f}; "
          f"median cosine of a seen Gaussian's lifted embedding to its own {np.median(cos[seen]):.3f}")
    for g, name in enumerate(names, start=1):
        mine = (gid == g) & seen
        back = int((masks[name] & mine).sum())
        print(f"{name}: {back} of {int(mine.sum())} seen Gaussians came back in their own mask ({100.0 * back / max(1, int(mine.sum())):.1f} %), "
              f"{int((masks[name] & ~mine).sum())} of others joined")
    static = (gid == 0) & seen
    taken = np.zeros(a.n, bool)
    for m in masks.values():
        taken |= m
    print(f"static scene: {int((static & ~taken).sum())} of {int(static.sum())} seen Gaussians stayed out of every mask "
          f"({100.0 * (static & ~taken).sum() / max(1, int(static.sum())):.1f} %)")


if __name__ == "__main__":
    main()
