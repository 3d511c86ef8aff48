"""What a feature frame costs: HIP-event times of a plain SAS_FULL_SORT frame and of sas_render_features frames with
C = 3, 8, 16, 64 channels, at config 3 (1 M Gaussians, 1920x1080) and on one 320x240 Gym camera (config 2's scene).

    python tools/feature_probe.py [--reps 30] [--out profiles/features_probe.json]

The feature pass is the difference of the two medians (the frames are otherwise the same launches).  Kernel times
alone come from a separate run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/feature_probe.py --reps 10
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import config_scene_and_cameras, ring_camera  # noqa: E402


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = Rasterizer(0)
    rows = []
    for label, cfg, cam in (("config3_1080p", 3, None), ("gym_320x240", 2, ring_camera(320, 240, 260.0, yaw_deg=20.0))):
        sc, cams = config_scene_and_cameras(cfg)
        cam = cam or cams[0]
        r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree,
                 group_id=sc.group_id, n_groups=int(sc.group_id.max()) + 1 if sc.group_id is not None else 0)
        W, H = cam.width, cam.height
        out = {k: torch.empty((H, W, c), device="cuda") for k, c in (("rgb", 3), ("alpha", 1), ("depth", 1))}
        plain = lambda: r.render(cam.viewmat, cam.K, W, H, want=("rgb", "alpha", "depth"), full_sort=True, out=out)
        lazy = lambda: r.render(cam.viewmat, cam.K, W, H, want=("rgb", "alpha", "depth"), out=out)
        for fn in (plain, lazy):
            timed(fn, 3)
        base = timed(plain, a.reps)
        row = dict(view=label, n=int(sc.means.shape[0]), W=W, H=H, lazy_ms=timed(lazy, a.reps)[0], full_sort_ms=base[0],
                   stats=r.stats(), features={})
        rng = np.random.default_rng(0)
        for C in (3, 8, 16, 64):
            r.upload_features(rng.uniform(0, 1, size=(sc.means.shape[0], C)).astype(np.float32))
            fo = dict(out, features=torch.empty((H, W, C), device="cuda"))
            feat = lambda: r.render_features(cam.viewmat, cam.K, W, H, want=("features", "rgb", "alpha", "depth"), out=fo)
            timed(feat, 3)
            med, lo = timed(feat, a.reps)
            row["features"][C] = dict(frame_ms=med, frame_min_ms=lo, pass_ms=med - base[0])
        rows.append(row)
        print(json.dumps(row))
    r.close()
    if a.out:
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
