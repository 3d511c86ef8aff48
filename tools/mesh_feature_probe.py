"""What a feature frame WITH meshes costs: the 1920x1080 mesh case of tests/tools/mesh_cases.py (about 20 k Gaussians, 3 584
triangles) with C feature channels, beside the same scene without its meshes.

    python tools/mesh_feature_probe.py [--channels 8] [--reps 10]

Prints the median HIP-event time of each frame; kernel times come from a run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/mesh_feature_probe.py
(k_blend_features is the kernel of the frames without meshes, k_blend_features_mesh of those with; plain mesh frames run
k_blend_mesh, those with features or mesh_surface k_blend_mesh_scene).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests" / "tools")]
import mesh_cases as mc  # noqa: E402
from feature_probe import timed  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    case = mc.case_1080p()
    V, K, W, H = case["cams"][0]
    rng = np.random.default_rng(0)
    f = rng.uniform(0, 1, size=(case["sc"]["means"].shape[0], a.channels)).astype(np.float32)
    fm = rng.uniform(0, 1, size=(len(case["mesh"]["tris"]), a.channels)).astype(np.float32)
    r = Rasterizer(0)
    row = dict(W=W, H=H, n=int(f.shape[0]), triangles=int(fm.shape[0]), channels=a.channels)
    want = ("features", "rgb", "alpha", "depth")
    for label, meshes in (("without_meshes", False), ("with_meshes", True)):
        mc.upload(r, case["sc"])
        if meshes:
            m = case["mesh"]
            r.upload_meshes(m["verts"], m["tris"], m["cols"], groups=m["groups"], ambient=m["ka"], diffuse=m["kd"])
        r.upload_features(f)
        if meshes:
            r.upload_mesh_features(fm)
        plain = lambda: r.render(V, K, W, H, want=want[1:], full_sort=True)
        feat = lambda: r.render_features(V, K, W, H, want=want)
        for fn in (plain, feat):
            timed(fn, 3)
        row[label] = dict(frame_ms=timed(plain, a.reps)[0], feature_frame_ms=timed(feat, a.reps)[0])
        if meshes:
            surface = lambda: r.render(V, K, W, H, want=want[1:], mesh_surface=True)
            timed(surface, 3)
            row[label]["surface_frame_ms"] = timed(surface, a.reps)[0]
    r.close()
    print(json.dumps(row))


if __name__ == "__main__":
    main()
