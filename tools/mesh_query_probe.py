"""How long the mesh query of a real segmentation takes (Rasterizer.query_meshes; DESIGN.md 3, "Mesh queries"): the 292 247 centres
of the reference's robot scene as normals around the origin, seven posed copies of the xarm6 base mesh (2464 triangles each) under
the shipped ICP similarity, max_distance 0.015 (the segmentation's) and inf (no culling).  HIP events around the call (which is
blocking: validation, the copies and both kernels), a warm-up first, the median of the repeats.  For scale, the float64 NumPy
reference's pairs per second on a subset, on the same machine.

    python tools/mesh_query_probe.py [--points 292247] [--repeats 7] [--out profiles/mesh_query.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import mesh_query_cases as qc  # noqa: E402
import mesh_query_ref as ref  # noqa: E402

from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402


def posed_copies(k=7):
    """k copies of the base mesh: link j turned by 0.9 j rad about z and lifted 0.12 j (robot frame), then the shipped similarity."""
    icp = qc.shipped_similarity()
    out = []
    for j in range(k):
        T = np.eye(4)
        c, s = np.cos(0.9 * j), np.sin(0.9 * j)
        T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        T[2, 3] = 0.12 * j
        out.append(qc.moved(qc.base_mesh(), icp @ T))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=292247)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ref-points", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: no HIP device"
    rng = np.random.default_rng(0)
    pts = rng.normal(0.0, 0.35, (a.points, 3)).astype(np.float32)
    meshes = posed_copies()
    pairs = a.points * sum(len(f) for _, f in meshes)
    lines = [f"# tools/mesh_query_probe.py: {a.points} points x {len(meshes)} meshes x {len(meshes[0][1])} triangles = {pairs:.3e} point-triangle pairs",
             f"# {torch.cuda.get_device_name(0)}; median of {a.repeats} blocking calls after a warm-up, HIP events around the call (host clock beside it)"]
    r = Rasterizer(0)
    dev_pts = torch.from_numpy(pts).to(r.device)
    results = {}
    for md in (0.015, float("inf")):
        res = r.query_meshes(dev_pts, meshes, md)     # warm-up (code objects, scratch)
        culled = float(torch.isinf(res["distance"]).float().mean())
        ms, host = [], []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            res = r.query_meshes(dev_pts, meshes, md)
            e1.record()
            torch.cuda.synchronize()
            host.append(1e3 * (time.perf_counter() - t0))
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        results[md] = (med, res)
        lines.append(f"max_distance {md:<6}: {med:9.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f}; host clock median {np.median(host):.3f} ms), "
                     f"{100 * culled:.2f} % of the (mesh, point) pairs culled, {pairs / (1e-3 * med):.3e} nominal pairs/s, "
                     f"{pairs * (1 - culled) / (1e-3 * med):.3e} evaluated pairs/s")
    speedup = results[float("inf")][0] / results[0.015][0]
    lines.append(f"the 0.015 call is {speedup:.2f} x faster than the inf call")
    d0, d1 = results[0.015][1]["distance"], results[float("inf")][1]["distance"]
    both = torch.isfinite(d0)
    same = bool((d0[both] == d1[both]).all())
    lines.append(f"distance bits where both calls are finite: {'equal' if same else 'DIFFERENT'} ({int(both.sum())} pairs)")
    r.close()
    sub = pts[:a.ref_points]
    t0 = time.perf_counter()
    ref.query_mesh(sub, meshes[0][0], meshes[0][1], np.float64)
    dt = time.perf_counter() - t0
    lines.append(f"float64 NumPy reference (tests/tools/mesh_query_ref.py), {a.ref_points} points x 1 mesh, one CPU thread: "
                 f"{a.ref_points * len(meshes[0][1]) / dt:.3e} pairs/s -> {pairs / (a.ref_points * len(meshes[0][1]) / dt) / 60:.1f} min for the whole query")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0 if same and speedup > 1.5 else 1


if __name__ == "__main__":
    raise SystemExit(main())
