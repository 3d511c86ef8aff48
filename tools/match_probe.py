"""How long the point matching of a real registration takes (Rasterizer.match_points; DESIGN.md 3, "Point matching"): 20 000 points
sampled from seven posed copies of the xarm6 base mesh against 113 831 and 292 247 target points (the sizes of the reference's two
scenes), the robot's own surface under a similarity plus background; correspondence distance 0.2, the library's slice choice.  HIP
events around the call (which is blocking: validation, the copies and the three kernels), a warm-up first, the median of the repeats
with their spread; then one whole 30-iteration registration on the host clock.  For scale, scipy's cKDTree (16 workers) on the same
clouds: building the tree once and one query of the 20 000 points.

    python tools/match_probe.py [--source 20000] [--repeats 9] [--out profiles/match_points.txt]
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
import match_cases as mc  # noqa: E402
import mesh_query_cases as qc  # noqa: E402

from sim_a_splat_amd import mesh_io, register  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402


def robot_surface():
    """Seven copies of the base mesh as one surface: link j turned by 0.9 j rad about z and lifted 0.12 j."""
    v, f = qc.base_mesh()
    vs, fs = [], []
    for j in range(7):
        T = np.eye(4)
        c, s = np.cos(0.9 * j), np.sin(0.9 * j)
        T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        T[2, 3] = 0.12 * j
        vs.append(mc.apply(T, v))
        fs.append(f + j * len(v))
    return np.concatenate(vs), np.concatenate(fs)


def clouds(n_source, n_target, rng):
    """(source, target, truth, guess): a third of the target lies on the robot under the shipped similarity (normal(0, 0.004) off
    it), the rest is a scene around it."""
    v, f = robot_surface()
    truth = qc.shipped_similarity()
    source = mesh_io.sample_surface(v, f, n_source, seed=0).astype(np.float32)
    on = mc.apply(truth, mesh_io.sample_surface(v, f, n_target // 3, seed=1)) + rng.normal(0, 0.004, (n_target // 3, 3))
    lo, hi = on.min(0) - 1.5, on.max(0) + 1.5
    target = np.concatenate([on, rng.uniform(lo, hi, (n_target - len(on), 3))]).astype(np.float32)
    guess = mc.perturbed(truth, 3.0, 0.01, 1.02, about=on.mean(0))
    return source, target, truth, guess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", type=int, default=20000)
    ap.add_argument("--targets", type=int, nargs="+", default=[113831, 292247])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: no HIP device"
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    lines = [f"# tools/match_probe.py: {a.source} source points; {torch.cuda.get_device_name(0)}",
             f"# per size: median of {a.repeats} blocking calls after a warm-up, HIP events around the call (host clock beside it); one registration; cKDTree"]
    r = Rasterizer(0)
    ok = True
    for n_target in a.targets:
        source, target, truth, guess = clouds(a.source, n_target, rng)
        pairs = a.source * n_target
        ds, dt = torch.from_numpy(source).to(r.device), torch.from_numpy(target).to(r.device)
        res = r.match_points(ds, dt, guess, 0.2)      # warm-up (code objects, scratch)
        ms, host = [], []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            again = r.match_points(ds, dt, guess, 0.2)
            e1.record()
            torch.cuda.synchronize()
            host.append(1e3 * (time.perf_counter() - t0))
            ms.append(e0.elapsed_time(e1))
        same = bool((again["index"] == res["index"]).all()) and bool((again["dist2"] == res["dist2"]).all()) and \
            again["moments"].tobytes() == res["moments"].tobytes()
        ok = ok and same
        med = float(np.median(ms))
        lines.append(f"{a.source} x {n_target} = {pairs:.3e} pairs: {med:8.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f}; host clock median "
                     f"{np.median(host):.3f} ms), {pairs / (1e-3 * med):.3e} pairs/s, {int(res['moments'][0])} held; repeated calls "
                     f"{'the same bits' if same else 'DIFFERENT'}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reg = register.register_similarity(ds, dt, guess, max_correspondence_distance=0.2, max_iteration=30, relative_fitness=0.0,
                                           relative_rmse=0.0, rasterizer=r)     # (limits of 0: all 30 iterations run)
        wall = 1e3 * (time.perf_counter() - t0)
        lines.append(f"    registration, {reg.iterations} iterations ({reg.iterations + 1} match_points calls + the fits on the host): {wall:.1f} ms; "
                     f"fitness {reg.fitness:.4f}, rmse {reg.inlier_rmse:.5f}, |T - truth| max {np.abs(reg.transformation - truth).max():.2e}")
        t0 = time.perf_counter()
        tree = cKDTree(target)
        t1 = time.perf_counter()
        moved = mc.apply(guess, source)
        dist, idx = tree.query(moved, k=1, distance_upper_bound=0.2, workers=16)
        t2 = time.perf_counter()
        gi = res["index"].cpu().numpy()
        held = gi >= 0
        agree = float((idx[held] == gi[held]).mean()) if held.any() else 1.0
        lines.append(f"    scipy cKDTree, 16 workers, float64: build {1e3 * (t1 - t0):.1f} ms + query {1e3 * (t2 - t1):.1f} ms; "
                     f"{100 * agree:.3f} % of the held matches name the same target")
    r.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
