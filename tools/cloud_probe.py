"""What a fixed-size point cloud costs a Door-B step (Rasterizer.sample_point_cloud; DESIGN.md 3, "Point clouds"): the stand-in scene
(292 247 Gaussians, the static rest + 7 link groups) with the procedural robot's meshes, 2 cameras of 240x320, a workspace crop, a 5 mm
voxel grid, K = 512 / 1024 / 4096 points -- for one env, and for 16 envs (32 views, 16 clouds) in one call.

Per configuration: the label-frame call the cloud follows (render_batch_labels with rgb8 and depth), then the sample call -- HIP events
around the blocking call and the host clock beside it, a warm-up first, the median of the repeats with their spread -- M before and
after the grid, and the split between the call's kernels (a timed call of its own: mark / compact / sample).  As the baseline, the same
cloud by plain torch on the same GPU, written here: unprojection and crop with torch.where, the grid's lowest pixel per cell with
unique + scatter_reduce, and a K-iteration minimum / argmax loop (all clouds of the call in one padded batch, nothing synchronised
inside the loop).  It must return the same ``index``: the probe doubles as a check and exits 1 when it does not.

    python tools/cloud_probe.py [--repeats 9] [--out profiles/point_cloud.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(Path(__file__).resolve().parent)]
from robot_mesh_probe import robot  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer, cloud_transforms  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, random_group_poses, ring_camera  # noqa: E402

W, H, G = 320, 240, 8
# the workspace: the part of the stand-in's front the cameras see (they stand 3 m out; the dense scene shows its outer shell), sized so that
# the 5 mm grid stays within the contract's 2^24 cells (240 x 240 x 180)
BOUNDS = ((-0.6, -0.6, 0.2), (0.6, 0.6, 1.1))
VOXEL = 0.005


def torch_cloud(depth, Ks, T, K, clouds, E, bounds, voxel):
    """The contract in plain torch ops on the device (each one rounded float32 operation, as the kernels'): index [E,K] int32."""
    dev = depth.device
    C = depth.shape[0]
    d = depth.reshape(C, H, W)
    v, u = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    Kt, Tt = torch.from_numpy(Ks.reshape(C, 9)).to(dev), torch.from_numpy(T.reshape(C, 12)).to(dev)
    k = lambda i: Kt[:, i].reshape(C, 1, 1)
    a = lambda i: Tt[:, i].reshape(C, 1, 1)
    x = (u.float() - k(2)) * d / k(0)
    y = (v.float() - k(5)) * d / k(4)
    w = torch.stack([((a(4 * j) * x + a(4 * j + 1) * y) + a(4 * j + 2) * d) + a(4 * j + 3) for j in range(3)], dim=-1)
    lo, hi = (torch.tensor(b, dtype=torch.float32, device=dev) for b in bounds)
    ok = (d > 0) & (d < float("inf")) & torch.isfinite(w).all(-1) & ((lo <= w) & (w <= hi)).all(-1)
    n = torch.clamp(torch.ceil((hi - lo) / voxel), min=1).long()
    rows, ps = [], []
    for e in range(E):
        views = torch.tensor([c for c in range(C) if clouds[c] == e], device=dev)
        p = torch.where(ok[views].reshape(-1))[0]
        p = views[p // (H * W)] * (H * W) + p % (H * W)                      # flat pixel of the call, ascending
        we = w.reshape(-1, 3)[p]
        if voxel > 0:
            i = torch.minimum(torch.floor((we - lo) / voxel), (n - 1).float()).long()
            cell = (i[:, 0] * n[1] + i[:, 1]) * n[2] + i[:, 2]
            uniq, inv = torch.unique(cell, return_inverse=True)
            first = torch.full((len(uniq),), 2 ** 62, dtype=torch.long, device=dev).scatter_reduce(0, inv, p, "amin")
            keep = first[inv] == p
            p, we = p[keep], we[keep]
        rows.append(we)
        ps.append(p)
    M = [len(p) for p in ps]
    Mmax = max(max(M), 1)
    pts = torch.zeros((E, Mmax, 3), device=dev)
    dist = torch.full((E, Mmax), -1.0, device=dev)                           # -1: picked, or padding
    for e in range(E):
        pts[e, :M[e]] = rows[e]
        dist[e, :M[e]] = float("inf")
    picks = torch.zeros((E, K), dtype=torch.long, device=dev)
    s = torch.zeros((E,), dtype=torch.long, device=dev)
    ar = torch.arange(E, device=dev)
    for j in range(K):
        picks[:, j] = s
        dlt = pts - pts[ar, s][:, None, :]
        d2 = (dlt[..., 0] * dlt[..., 0] + dlt[..., 1] * dlt[..., 1]) + dlt[..., 2] * dlt[..., 2]
        dist = torch.where(dist < 0, dist, torch.minimum(dist, d2))
        dist[ar, s] = -1.0
        s = torch.argmax(dist, dim=1)
    index = torch.full((E, K), -1, dtype=torch.int32, device=dev)
    for e in range(E):
        k_ = min(K, M[e])
        index[e, :k_] = ps[e][picks[e, :k_]].int()
    return index, M


def timed(fn, repeats):
    fn()
    ms, host = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        host.append(1e3 * (time.perf_counter() - t0))
        ms.append(e0.elapsed_time(e1))
    return out, float(np.median(ms)), min(ms), max(ms), float(np.median(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--n", type=int, default=292_247)
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--points", type=int, nargs="+", default=[512, 1024, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: no HIP device"
    sc = make_scene(a.n, seed=2, n_groups=G)
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=3, group_id=sc.group_id, n_groups=G)
    m = robot()
    r.upload_meshes(m["verts"], m["tris"], (0.7, 0.7, 0.75), groups=m["groups"])
    cams = [ring_camera(W, H, 262.0, yaw_deg=0.0), ring_camera(W, H, 262.0, yaw_deg=60.0, elev=0.5)]
    lines = [f"# tools/cloud_probe.py: {a.n} Gaussians + {len(m['tris'])} triangles, 2 cameras of {W}x{H} per env, crop {BOUNDS}, voxel {VOXEL}; "
             f"{torch.cuda.get_device_name(0)}",
             f"# medians of {a.repeats} blocking calls after a warm-up (torch baseline: {a.torch_repeats}), HIP events around the call, host clock beside it"]
    ok = True
    for E in a.envs:
        V = np.stack([np.asarray(c.viewmat, np.float32) for c in cams] * E)
        Ks = np.stack([np.asarray(c.K, np.float32) for c in cams] * E)
        sets = np.stack([random_group_poses(G, seed=100 + e) for e in range(E)])
        pose_set = np.repeat(np.arange(E), 2).astype(np.int32)
        clouds = pose_set.copy()
        frames = lambda: r.render_batch_labels(V, Ks, W, H, want=("rgb8", "depth"), pose_sets=sets, pose_set=pose_set)
        o, f_ms, f_min, f_max, f_host = timed(frames, a.repeats)
        T = cloud_transforms(V)
        sample = lambda K, voxel=VOXEL, timing=False: r.sample_point_cloud(o["depth"], V, Ks, W, H, K, rgb8=o["rgb8"], labels=o["labels"], bounds=BOUNDS,
                                                                        voxel_size=voxel, clouds=clouds, n_clouds=E, timing=timing)
        before = sample(1, voxel=0.0)["count"].cpu().numpy()
        lines.append(f"E = {E} ({2 * E} views): label frames with rgb8 and depth {f_ms:.3f} ms per call (min {f_min:.3f}, max {f_max:.3f}; host clock {f_host:.3f})")
        for K in a.points:
            res, ms, lo, hi, host = timed(lambda: sample(K), a.repeats)
            again = sample(K, timing=True)
            st = r.stage_times()
            same = all(torch.equal(res[k], again[k]) for k in res)
            after = res["count"].cpu().numpy()
            (tidx, tM), t_ms, t_lo, t_hi, t_host = timed(lambda: torch_cloud(o["depth"], Ks, T, K, clouds, E, BOUNDS, VOXEL), a.torch_repeats)
            equal = bool(torch.equal(tidx, res["index"])) and list(after) == tM
            ok = ok and same and equal
            lines.append(f"  K = {K}: sample call {ms:.3f} ms (min {lo:.3f}, max {hi:.3f}; host clock {host:.3f}); M per cloud before the grid "
                         f"{int(before.min())}..{int(before.max())}, after {int(after.min())}..{int(after.max())}; kernels: mark {st['project']:.3f} + compact "
                         f"{st['scatter']:.3f} + sample {st['blend']:.3f} = {st['total']:.3f} ms; repeated calls {'the same bytes' if same else 'DIFFERENT'}")
            lines.append(f"      torch on the GPU: {t_ms:.3f} ms (min {t_lo:.3f}, max {t_hi:.3f}; host clock {t_host:.3f}); index "
                         f"{'equal' if equal else 'DIFFERENT'}; torch / HIP = {t_ms / ms:.1f}" + ("" if ms < t_ms else "   (the HIP call is NOT faster here)"))
    r.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
