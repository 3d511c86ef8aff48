"""What TSDF fusion costs (Rasterizer.fuse_depth; DESIGN.md 3, "Depth fusion"): the Door-B stand-in scene (292 247 Gaussians, the static
rest + 7 link groups) with the procedural robot's meshes, seen by 2 and by 32 ring cameras of 240x320, fused into a 128^3 and a 256^3
volume around the scene (2.56 m a side, the stand-in's 2 m cube inside it: 20 mm and 10 mm voxels), with colour, labels and a keep table
that keeps every row: the filled background carves.

Per configuration: the label-frame call that feeds the fusion (render_batch_labels with rgb8 and depth, the background's depth filled),
then the blocking fuse call into a fresh volume -- HIP events around the call and the host clock beside it, behind a clock ramp of warm-up
calls, the median of the repeats with their spread -- the kernel alone (a SAS_TIMING call of its own), the voxels touched, and the traffic
floor beside the numbers: 20 B read per voxel (tsdf, weight, colour), 20 B written per touched voxel, the depth, label and colour images
once (8 B per pixel).  As the baseline, the same contract by plain torch on the same GPU, written here: one pass of whole-volume
tensor operations per view.  It must return the same bytes: the probe doubles as a check and exits 1 when it does not.

    python tools/fuse_probe.py [--repeats 9] [--out profiles/tsdf_fuse.txt]
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
from sim_a_splat_amd.rasterizer import Rasterizer, cloud_keep_table, fuse_transforms  # noqa: E402
from sim_a_splat_amd.reconstruct import TsdfVolume  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

W, H, G = 320, 240, 8
SIDE = 2.56
KEEP = list(range(0, 9))   # every row is surface; the filled background (label 255) carves


def torch_fuse(vol, depth, rgb8, labels, Ks, T, keep, trunc, near=0.01, pc=0.5, max_weight=64.0):
    """The contract in plain torch ops on the device (each one rounded float32 operation, as the kernel's), view by view, in place."""
    dev = depth.device
    nx, ny, nz = vol.dims
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    ax = lambda n, lo: f32(float(lo)) + (torch.arange(n, device=dev).float() + 0.5) * f32(vol.voxel_size)
    cz, cy, cx = torch.meshgrid(ax(nz, vol.lo[2]), ax(ny, vol.lo[1]), ax(nx, vol.lo[0]), indexing="ij")
    cx, cy, cz = cx.reshape(-1), cy.reshape(-1), cz.reshape(-1)
    tsdf, weight, color = vol.tsdf.reshape(-1), vol.weight.reshape(-1), vol.color.reshape(-1, 3)
    keep_t = torch.from_numpy(keep).to(dev)
    d_all, lab_all, rgb_all = depth.reshape(-1), labels.reshape(-1), rgb8.reshape(-1, 3)
    Tt, Kt = torch.from_numpy(T).to(dev), torch.from_numpy(np.ascontiguousarray(Ks.reshape(-1, 9))).to(dev)
    for c in range(T.shape[0]):
        A = Tt[c]
        q = [((A[4 * m] * cx + A[4 * m + 1] * cy) + A[4 * m + 2] * cz) + A[4 * m + 3] for m in range(3)]
        uf = ((Kt[c, 0] * (q[0] / q[2])) + Kt[c, 2]) - pc
        uf = uf + 0.5
        vf = ((Kt[c, 4] * (q[1] / q[2])) + Kt[c, 5]) - pc
        vf = vf + 0.5
        ok = (q[2] >= near) & (uf >= 0) & (uf < float(W)) & (vf >= 0) & (vf < float(H))
        u = torch.where(ok, torch.floor(uf), torch.zeros_like(uf)).long()
        v = torch.where(ok, torch.floor(vf), torch.zeros_like(vf)).long()
        p = (c * H + v) * W + u
        d = d_all[p]
        ok &= (d > 0) & (d < float("inf"))
        sdf = d - q[2]
        surface = keep_t[lab_all[p].long()] != 0
        upd = ok & torch.where(surface, ~(sdf < -trunc), sdf >= trunc)
        val = torch.where(surface, torch.clamp(sdf / trunc, max=1.0), torch.ones_like(sdf))
        w1 = weight + 1.0
        tsdf.copy_(torch.where(upd, ((tsdf * weight) + val) / w1, tsdf))
        color.copy_(torch.where((upd & surface)[:, None], ((color * weight[:, None]) + rgb_all[p].float()) / w1[:, None], color))
        weight.copy_(torch.where(upd, torch.clamp(w1, max=max_weight), weight))


def timed(fn, repeats, warm):
    for _ in range(warm):      # the clock ramp: the first calls after an idle spell run at a lower clock
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
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--n", type=int, default=292_247)
    ap.add_argument("--views", type=int, nargs="+", default=[2, 32])
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: no HIP device"
    sc = make_scene(a.n, seed=2, n_groups=G)
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=3, group_id=sc.group_id, n_groups=G)
    m = robot()
    r.upload_meshes(m["verts"], m["tris"], (0.7, 0.7, 0.75), groups=m["groups"])
    keep = cloud_keep_table(KEEP)
    lines = [f"# tools/fuse_probe.py: {a.n} Gaussians + {len(m['tris'])} triangles, ring cameras of {W}x{H}, a volume of {SIDE} m a side around the origin, "
             f"trunc 4 voxels, colour, labels, keep rows {KEEP[0]}..{KEEP[-1]} (the background carves); {torch.cuda.get_device_name(0)}",
             f"# medians of {a.repeats} blocking calls behind {a.warm} warm-up calls (torch baseline: {a.torch_repeats} behind 1), HIP events around the call, "
             f"host clock beside it; every fuse call starts from a fresh volume (the reset is outside the events)",
             "# traffic floor: 20 B read per voxel + 20 B written per touched voxel + 8 B per pixel (depth, label, rgb8) once"]
    ok = True
    for C in a.views:
        cams = [ring_camera(W, H, 262.0, yaw_deg=360.0 * k / C, elev=(0.0, 0.5, 1.0, -0.5)[k % 4]) for k in range(C)]
        V = np.stack([np.asarray(c.viewmat, np.float32) for c in cams])
        Ks = np.stack([np.asarray(c.K, np.float32) for c in cams])
        frames = lambda: r.render_batch_labels(V, Ks, W, H, want=("rgb8", "depth"), depth_fill_max=True)
        o, f_ms, f_min, f_max, f_host = timed(frames, a.repeats, a.warm)
        lines.append(f"C = {C} views: label frames with rgb8 and filled depth {f_ms:.3f} ms per call (min {f_min:.3f}, max {f_max:.3f}; host clock {f_host:.3f})")
        for n in a.dims:
            vol = TsdfVolume(r, (-0.5 * SIDE,) * 3, SIDE / n, dims=(n, n, n))

            def fuse(timing=False):
                vol.reset()
                torch.cuda.synchronize()
                vol.integrate(o["depth"], V, Ks, W, H, rgb8=o["rgb8"], labels=o["labels"], keep_labels=KEEP, timing=timing)

            def fuse_timed():          # events around the call alone: the reset is waited for first
                vol.reset()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                vol.integrate(o["depth"], V, Ks, W, H, rgb8=o["rgb8"], labels=o["labels"], keep_labels=KEEP)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

            for _ in range(a.warm):
                fuse_timed()
            runs = [fuse_timed() for _ in range(a.repeats)]
            ms = sorted(x[0] for x in runs)
            host = float(np.median([x[1] for x in runs]))
            got = [t.clone() for t in (vol.tsdf, vol.weight, vol.color)]
            fuse(timing=True)
            kernel = r.stage_times()["blend"]
            same = all(torch.equal(g, t) for g, t in zip(got, (vol.tsdf, vol.weight, vol.color)))
            touched = int((vol.weight > 0).sum())
            floor = 20 * n ** 3 + 20 * touched + 8 * C * H * W
            T = fuse_transforms(V)
            trunc = 4.0 * vol.voxel_size * float(np.cbrt(abs(np.linalg.det(V[0, :3, :3].astype(np.float64)))))

            def by_torch():
                vol.reset()
                torch_fuse(vol, o["depth"], o["rgb8"], o["labels"], Ks, T, keep, trunc)

            _, t_ms, t_lo, t_hi, t_host = timed(by_torch, a.torch_repeats, 1)
            equal = all(torch.equal(g, t) for g, t in zip(got, (vol.tsdf, vol.weight, vol.color)))
            ok = ok and same and equal
            med = float(np.median(ms))
            lines.append(f"  {n}^3 voxels: fuse call {med:.3f} ms (min {ms[0]:.3f}, max {ms[-1]:.3f}; host clock {host:.3f}); kernel alone {kernel:.3f} ms; "
                         f"{touched} voxels touched ({100.0 * touched / n ** 3:.1f} %); floor {floor / 1e6:.1f} MB = {floor / 1e6 / max(kernel, 1e-6):.0f} GB/s at the "
                         f"kernel's time; {n ** 3 * C / max(kernel, 1e-6) / 1e6:.1f} G voxel-views/s; repeated calls {'the same bytes' if same else 'DIFFERENT'}")
            lines.append(f"      torch on the GPU (reset included): {t_ms:.3f} ms (min {t_lo:.3f}, max {t_hi:.3f}; host clock {t_host:.3f}); volume "
                         f"{'equal' if equal else 'DIFFERENT'}; torch / HIP = {t_ms / med:.1f}" + ("" if med < t_ms else "   (the HIP call is NOT faster here)"))
            del vol, got
            torch.cuda.empty_cache()
    r.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
