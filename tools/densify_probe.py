"""Density control on the resident scene beside the only alternative the library had before it: read_scene, the same rules in torch on the
device, upload (profiles/densify.txt).

    python tools/densify_probe.py [--out FILE] [--small]

Two scenes: the 292 247-Gaussian stand-in at a 240x320 Gym camera, and config 3's million at 1920x1080; SH degree 3, all five variable
groups stepped once so that the optimiser state exists and is carried.  The statistics are drawn so that about 10 % of the Gaussians are
cloned, 10 % split and 5 % pruned (the thresholds are percentiles of the scene).  Per scene, in one process on one box, medians over the
rounds after a warm-up, the scene uploaded and stepped anew (untimed) in front of every densify:

  density_accumulate     device events around the call, after a render_backward
  densify                wall time of the blocking call, and its parts as the library clocks them on the host (sas_scene_densify_times):
                         classes + totals read-back | scatter (enqueue) | storage order (enqueue) | relayout + state + the wait for all three
                           (under SAS_ORDER=0: rows + means read-back | storage_order, the host sort | relayout + state; tools/order_probe.py compares the two)
  reset_opacity          device events around the call
  torch alternative      read_scene -> masks, cat, randn children in torch on the device -> upload; it LOSES the optimiser moments (an
                         upload drops them), which densify carries"""
import argparse
import ctypes
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sim_a_splat_amd import fit  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

lines = []
WHAT = ("means", "opacities", "colors", "quats", "scales")


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def torch_densify(r, stats, cfg, sh_degree, gid, G):
    """The rules of sas_scene_densify in torch on read_scene's tensors, then upload: what a caller had to do before."""
    x = r.read_scene()
    smax = x["scales"].max(dim=1).values
    avg = stats["grad_sum"] / stats["count"].clamp(min=1)
    high = (stats["count"] > 0) & (avg > cfg["grow_grad2d"])
    small = smax <= cfg["grow_scale3d"] * cfg["scene_extent"]
    pruned = x["opacities"] < cfg["prune_opacity"]
    clone, split = high & small & ~pruned, high & ~small & ~pruned
    keep = ~pruned & ~split
    q = torch.nn.functional.normalize(x["quats"][split], dim=1)
    w, a, b, c = q.unbind(1)
    R = torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b), 2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a),
                     2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], dim=1).reshape(-1, 3, 3)
    kids = x["means"][split][:, None] + torch.einsum("pij,pcj->pci", R, x["scales"][split][:, None] * torch.randn(int(split.sum()), 2, 3, device=q.device))
    rep = lambda t: t[split].repeat_interleave(2, dim=0)
    new = {k: torch.cat([x[k][keep], x[k][clone], rep(x[k])]) for k in x}
    new["means"][-kids.shape[0] * 2:] = kids.reshape(-1, 3)
    new["scales"][-kids.shape[0] * 2:] = rep(x["scales"]) / cfg["split_factor"]
    g = None if gid is None else torch.cat([gid[keep], gid[clone], rep(gid)])
    r.upload(new["means"], new["opacities"], new["colors"], quats=new["quats"], scales=new["scales"], sh_degree=sh_degree, group_id=g, n_groups=G)
    return r.n


def case(name, n, seed, ls, G, W, H, f, rounds):
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    c = ring_camera(W, H, f)
    V, K = c.viewmat, c.K
    r = Rasterizer(0)
    dev = r.device
    gid = None if sc.group_id is None else torch.tensor(sc.group_id, device=dev)
    rng = np.random.default_rng(seed)
    grow = rng.random(n) < 0.2
    stats0 = dict(grad_sum=torch.tensor(np.where(grow, 1.0, 0.0).astype(np.float32), device=dev), count=torch.ones(n, dtype=torch.int32, device=dev),
                  max_radius=torch.zeros(n, device=dev))
    cfg = dict(grow_grad2d=0.5, grow_scale3d=float(np.median(sc.scales.max(axis=1))), scene_extent=1.0, prune_opacity=float(np.quantile(sc.opacities, 0.05)),
               split_factor=1.6, prune_scale_on=False)
    grads = {k: torch.randn(s, device=dev) * 1e-3 for k, s in dict(means=(n, 3), opacities=(n,), colors=(n, sc.sh.shape[1], 3), quats=(n, 4), scales=(n, 3)).items()}

    def fresh():   # the scene with optimiser state, as a fit holds it
        r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
        r.adam_step(grads, fit.DEFAULT_LRS, 1)
        return {k: v.clone() for k, v in stats0.items()}

    stats = fresh()
    g_rgb = torch.randn(H, W, 3, device=dev) / (3 * W * H)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:   # clocks up
        r.render(V, K, W, H)
    acc, dens, parts, alt, rst, counts = [], [], [], [], [], None
    times = (ctypes.c_float * 4)()
    for k in range(rounds + 1):
        stats = fresh()
        r.render_backward(V, K, W, H, g_rgb, want=("means",))
        a = events(lambda: r.density_accumulate(W, H, stats))
        stats = {k2: v.clone() for k2, v in stats0.items()}
        rs = events(lambda: r.reset_opacity(0.9999))   # (a cap nothing exceeds changes no decision below; the kernel's traffic is its reads)
        d, out = wall(lambda: r.densify(stats, **cfg))
        r._L.sas_scene_densify_times(r._ctx, times, 4)
        stats = fresh()
        t, n_alt = wall(lambda: torch_densify(r, stats, cfg, sc.sh_degree, gid, G))
        if k:   # (the first round warms allocators up)
            acc.append(a); dens.append(d); parts.append(list(times)); alt.append(t); rst.append(rs)
            counts = (out, n_alt)
    out, n_alt = counts
    med = lambda v: float(np.median(np.array(v), axis=0)) if np.ndim(v) == 1 else np.median(np.array(v), axis=0)
    p = med(parts)
    say(f"== {name}: {n} Gaussians, SH degree {sc.sh_degree}, {G} groups, backward frame {W}x{H}; medians of {rounds} rounds")
    say(f"densify: N {n} -> {out['n']}: cloned {out['cloned']} ({100 * out['cloned'] / n:.1f} %), split {out['split']} ({100 * out['split'] / n:.1f} %), "
        f"pruned {out['pruned']} ({100 * out['pruned'] / n:.1f} %); the torch alternative reaches N {n_alt}")
    say(f"  density_accumulate (device events)            {med(acc):9.3f} ms  [{min(acc):.3f}..{max(acc):.3f}]")
    say(f"  reset_opacity (device events)                 {med(rst):9.3f} ms  [{min(rst):.3f}..{max(rst):.3f}]")
    say(f"  densify, blocking call (wall)                 {med(dens):9.3f} ms  [{min(dens):.3f}..{max(dens):.3f}]")
    say(f"    classes + totals read-back                  {p[0]:9.3f} ms")
    say(f"    scatter: enqueue (SAS_ORDER=0: + read-back) {p[1]:9.3f} ms")
    say(f"    storage order: enqueue (SAS_ORDER=0: sort)  {p[2]:9.3f} ms   = {100 * p[2] / max(sum(p), 1e-9):.0f} % of the call's clocked parts")
    say(f"    allocation, relayout + state, commit        {p[3]:9.3f} ms")
    say(f"  read_scene -> torch rules -> upload (wall)    {med(alt):9.3f} ms  [{min(alt):.3f}..{max(alt):.3f}]   (loses the moments)")
    say(f"  alternative / densify = {med(alt) / med(dens):.2f}x")
    say()
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--small", action="store_true", help="the Gym-camera scene only")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}")
    case("Gym camera", 292_247, 2, 0.01, 7, 320, 240, 262.5, 5)
    if not a.small:
        case("config 3", 1_000_000, 3, 0.006, 0, 1920, 1080, 1000.0, 5)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
