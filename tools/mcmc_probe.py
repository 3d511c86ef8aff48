"""MCMC density control on the resident scene: what the noise costs every step, and what a refine costs beside a densify
(profiles/mcmc.txt).

    python tools/mcmc_probe.py [--out FILE] [--small]

Two scenes: the 292 247-Gaussian stand-in at a 240x320 Gym camera, and config 3's million at 1920x1080; SH degree 3, all five variable
groups stepped so that the optimiser state exists and is carried.  A tenth of the opacities are set below min_opacity (dead), so a refine
relocates 10 % and adds 5 %.  Per scene, in one process on one box, medians over the rounds after a warm-up:

  mcmc_noise, adam_step    device events around each call, alternating in the same loop; bytes per Gaussian / time = the rate each reaches
                           (noise: perm + three 16-byte planes read + one written = 68 B; adam_step with all five groups at SH degree 3:
                           the planes, the gradients and the moments, 1 740 B)
  iteration                render + photometric_loss + render_backward + adam_step, with and without mcmc_noise behind it (wall, synchronised)
  mcmc_refine              wall time of the blocking call, and its parts as the library clocks them on the host (sas_scene_densify_times):
                           weights + totals read-back | draws, rows (enqueue) | storage order (enqueue) | relayout + state + the wait for all three
                           (under SAS_ORDER=0: rows + means read-back | storage_order, the host sort | relayout + state; tools/order_probe.py compares the two)
  densify                  the same scene and state through the default strategy's call (about 10 % cloned, 10 % split, 5 % pruned), for scale"""
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
NOISE_BYTES = 4 + 4 * 16
ADAM_BYTES = 1740   # adam_step, five groups, SH degree 3: the algorithmic bytes per Gaussian DESIGN.md 3, "Optimiser step" counts


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


def case(name, n, seed, ls, G, W, H, f, rounds):
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    c = ring_camera(W, H, f)
    V, K = c.viewmat, c.K
    r = Rasterizer(0)
    dev = r.device
    rng = np.random.default_rng(seed)
    op = sc.opacities.copy()
    op[rng.random(n) < 0.1] = np.float32(0.001)
    grads = {k: torch.randn(s, device=dev) * 1e-3 for k, s in dict(means=(n, 3), opacities=(n,), colors=(n, sc.sh.shape[1], 3), quats=(n, 4), scales=(n, 3)).items()}
    grow = rng.random(n) < 0.2
    stats0 = dict(grad_sum=torch.tensor(np.where(grow, 1.0, 0.0).astype(np.float32), device=dev), count=torch.ones(n, dtype=torch.int32, device=dev),
                  max_radius=torch.zeros(n, device=dev))
    dcfg = dict(grow_grad2d=0.5, grow_scale3d=float(np.median(sc.scales.max(axis=1))), scene_extent=1.0, prune_opacity=float(np.quantile(sc.opacities, 0.05)),
                split_factor=1.6, prune_scale_on=False)

    def fresh():   # the scene with optimiser state, as a fit holds it
        r.upload(sc.means, op, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
        r.adam_step(grads, fit.DEFAULT_LRS, 1)

    fresh()
    target = r.render(V, K, W, H)["rgb"].clone()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:   # clocks up
        r.render(V, K, W, H)

    def iteration(t, noise):
        out = r.render(V, K, W, H)
        pl = r.photometric_loss(out["rgb"], target, alpha=out["alpha"])
        acc = r.render_backward(V, K, W, H, pl["g_rgb"], pl["g_alpha"], None, want=WHAT)
        r.adam_step(acc, fit.DEFAULT_LRS, t)
        if noise:
            r.mcmc_noise(1.0, t, 0)

    # the two kernels in one loop, and the iteration with and without the noise, interleaved
    tn, ta, it0, it1 = [], [], [], []
    for k in range(3 + 20):
        a = events(lambda: r.adam_step(grads, fit.DEFAULT_LRS, 2 + k))
        b = events(lambda: r.mcmc_noise(1e-3, 2 + k, 0))
        x, _ = wall(lambda: iteration(30 + k, False))
        y, _ = wall(lambda: iteration(30 + k, True))
        if k >= 3:
            ta.append(a); tn.append(b); it0.append(x); it1.append(y)
    ref, parts, dens, dparts, counts = [], [], [], [], None
    times = (ctypes.c_float * 4)()
    for k in range(rounds + 1):
        fresh()
        d, out = wall(lambda: r.mcmc_refine(cap_max=2 * n, seed=k))
        r._L.sas_scene_densify_times(r._ctx, times, 4)
        p = list(times)
        fresh()
        stats = {k2: v.clone() for k2, v in stats0.items()}
        e, dout = wall(lambda: r.densify(stats, **dcfg))
        r._L.sas_scene_densify_times(r._ctx, times, 4)
        if k:   # (the first round warms allocators up)
            ref.append(d); parts.append(p); dens.append(e); dparts.append(list(times))
            counts = (out, dout)
    out, dout = counts
    med = lambda v: float(np.median(np.array(v)))
    p, dp = np.median(np.array(parts), axis=0), np.median(np.array(dparts), axis=0)
    say(f"== {name}: {n} Gaussians, SH degree {sc.sh_degree}, {G} groups, frame {W}x{H}")
    say(f"  mcmc_noise (device events, 20 calls)          {1e3 * med(tn):9.1f} us  [{1e3 * min(tn):.1f}..{1e3 * max(tn):.1f}]   {NOISE_BYTES} B/Gaussian -> {n * NOISE_BYTES / (med(tn) * 1e-3) / 1e12:.2f} TB/s")
    say(f"  adam_step, five groups (device events)        {1e3 * med(ta):9.1f} us  [{1e3 * min(ta):.1f}..{1e3 * max(ta):.1f}]   {ADAM_BYTES} B/Gaussian -> {n * ADAM_BYTES / (med(ta) * 1e-3) / 1e12:.2f} TB/s")
    say(f"  iteration without noise (wall, synchronised)  {med(it0):9.3f} ms  [{min(it0):.3f}..{max(it0):.3f}]")
    say(f"  iteration with noise                          {med(it1):9.3f} ms  [{min(it1):.3f}..{max(it1):.3f}]   difference of the medians {1e3 * (med(it1) - med(it0)):+.0f} us")
    say(f"  mcmc_refine: N {n} -> {out['n']}: relocated {out['relocated']} ({100 * out['relocated'] / n:.1f} %), added {out['added']} ({100 * out['added'] / n:.1f} %); medians of {rounds} rounds")
    say(f"  mcmc_refine, blocking call (wall)             {med(ref):9.3f} ms  [{min(ref):.3f}..{max(ref):.3f}]")
    say(f"    weights + totals read-back                  {p[0]:9.3f} ms")
    say(f"    draws, rows: enqueue (SAS_ORDER=0: + r.-b.) {p[1]:9.3f} ms")
    say(f"    storage order: enqueue (SAS_ORDER=0: sort)  {p[2]:9.3f} ms   = {100 * p[2] / max(sum(p), 1e-9):.0f} % of the call's clocked parts")
    say(f"    allocation, relayout + state, commit        {p[3]:9.3f} ms")
    say(f"  densify: N {n} -> {dout['n']} (cloned {dout['cloned']}, split {dout['split']}, pruned {dout['pruned']})")
    say(f"  densify, blocking call (wall)                 {med(dens):9.3f} ms  [{min(dens):.3f}..{max(dens):.3f}]   parts {dp[0]:.3f} | {dp[1]:.3f} | {dp[2]:.3f} | {dp[3]:.3f} ms")
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
