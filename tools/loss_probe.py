"""The photometric loss on the device beside the only ways the library had before it (profiles/photometric_loss.txt).

    python tools/loss_probe.py [--out FILE] [--small]

Two scenes: the 292 247-Gaussian stand-in at a 240x320 Gym camera, and config 3 (1 M Gaussians at 1920x1080).  Per scene, in one process
on one box, device-event times, the calls alternating, medians over the rounds with min..max, after a warm-up that brings the clocks up
(tools/ramp_probe.py).  A loss call is tens of microseconds, so a timed window holds REPS calls back to back and is divided by REPS:

  (a)  Rasterizer.photometric_loss, prechained, at lambda = 0.2 and at lambda = 0
  (b)  the same loss in torch: five grouped 11x11 conv2d, autograd, autograd.prechain -- the only way before the kernels
  (c)  fit.l1_loss_and_grad + autograd.prechain: what fit_scene runs without ``loss``
  (d)  the whole iteration (render, loss, render_backward, adam_step) with loss="dssim", beside the whole iteration of (c) and of (b)

Comparisons stated at the end of each scene: (a) at 0.2 below (b) with ranges that do not overlap; (a) at 0 not above (c).
The kernels' algorithmic bytes per pixel: k_loss_stats reads x and y (24) and writes nine partial planes (36); k_loss_grad reads the planes
(36; the halo re-reads hit the cache), x and y (24) and writes g_rgb and g_alpha (16): 136, against a first estimate of about 120."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sim_a_splat_amd import fit  # noqa: E402
from sim_a_splat_amd.autograd import prechain  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

lines = []
WHAT = ("means", "opacities", "colors", "quats", "scales")
LRS = dict(fit.DEFAULT_LRS)
ROOF_TBS = 8.0
REPS = 20
BYTES_PER_PIXEL = 136
LAMBDA = 0.2


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t) * 1e3 / reps


def window(dev):
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))
    g = (g / g.sum()).float().to(dev)
    return (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()


def torch_dssim(rgb, target, kern, lam):
    """(loss, g_rgb): the definition through conv2d and autograd."""
    x = rgb.detach().requires_grad_(True)
    X, Y = x.permute(2, 0, 1)[None], target.permute(2, 0, 1)[None]
    blur = lambda a: torch.nn.functional.conv2d(a, kern, padding=5, groups=3)
    mx, my = blur(X), blur(Y)
    vx, vy, cxy = blur(X * X) - mx * mx, blur(Y * Y) - my * my, blur(X * Y) - mx * my
    ssim = (((2 * mx * my + 1e-4) * (2 * cxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))).mean()
    loss = (1.0 - lam) * (X - Y).abs().mean() + lam * (1.0 - ssim)
    loss.backward()
    return loss.detach(), x.grad


def case(name, n, seed, ls, G, W, H, f, rounds):
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    c = ring_camera(W, H, f)
    V, K = c.viewmat, c.K
    bg = (0.0, 0.0, 0.0)
    r = Rasterizer(0)
    up = dict(sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, **up)
    target = r.render(V, K, W, H, bg)["rgb"].clone()
    r.upload(sc.means, sc.opacities * 0.7, sc.sh * 0.8, quats=sc.quats, scales=sc.scales, **up)
    frame = {k: v.clone() for k, v in r.render(V, K, W, H, bg).items()}
    kern = window(r.device)
    step = [0]

    def hip_loss(lam):
        return r.photometric_loss(frame["rgb"], target, alpha=frame["alpha"], background=bg, lambda_dssim=lam)

    def torch_loss():
        _, g = torch_dssim(frame["rgb"], target, kern, LAMBDA)
        return prechain(frame["rgb"], frame["alpha"], frame["depth"], bg, g, None, None)

    def l1_loss():
        _, g = fit.l1_loss_and_grad(frame["rgb"], target, None)
        return prechain(frame["rgb"], frame["alpha"], frame["depth"], bg, g, None, None)

    def iteration(kind):
        out = r.render(V, K, W, H, bg)
        if kind == "hip":
            pl = r.photometric_loss(out["rgb"], target, alpha=out["alpha"], background=bg, lambda_dssim=LAMBDA)
            g_acc, g_a = pl["g_rgb"], pl["g_alpha"]
        else:
            g = torch_dssim(out["rgb"], target, kern, LAMBDA)[1] if kind == "torch" else fit.l1_loss_and_grad(out["rgb"], target, None)[1]
            g_acc, g_a, _ = prechain(out["rgb"], out["alpha"], out["depth"], bg, g, None, None)
        step[0] += 1
        r.adam_step(r.render_backward(V, K, W, H, g_acc, g_a, None, want=WHAT), LRS, step[0])

    calls = {"(a) photometric_loss, lambda 0.2": (lambda: hip_loss(LAMBDA), REPS), "(a) photometric_loss, lambda 0": (lambda: hip_loss(0.0), REPS),
             "(b) torch conv2d + autograd + prechain, lambda 0.2": (torch_loss, REPS), "(c) l1_loss_and_grad + prechain": (l1_loss, REPS),
             "(d) whole iteration, loss=\"dssim\"": (lambda: iteration("hip"), 1), "(d) whole iteration, the parent's L1 path": (lambda: iteration("l1"), 1),
             "(d) whole iteration, the torch form of (b)": (lambda: iteration("torch"), 1)}
    # the same loss three ways, before anything is timed
    a, (gb, gab, _) = hip_loss(LAMBDA), torch_loss()
    scale = float(gb.abs().max())
    say(f"== {name}: {n} Gaussians, one view of {W}x{H}; windows of {REPS} loss calls, {rounds} rounds")
    say(f"(a) against (b) on this frame: loss {float(a['loss']):.6e} / {float(torch_dssim(frame['rgb'], target, kern, LAMBDA)[0]):.6e}, "
        f"max |g_rgb - g_rgb(b)| / max |g_rgb(b)| = {float((a['g_rgb'] - gb).abs().max()) / scale:.2e}, max |g_alpha - g_alpha(b)| = {float((a['g_alpha'] - gab).abs().max()):.2e} (background 0: both are 0)")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:   # clocks up
        r.render(V, K, W, H, bg)
    for fn, _ in calls.values():
        fn()
    res = {k: [] for k in calls}
    for _ in range(rounds):
        for k, (fn, reps) in calls.items():
            res[k].append(timed(fn, reps))
    say(f"{'ms per call, median of ' + str(rounds) + ' rounds [min..max]':54s} {'device events':>28s} {'call wall':>10s}")
    rng = {}
    for k, rows in res.items():
        t = np.array(rows)
        m = np.median(t, axis=0)
        rng[k] = (m[0], t[:, 0].min(), t[:, 0].max())
        say(f"{k:54s} {m[0]:8.4f} [{t[:, 0].min():.4f}..{t[:, 0].max():.4f}] {m[1]:10.4f}")
    a2, a0, b, c = (rng[k] for k in list(calls)[:4])
    byts = BYTES_PER_PIXEL * W * H
    say(f"(a) at lambda 0.2: {BYTES_PER_PIXEL} algorithmic bytes per pixel, {byts / 1e6:.1f} MB; {byts / (a2[0] * 1e-3) / 1e12:.3f} TB/s achieved = "
        f"{100 * byts / (a2[0] * 1e-3) / 1e12 / ROOF_TBS:.1f} % of the {ROOF_TBS:.0f} TB/s roof (device events around three launches: launch latency included)")
    say(f"comparison 1: (a) at lambda 0.2 below (b), ranges apart: {a2[0]:.4f} [{a2[1]:.4f}..{a2[2]:.4f}] against {b[0]:.4f} [{b[1]:.4f}..{b[2]:.4f}], "
        f"{b[0] / a2[0]:.1f}x -- {'MET' if a2[2] < b[1] else 'NOT MET'}")
    say(f"comparison 2: (a) at lambda 0 not above (c): {a0[0]:.4f} [{a0[1]:.4f}..{a0[2]:.4f}] against {c[0]:.4f} [{c[1]:.4f}..{c[2]:.4f}] -- "
        f"{'MET' if a0[0] <= c[0] else 'NOT MET'}")
    d = [rng[k] for k in list(calls)[4:]]
    say(f"whole iteration: loss=\"dssim\" {d[0][0]:.3f} ms, the parent's L1 path {d[1][0]:.3f} ms, the torch form {d[2][0]:.3f} ms")
    say()
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--small", action="store_true", help="the Gym-camera scene only")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}")
    case("Gym camera", 292_247, 2, 0.01, 7, 320, 240, 262.5, 9)
    if not a.small:
        case("config 3", 1_000_000, 3, 0.006, 0, 1920, 1080, 1000.0, 7)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
