"""render_backward beside the forward frame and lift_features with 3 channels: device-event times of the same views on the same box in the
same run, the calls alternating, medians over the rounds (profiles/render_backward.txt).

    python tools/grad_probe.py [--out FILE]     one 240x320 Gym-camera frame of the 292 247-Gaussian stand-in and one 1920x1080 view of
                                                config 3
    python tools/grad_probe.py --poses N [--out FILE]   the same two settings with N posed splat groups: render_backward for
                                                ("viewmat",), for ("group_poses",), and the full call with and without pose_groups
                                                (appended to FILE: profiles/group_pose_grad.txt).  Copied into the tools/ of a
                                                checkout of an earlier commit it times the rows that build has, for a comparison
                                                within one session.

Every row is a whole blocking call (projection, binning, sort, k_blend and what the call adds behind it).  The calls differ in what they
write besides: the two render rows write rgb, alpha and depth, the lift and backward rows write none of them.
Atomic bytes: k_grad_tiles hands every (list entry, tile) over with at most ten float atomics, so a frame adds at most
40 bytes x n_isect; the rate printed is that bound over the whole screen-space call, the kernel's share of which is smaller.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t) * 1e3


def case(name, n, seed, ls, G, W, H, f, rounds):
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    c = ring_camera(W, H, f)
    V, K = c.viewmat, c.K
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    gen = torch.Generator(device="cuda").manual_seed(1)
    g_rgb = torch.randn((H, W, 3), device="cuda", generator=gen)
    g_a = torch.randn((H, W), device="cuda", generator=gen)
    g_d = torch.randn((H, W), device="cuda", generator=gen)
    images = torch.randn((1, H, W, 3), device="cuda", generator=gen)
    sums = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    weight = torch.zeros(n, dtype=torch.int64, device="cuda")
    screen = r.render_backward(V, K, W, H, g_rgb, g_a, g_d, screen_space=True)
    full = r.render_backward(V, K, W, H, g_rgb, g_a, g_d)
    r.render(V, K, W, H, full_sort=True)
    n_isect = int(r.stats()["n_isect"])
    say(f"== {name}: {n} Gaussians, one view of {W}x{H}, n_isect {n_isect}")
    calls = {
        "forward frame (render)": lambda: r.render(V, K, W, H),
        "full-sort frame (k_blend on complete lists)": lambda: r.render(V, K, W, H, full_sort=True),
        "lift_features C=3 (sums + weight)": lambda: r.lift_features(V[None], K[None], W, H, images, feature_scale=8000.0, sums=sums, weight=weight),
        "render_backward screen_space (k_grad_tiles)": lambda: r.render_backward(V, K, W, H, g_rgb, g_a, g_d, screen_space=True, out=screen),
        "render_backward (k_grad_tiles + k_grad_project)": lambda: r.render_backward(V, K, W, H, g_rgb, g_a, g_d, out=full),
        "render_backward want=viewmat (a pose optimiser's)": lambda: r.render_backward(V, K, W, H, g_rgb, g_a, g_d, out=full, want=("viewmat",)),
    }
    for fn in calls.values():
        fn()
    res = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            res[k].append(timed(fn))
    med = {}
    say(f"{'ms, median of ' + str(rounds) + ' rounds [min..max]':52s} {'device events':>28s} {'call wall':>10s}")
    for k, rows in res.items():
        a = np.array(rows)
        m = np.median(a, axis=0)
        med[k] = m[0]
        say(f"{k:52s} {m[0]:8.3f} [{a[:, 0].min():.3f}..{a[:, 0].max():.3f}] {m[1]:10.3f}")
    fwd, fs = med["forward frame (render)"], med["full-sort frame (k_blend on complete lists)"]
    tiles = med["render_backward screen_space (k_grad_tiles)"]
    proj = med["render_backward (k_grad_tiles + k_grad_project)"] - tiles
    say(f"k_grad_project + k_grad_viewmat + the scratch memset (full minus screen-space call): {proj:.3f} ms")
    say(f"render_backward / forward frame = {med['render_backward (k_grad_tiles + k_grad_project)'] / fwd:.2f}; / full-sort frame = "
        f"{med['render_backward (k_grad_tiles + k_grad_project)'] / fs:.2f}; / lift_features C=3 = "
        f"{med['render_backward (k_grad_tiles + k_grad_project)'] / med['lift_features C=3 (sums + weight)']:.2f}")
    say(f"atomic bytes <= 40 B x n_isect = {40 * n_isect / 1e6:.1f} MB; over the screen-space call's {tiles:.3f} ms: <= {40 * n_isect / max(tiles, 1e-9) / 1e9:.3f} TB/s "
        f"(the chip-wide float-atomic rate is about 1.3 TB/s)")
    say()
    r.close()


def poses_case(name, n, seed, ls, W, H, f, rounds, n_poses):
    """The --poses leg: the scene with n_poses splat groups under random poses; the pose optimisers' calls and the full call with and
    without the pose gradient, alternating.  A library without sas_render_backward_poses (this file run from a checkout of an earlier
    commit) runs the rows it has: the unposed ones, for the comparison in one session."""
    from sim_a_splat_amd import _capi
    from sim_a_splat_amd.synthetic import random_group_poses
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=n_poses)
    c = ring_camera(W, H, f)
    V, K = c.viewmat, c.K
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=n_poses)
    r.set_group_poses(random_group_poses(n_poses, seed + 1))
    gen = torch.Generator(device="cuda").manual_seed(1)
    g_rgb = torch.randn((H, W, 3), device="cuda", generator=gen)
    g_a = torch.randn((H, W), device="cuda", generator=gen)
    g_d = torch.randn((H, W), device="cuda", generator=gen)
    posed = hasattr(_capi.lib(), "sas_render_backward_poses")
    groups = tuple(range(n_poses))
    full = r.render_backward(V, K, W, H, g_rgb, g_a, g_d)
    say(f"== {name}, {n_poses} posed groups: {n} Gaussians, one view of {W}x{H}; package {Path(_capi.__file__).resolve().parent.parent.name}, "
        f"{'with' if posed else 'WITHOUT'} sas_render_backward_poses")
    calls = {
        "render_backward want=viewmat": lambda: r.render_backward(V, K, W, H, g_rgb, g_a, g_d, out=full, want=("viewmat",)),
        "render_backward (no pose_groups)": lambda: r.render_backward(V, K, W, H, g_rgb, g_a, g_d, out=full),
    }
    if posed:
        fullp = r.render_backward(V, K, W, H, g_rgb, g_a, g_d, pose_groups=groups)
        calls[f"render_backward want=group_poses ({n_poses} groups)"] = lambda: r.render_backward(V, K, W, H, g_rgb, g_a, g_d, out=fullp, want=("group_poses",), pose_groups=groups)
        calls[f"render_backward pose_groups ({n_poses} groups)"] = lambda: r.render_backward(V, K, W, H, g_rgb, g_a, g_d, out=fullp, pose_groups=groups)
    for _ in range(3):   # warm-up: allocations, the clock ramp
        for fn in calls.values():
            fn()
    res = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            res[k].append(timed(fn))
    say(f"{'ms, median of ' + str(rounds) + ' rounds [min..max]':52s} {'device events':>28s} {'call wall':>10s}")
    for k, rows in res.items():
        a = np.array(rows)
        m = np.median(a, axis=0)
        say(f"{k:52s} {m[0]:8.3f} [{a[:, 0].min():.3f}..{a[:, 0].max():.3f}] {m[1]:10.3f}")
    say()
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--poses", type=int, default=0, help="N: time the pose-gradient calls with N posed groups instead (profiles/group_pose_grad.txt)")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}")
    if a.poses:
        poses_case("Gym camera", 292_247, 2, 0.01, 320, 240, 262.5, 15, a.poses)
        poses_case("config 3", 1_000_000, 3, 0.006, 1920, 1080, 1000.0, 11, a.poses)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    case("Gym camera", 292_247, 2, 0.01, 7, 320, 240, 262.5, 9)
    case("config 3", 1_000_000, 3, 0.006, 0, 1920, 1080, 1000.0, 7)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
