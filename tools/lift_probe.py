"""lift_labels beside render_batch_labels: SAS_TIMING stage times of the same views on the same box in the same run, the calls
alternating (profiles/lift_labels.txt).

    python tools/lift_probe.py [--out FILE]        the Gym cameras (292 247 Gaussians, 32 views of 240x320) and one 1920x1080 view of config 3
    python tools/lift_probe.py --frames 4          only that many lift frames of the config-3 view: the probe of a counter pass
                                                   (python tools/pmc.py --kernels k_lift_labels -- python tools/lift_probe.py --frames 4)
Config 3 has no splat groups; eight are drawn for it here, since label frames need some."""
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


def timed(r, fn):
    r.stage_time_means(reset=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    ms, nf = r.stage_time_means(reset=True)
    return ms, nf, wall


def case(name, n, seed, ls, G, W, H, f, views, n_labels, rounds):
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    cams = [ring_camera(W, H, f, yaw_deg=360.0 * k / views) for k in range(views)]
    Vs, Ks = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    labels = r.render_batch_labels(Vs, Ks, W, H)["labels"]
    votes = torch.zeros((n, n_labels), dtype=torch.int64, device="cuda")
    seen = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = {"labels": torch.empty_like(labels)}
    calls = {
        "plain full-sort frames (k_blend alone)": lambda: [r.render(Vs[v], Ks[v], W, H, want=("alpha",), full_sort=True, timing=True) for v in range(views)],
        "render_batch_labels": lambda: r.render_batch_labels(Vs, Ks, W, H, out=out, timing=True),
        "lift_labels (votes + seen)": lambda: r.lift_labels(Vs, Ks, W, H, labels, n_labels, votes=votes, seen=seen, timing=True),
        "lift_labels (seen only)": lambda: r.lift_labels(Vs, Ks, W, H, labels, n_labels, votes=False, seen=seen, timing=True),
    }
    for fn in calls.values():   # warm-up of every shape
        fn()
        fn()
    st = r.stats()
    say(f"== {name}: {n} Gaussians, {G} groups, {views} view(s) of {W}x{H}, n_labels {n_labels}; last frame: {st['n_isect']} intersections, "
        f"longest list {st['max_tile_len']}")
    res = {k: [] for k in calls}
    for _ in range(rounds):     # alternating
        for k, fn in calls.items():
            ms, nf, wall = timed(r, fn)
            assert nf == views, (k, nf)
            res[k].append((ms["blend"], ms["sort"], ms["project"], ms["total"], wall))
    say(f"{'per view, ms (mean of ' + str(rounds) + ' rounds [min..max])':60s} {'tile stage':>22s} {'sort':>8s} {'project':>8s} {'frame total':>12s} {'call wall/view':>15s}")
    for k, rows in res.items():
        a = np.array(rows)
        say(f"{k:60s} {a[:, 0].mean():8.3f} [{a[:, 0].min():.3f}..{a[:, 0].max():.3f}] {a[:, 1].mean():8.3f} {a[:, 2].mean():8.3f} {a[:, 3].mean():12.3f} {a[:, 4].mean() / views:15.3f}")
    b = {k: np.array(v)[:, 0].mean() for k, v in res.items()}
    plain = b["plain full-sort frames (k_blend alone)"]
    say(f"tile stage minus k_blend: k_blend_labels {b['render_batch_labels'] - plain:.3f} ms, k_lift_labels {b['lift_labels (votes + seen)'] - plain:.3f} ms "
        f"(seen only {b['lift_labels (seen only)'] - plain:.3f} ms); lift / label tile stage = {b['lift_labels (votes + seen)'] / b['render_batch_labels']:.2f}")
    say()
    r.close()


def frames_only(k):
    n, G, W, H = 1_000_000, 8, 1920, 1080
    sc = make_scene(n, seed=3, log_scale_mean=float(np.log(0.006)), n_groups=G)
    c = ring_camera(W, H, 1000.0)
    V, K = c.viewmat[None], c.K[None]
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    labels = r.render_batch_labels(V, K, W, H)["labels"]
    out = None
    for _ in range(k):
        out = r.lift_labels(V, K, W, H, labels, 8, **(out or {}))
    torch.cuda.synchronize()
    say(f"per frame: {float(out['seen'].sum()) / k / 2 ** 32:.0f} pixels' worth of weight, {int((out['seen'] > 0).sum())} Gaussians seen, "
        f"{int((out['votes'] > 0).sum())} (Gaussian, label) cells voted for")
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=0)
    a = ap.parse_args()
    if a.frames > 0:
        frames_only(a.frames)
        return
    say(f"device: {torch.cuda.get_device_name(0)}")
    case("Gym cameras", 292_247, 2, 0.01, 7, 320, 240, 262.5, 32, 8, 5)
    case("config 3 (with 8 groups drawn for the label frames)", 1_000_000, 3, 0.006, 8, 1920, 1080, 1000.0, 1, 8, 8)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
