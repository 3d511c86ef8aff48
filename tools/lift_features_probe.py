"""lift_features beside lift_labels and render_features: SAS_TIMING stage times of the same views on the same box in the same run, the
calls alternating, medians over the rounds (profiles/lift_features.txt).  render_features takes no SAS_TIMING: its rows hold the frame
total from device events around the calls, nothing per stage.

    python tools/lift_features_probe.py [--out FILE]     the Gym cameras (292 247 Gaussians, 32 views of 240x320) and one 1920x1080 view of
                                                         config 3, each for C in {3, 8, 32, 256}
    python tools/lift_features_probe.py --frames 4 [--channels 8]
                                                         only that many lift frames of the config-3 view: the probe of a counter pass
                                                         (python tools/pmc.py --kernels k_lift_features -- python tools/lift_features_probe.py --frames 4)
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

CHANNELS = (3, 8, 32, 256)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed_events(r, fn, views):
    """render_features takes no SAS_TIMING: device events around the call; only the frame total per view is known."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    nan = float("nan")
    return {"blend": nan, "sort": nan, "project": nan, "total": a.elapsed_time(b) / views}, views, wall


def timed(r, fn):
    r.stage_time_means(reset=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    ms, nf = r.stage_time_means(reset=True)
    return ms, nf, wall


def case(name, n, seed, ls, G, W, H, f, views, rounds):
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    cams = [ring_camera(W, H, f, yaw_deg=360.0 * k / views) for k in range(views)]
    Vs, Ks = np.stack([c.viewmat for c in cams]), np.stack([c.K for c in cams])
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    labels = r.render_batch_labels(Vs, Ks, W, H)["labels"]
    votes = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    seen = torch.zeros(n, dtype=torch.int64, device="cuda")
    weight = torch.zeros(n, dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    say(f"== {name}: {n} Gaussians, {views} view(s) of {W}x{H}")
    say(f"{'per view, ms (median of ' + str(rounds) + ' rounds [min..max])':58s} {'tile stage':>24s} {'sort':>8s} {'project':>8s} {'frame total':>12s} {'call wall/view':>15s}")
    for C in CHANNELS:
        images = torch.randn((views, H, W, C), device="cuda", generator=gen)
        feats = torch.randn((n, C), device="cuda", generator=gen)
        sums = torch.zeros((n, C), dtype=torch.int64, device="cuda")
        fout = {"features": torch.empty((H, W, C), device="cuda")}
        r.upload_features(feats)
        calls = {
            "plain full-sort frames (k_blend alone)": lambda: [r.render(Vs[v], Ks[v], W, H, want=("alpha",), full_sort=True, timing=True) for v in range(views)],
            "lift_labels (8 labels, votes + seen)": lambda: r.lift_labels(Vs, Ks, W, H, labels, 8, votes=votes, seen=seen, timing=True),
            f"render_features C={C}": lambda: [r.render_features(Vs[v], Ks[v], W, H, want=("features",), out=fout) for v in range(views)],
            f"lift_features C={C} (sums + weight)": lambda: r.lift_features(Vs, Ks, W, H, images, feature_scale=8000.0, sums=sums, weight=weight, timing=True),
            f"lift_features C={C} (weight only)": lambda: r.lift_features(Vs, Ks, W, H, images, feature_scale=8000.0, sums=False, weight=weight, timing=True),
        }
        for fn in calls.values():   # warm-up of every shape
            fn()
        res = {k: [] for k in calls}
        for _ in range(rounds):     # alternating
            for k, fn in calls.items():
                ms, nf, wall = timed_events(r, fn, views) if k.startswith("render_features") else timed(r, fn)
                assert nf == views, (k, nf)
                res[k].append((ms["blend"], ms["sort"], ms["project"], ms["total"], wall / views))
        med, tot = {}, {}
        for k, rows in res.items():
            a = np.array(rows)
            m = np.median(a, axis=0)
            med[k], tot[k] = m[0], m[3]
            say(f"{k:58s} {m[0]:8.3f} [{a[:, 0].min():.3f}..{a[:, 0].max():.3f}] {m[1]:8.3f} {m[2]:8.3f} {m[3]:12.3f} {m[4]:15.3f}")
        plain = med["plain full-sort frames (k_blend alone)"]
        chunks = (C + 7) // 8
        lift, lab = med[f"lift_features C={C} (sums + weight)"] - plain, med["lift_labels (8 labels, votes + seen)"] - plain
        ren = tot[f"render_features C={C}"] - tot["plain full-sort frames (k_blend alone)"]   # (frame totals: events around the calls against SAS_TIMING's)
        say(f"C={C}: tile stage minus k_blend: k_lift_features {lift:.3f} ms = {lift / chunks:.3f} ms per chunk of 8 ({chunks} chunks), k_lift_labels {lab:.3f} ms, "
            f"k_blend_features about {ren:.3f} ms = {ren / chunks:.3f} ms per chunk (from frame totals); per-chunk lift_features / lift_labels = {lift / chunks / lab:.2f}")
        say()
        del images, feats, sums
    r.close()


def frames_only(k, C):
    n, G, W, H = 1_000_000, 8, 1920, 1080
    sc = make_scene(n, seed=3, log_scale_mean=float(np.log(0.006)), n_groups=G)
    c = ring_camera(W, H, 1000.0)
    V, K = c.viewmat[None], c.K[None]
    r = Rasterizer(0)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    images = torch.randn((1, H, W, C), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    out = {}
    for _ in range(k):
        out = r.lift_features(V, K, W, H, images, feature_scale=8000.0, sums=out.get("sums"), weight=out.get("weight"))
    torch.cuda.synchronize()
    say(f"per frame: {float(out['weight'].sum()) / k / 2 ** 24:.0f} pixels' worth of weight, {int((out['weight'] > 0).sum())} Gaussians seen, "
        f"{int((out['sums'] != 0).sum())} (Gaussian, channel) cells added to")
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--channels", type=int, default=8)
    a = ap.parse_args()
    if a.frames > 0:
        frames_only(a.frames, a.channels)
        return
    say(f"device: {torch.cuda.get_device_name(0)}")
    case("Gym cameras", 292_247, 2, 0.01, 7, 320, 240, 262.5, 32, 5)
    case("config 3 (with 8 groups drawn for the label frames)", 1_000_000, 3, 0.006, 8, 1920, 1080, 1000.0, 1, 7)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
