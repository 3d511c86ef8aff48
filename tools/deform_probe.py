"""The deformation step of a resident scene beside the only way there was before it: torch ops on read_scene() tensors, then upload
(profiles/deform.txt).

    python tools/deform_probe.py [--out FILE] [--sizes 292247,1000000] [--nodes 64,1024,16384] [--ks 4,8] [--rounds 5] [--resources]

ONE process, two contexts on one box: the LDS arm is a default context (node records staged in LDS while they fit SAS_SKIN_LDS), the GLOBAL
arm is created under SAS_SKIN_LDS=0 (every lane reads its records from global memory).  The rounds alternate the arms; one warm-up round;
medians and [min..max] over the rounds; device events around what only enqueues (deform, knn), the wall clock around what blocks (bind_skin,
frames, the torch baseline with its upload).  Per scene -- the 292 247-Gaussian stand-in and config 3's million -- and per (m, k):

  deform alone; bind_skin; the same deformation as torch ops on read_scene() tensors followed by upload (the baseline);
  deform + frame beside the frame alone, at config 1's camera (256 x 256, the Gym-sized view) and at 1920 x 1080;
  the frame's window misses and tile-kernel time (the median of the rounds' timed frames, after an untimed one) at rest and after a
  LARGE deformation (a parabolic bend whose far end moves by half the scene's extent), under the stale storage order and under one
  renewed by an upload of the deformed scene: what the order of the rest pose costs once a workgroup's Gaussians spread on screen;
  k_deform's bytes per microsecond beside k_adam_scene's in the same run (means, opacities, quaternions and scales stepped: 396 B per
  Gaussian -- 96 of planes, 256 of state, 44 of gradients; k_deform: 96 of planes plus 32 (k <= 4) or 64 of skin).

The nodes are a seeded draw of m of the scene's own means.  The deformed scenes of the two arms are compared bit for bit."""
import argparse
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import config_cameras, config_scene_and_cameras, make_scene  # noqa: E402

lines = []
LRS = dict(means=1.6e-4, opacities=5e-2, quats=1e-3, scales=5e-3)
ADAM_BYTES = 396


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def context(lds):
    old = os.environ.pop("SAS_SKIN_LDS", None)
    if not lds:
        os.environ["SAS_SKIN_LDS"] = "0"
    try:
        return Rasterizer(0)
    finally:
        os.environ.pop("SAS_SKIN_LDS", None)
        if old is not None:
            os.environ["SAS_SKIN_LDS"] = old


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def bend(nodes, amount):
    """[m,3,4] float32: a parabolic bend along x -- a node at x moves by amount * u^2 in y (u = its x offset over the half extent) and
    turns about z by the bend's slope; rigid per node."""
    c = nodes.astype(np.float64)
    cx, hx = 0.5 * (c[:, 0].max() + c[:, 0].min()), max(0.5 * (c[:, 0].max() - c[:, 0].min()), 1e-9)
    u = (c[:, 0] - cx) / hx
    a = np.arctan(2.0 * amount * u / hx)
    R = np.zeros((c.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
    moved = c + np.stack([np.zeros_like(u), amount * u * u, np.zeros_like(u)], axis=1)
    t = moved - np.einsum("mij,mj->mi", R, c)
    return np.ascontiguousarray(np.concatenate([R, t[:, :, None]], axis=2).astype(np.float32))


def torch_deform(x, idx, w, G):
    """The deformation of quaternion scenes as elementwise torch on device tensors (the baseline's arithmetic: what a user would write)."""
    m = G.shape[0]
    R, t = G[:, :, :3], G[:, :, 3]
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    qw = torch.sqrt(torch.clamp(1.0 + tr, min=1e-12)) * 0.5   # (the probe's bends stay on the trace branch)
    q = torch.stack([qw, (R[:, 2, 1] - R[:, 1, 2]) / (4 * qw), (R[:, 0, 2] - R[:, 2, 0]) / (4 * qw), (R[:, 1, 0] - R[:, 0, 1]) / (4 * qw)], dim=1)
    live = (idx >= 0) & (idx < m) & (w > 0)
    ic = torch.where(live, idx, torch.zeros_like(idx)).long()
    wl = torch.where(live, w, torch.zeros_like(w))
    mean = x["means"]
    y = torch.einsum("nkij,nj->nki", R[ic], mean) + t[ic]
    W = wl.sum(dim=1, keepdim=True).clamp_min(1e-30)
    means = mean + (wl[:, :, None] * (y - mean[:, None, :])).sum(dim=1) / W
    qj = q[ic]
    s = torch.where((qj * qj[:, :1]).sum(dim=2) < 0, -wl, wl)
    qb = torch.nn.functional.normalize((s[:, :, None] * qj).sum(dim=1), dim=1)
    any_ = live.any(dim=1, keepdim=True)
    qb = torch.where(any_, qb, torch.tensor([1.0, 0.0, 0.0, 0.0], device=qb.device))
    bw, bx, by, bz = qb.unbind(1)
    rw, rx, ry, rz = x["quats"].unbind(1)
    quats = torch.stack([bw * rw - bx * rx - by * ry - bz * rz, bw * rx + bx * rw + by * rz - bz * ry,
                         bw * ry - bx * rz + by * rw + bz * rx, bw * rz + bx * ry - by * rx + bz * rw], dim=1)
    return means, quats


def tile_stats(r, cam, frame, rounds):
    """(window misses, median tile-kernel ms over ``rounds`` timed frames) of the context's scene at ``cam``, after one untimed frame."""
    frame(r, cam)
    t = []
    for _ in range(max(rounds, 1)):
        frame(r, cam, timing=True)
        t.append(r.stage_times()["blend"])
    return r.stats()["window_misses"], float(np.median(t))


def med(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def fmt(v):
    a, lo, hi = med(v)
    return f"{a:10.3f}   [{lo:.3f}..{hi:.3f}]"


def case(n, node_counts, ks, rounds, arms):
    if n == 1_000_000:
        sc = config_scene_and_cameras(3)[0]
    else:
        sc = make_scene(n, seed=2, log_scale_mean=float(np.log(0.01)))
    n = sc.means.shape[0]
    dev = arms["lds"].device
    x = {k: torch.tensor(v, device=dev) for k, v in dict(means=sc.means, opacities=sc.opacities, colors=sc.sh, quats=sc.quats, scales=sc.scales).items()}
    extent = float(np.ptp(sc.means[:, 0]))
    cams = {"256 x 256": config_cameras(1)[0], "1920 x 1080": config_cameras(3)[0]}

    def upload(r, means=None, quats=None):
        r.upload(x["means"] if means is None else means, x["opacities"], x["colors"], quats=x["quats"] if quats is None else quats,
                 scales=x["scales"], sh_degree=sc.sh_degree)

    def frame(r, cam, timing=False):
        return r.render(cam.viewmat, cam.K, cam.width, cam.height, (0.0, 0.0, 0.0), want=("rgb",), timing=timing)

    say(f"== {n} Gaussians, SH degree {sc.sh_degree}; medians of {rounds} rounds [min..max], ms; arms alternating")
    for r in arms.values():
        upload(r)
    # k_adam_scene in the same run: the streaming kernel k_deform is measured against
    grads = {k: torch.randn(x[k].shape, device=dev) * 1e-4 for k in ("means", "opacities", "quats", "scales")}
    t_adam = []
    for k in range(rounds + 1):
        ms, _ = events(lambda: arms["lds"].adam_step(grads, LRS, k + 1))
        if k:
            t_adam.append(ms)
    adam_rate = n * ADAM_BYTES / (med(t_adam)[0] * 1e3)
    say(f"   adam_step (means, opacities, quats, scales)      {fmt(t_adam)}   {adam_rate:9.0f} B/us at {ADAM_BYTES} B per Gaussian")
    for r in arms.values():
        upload(r)
    t_frame = {name: [] for name in cams}
    rest_stats = {}
    for k in range(rounds + 1):
        for name, cam in cams.items():
            ms, _ = wall(lambda: frame(arms["lds"], cam))
            if k:
                t_frame[name].append(ms)
    for name, cam in cams.items():
        rest_stats[name] = tile_stats(arms["lds"], cam, frame, rounds)
        say(f"   frame alone, {name:12s} (wall)                  {fmt(t_frame[name])}   at rest: window misses {rest_stats[name][0]}, tile kernel {rest_stats[name][1]:.3f} ms")
    ok = True
    for m in node_counts:
        nodes = np.ascontiguousarray(sc.means[np.random.default_rng(7).choice(n, m, replace=False)])
        G_small, G_large = (torch.from_numpy(bend(nodes, a * extent)).to(dev) for a in (0.05, 0.5))
        for kk in ks:
            t = {a: {"deform": [], "bind": []} for a in arms}
            t_torch, t_with = [], {name: [] for name in cams}
            got = {}
            for k in range(rounds + 1):
                for arm, r in arms.items():   # the arms alternate inside every round
                    ms_b, bound = wall(lambda: r.bind_skin(nodes, k=kk))
                    ms_d, _ = events(lambda: r.deform(G_small))
                    got[arm] = r.read_scene()
                    if k:
                        t[arm]["bind"].append(ms_b)
                        t[arm]["deform"].append(ms_d)
                r = arms["lds"]
                for name, cam in cams.items():
                    ms, _ = wall(lambda: (r.deform(G_small), frame(r, cam)))
                    if k:
                        t_with[name].append(ms)
                idx, w = bound["indices"], bound["weights"]
                ms, _ = wall(lambda: upload(arms["global"], *torch_deform(x, idx, w, G_small)))
                if k:
                    t_torch.append(ms)
                upload(arms["global"])
            same = all(torch.equal(got["lds"][a], got["global"][a]) for a in got["lds"])
            ok = ok and same
            dev_t = float((got["lds"]["means"] - torch_deform(x, idx, w, G_small)[0]).abs().max())
            bytes_per = 96 + (32 if kk <= 4 else 64)
            rate = n * bytes_per / (med(t["lds"]["deform"])[0] * 1e3)
            path = "LDS" if m * 64 <= 16384 else "global (m * 64 B is beyond the LDS budget)"
            say(f"-- m = {m} nodes, k = {kk}: the default context takes the {path} path; the arms' scenes are {'identical bits' if same else 'DIFFERENT'}; "
                f"torch's means differ from the kernel's by up to {dev_t:.1e}")
            say(f"   deform alone (events), default context          {fmt(t['lds']['deform'])}   {rate:9.0f} B/us at {bytes_per} B per Gaussian = "
                f"{rate / adam_rate:.2f} x k_adam_scene's rate")
            say(f"   deform alone (events), SAS_SKIN_LDS=0           {fmt(t['global']['deform'])}")
            say(f"   bind_skin (wall: read_scene, kNN, weights, set) {fmt(t['lds']['bind'])}")
            say(f"   torch ops on read_scene() + upload (wall)       {fmt(t_torch)}   {med(t_torch)[0] / med(t['lds']['deform'])[0]:8.1f} x deform alone")
            for name in cams:
                say(f"   deform + frame, {name:12s} (wall)             {fmt(t_with[name])}   frame alone {med(t_frame[name])[0]:.3f}")
        # the stale storage order: the same frames after a large bend (k of the last binding)
        r = arms["lds"]
        r.deform(G_large)
        for name, cam in cams.items():
            a = tile_stats(r, cam, frame, rounds)
            s = r.read_scene()
            fresh = arms["global"]   # the same deformed scene in a storage order of its own (its skin goes with the upload)
            fresh.upload(s["means"], s["opacities"], s["colors"], quats=s["quats"], scales=s["scales"], sh_degree=sc.sh_degree)
            b = tile_stats(fresh, cam, frame, rounds)
            upload(fresh)
            say(f"   bend of half the extent, m = {m}, {name:12s}: window misses {rest_stats[name][0]} at rest -> {a[0]} (stale order) | {b[0]} (order renewed by "
                f"an upload); tile kernel {rest_stats[name][1]:.3f} -> {a[1]:.3f} | {b[1]:.3f} ms")
        for rr in arms.values():
            rr.clear_skin()
    say()
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="292247,1000000")
    ap.add_argument("--nodes", default="64,1024,16384")
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resources", action="store_true", help="append the kernels' registers, LDS and occupancy (compiles the library once more)")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}")
    arms = {"lds": context(True), "global": context(False)}
    t0 = time.perf_counter()
    warm = torch.randn(1 << 18, 3, device=arms["lds"].device)
    while time.perf_counter() - t0 < 1.0:   # clocks up
        arms["lds"].knn_nodes(warm, warm[:256], 4)
        torch.cuda.synchronize()
    ok = True
    for n in (int(s) for s in a.sizes.split(",")):
        ok = case(n, [int(s) for s in a.nodes.split(",")], [int(s) for s in a.ks.split(",")], a.rounds, arms) and ok
    for r in arms.values():
        r.close()
    if a.resources:
        for filt in ("k_deform", "k_knn_cross", "k_skin"):
            say(f"kernel resources (tools/kernel_resources.py {filt}):")
            say(subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_resources.py"), filt], capture_output=True, text=True).stdout.rstrip())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
