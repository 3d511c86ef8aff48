"""The storage order on the device beside the host function it replaces (profiles/storage_order.txt).

    python tools/order_probe.py [--out FILE] [--sizes 20000,292247,1000000] [--rounds 5] [--settle MS] [--resources]

ONE process, two contexts on one box: the HOST arm is created under SAS_ORDER=0 (storage_order() of sas_api.cpp on read-back means and
group ids: the library's path before the device sort existed), the DEVICE arm is a default context (sas_order.hip).  The rounds alternate
the arms; the figures are medians over the rounds after one warm-up round.  Per size -- 20 000, the 292 247-Gaussian stand-in, config 3's
million; SH degree 3, all five variable groups stepped once so that the optimiser state exists and is carried, the scene uploaded and
stepped anew (untimed) in front of every timed call:

  storage_order    Rasterizer.storage_order on device tensors, device events around the call (device arm's kernels; on either context)
  upload           wall time of the blocking call from device tensors
  densify, off     wall time of densify with every switch off: the order renewed alone; and the library's own laps (sas_scene_densify_times)
  densify, mix     ... at tools/densify_probe.py's mix: about 10 % cloned, 10 % split, 5 % pruned
  mcmc_refine      wall time at 5 % dead, grow_factor 1.05

The host arm's lap 2 is the host sort alone: the reference of the standalone figure."""
import argparse
import ctypes
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sim_a_splat_amd import fit  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402

lines = []
OFF = dict(grow=False, prune_opacity_on=False, prune_scale_on=False)
SCENES = {20_000: (1, 0.02, 3), 292_247: (2, 0.01, 7), 1_000_000: (3, 0.006, 0)}   # n -> (seed, scale, groups)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def context(host_order):
    old = os.environ.pop("SAS_ORDER", None)
    if host_order:
        os.environ["SAS_ORDER"] = "0"
    try:
        return Rasterizer(0)
    finally:
        os.environ.pop("SAS_ORDER", None)
        if old is not None:
            os.environ["SAS_ORDER"] = old


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


SETTLE = 0.0   # seconds the box idles between the untimed preparation and a timed blocking call (--settle)


def wall(fn):
    torch.cuda.synchronize()
    if SETTLE:
        time.sleep(SETTLE)
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def case(n, rounds):
    seed, ls, G = SCENES.get(n, (4, 0.01, 0))
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    arms = {"host": context(True), "device": context(False)}
    dev = arms["device"].device
    x = {k: torch.tensor(v, device=dev) for k, v in dict(means=sc.means, opacities=sc.opacities, colors=sc.sh, quats=sc.quats, scales=sc.scales).items()}
    gid = None if sc.group_id is None else torch.tensor(sc.group_id, device=dev)
    rng = np.random.default_rng(seed)
    grow = rng.random(n) < 0.2
    stats0 = dict(grad_sum=torch.tensor(np.where(grow, 1.0, 0.0).astype(np.float32), device=dev), count=torch.ones(n, dtype=torch.int32, device=dev),
                  max_radius=torch.zeros(n, device=dev))
    mix = dict(grow_grad2d=0.5, grow_scale3d=float(np.median(sc.scales.max(axis=1))), scene_extent=1.0, prune_opacity=float(np.quantile(sc.opacities, 0.05)),
               split_factor=1.6, prune_scale_on=False)
    refine = dict(min_opacity=float(np.quantile(sc.opacities, 0.05)), cap_max=int(1.05 * n), grow_factor=1.05, seed=1)
    grads = {k: torch.randn(v.shape, device=dev) * 1e-3 for k, v in x.items()}
    times = (ctypes.c_float * 4)()

    def upload(r):
        r.upload(x["means"], x["opacities"], x["colors"], quats=x["quats"], scales=x["scales"], sh_degree=sc.sh_degree, group_id=gid, n_groups=G)

    def fresh(r):   # the scene with optimiser state, as a fit holds it
        upload(r)
        r.adam_step(grads, fit.DEFAULT_LRS, 1)
        return {k: v.clone() for k, v in stats0.items()}

    def laps(r):
        r._L.sas_scene_densify_times(r._ctx, times, 4)
        return list(times)

    rows = {arm: {k: [] for k in ("order", "upload", "off", "off_laps", "mix", "mix_laps", "mcmc", "mcmc_laps")} for arm in arms}
    perms, counts = {}, {}
    for k in range(rounds + 1):
        for arm, r in arms.items():   # the arms alternate inside every round
            got = {}
            got["order"] = events(lambda: r.storage_order(x["means"], gid))
            got["upload"] = wall(lambda: upload(r))[0]
            perms[arm] = r.read_order()
            stats = fresh(r)
            got["off"] = wall(lambda: r.densify(stats, **OFF))[0]
            got["off_laps"] = laps(r)
            stats = fresh(r)
            got["mix"], out = wall(lambda: r.densify(stats, **mix))
            got["mix_laps"] = laps(r)
            fresh(r)
            got["mcmc"], out2 = wall(lambda: r.mcmc_refine(**refine))
            got["mcmc_laps"] = laps(r)
            counts[arm] = (out["n"], out["cloned"], out["split"], out["pruned"], out2["n"], out2["relocated"], out2["added"])
            if k:   # (the first round warms allocators and clocks up)
                for key, v in got.items():
                    rows[arm][key].append(v)
    same = torch.equal(perms["host"], perms["device"]) and counts["host"] == counts["device"]
    med = lambda v: np.median(np.array(v), axis=0)
    h, d = rows["host"], rows["device"]
    c = counts["device"]
    say(f"== {n} Gaussians, SH degree {sc.sh_degree}, {G} groups; medians of {rounds} rounds, arms alternating; upload's permutations and all counts "
        f"{'identical' if same else 'DIFFER'} between the arms")
    say(f"   densify mix: N -> {c[0]} (cloned {c[1]}, split {c[2]}, pruned {c[3]}); mcmc_refine: N -> {c[4]} (relocated {c[5]}, added {c[6]})")
    say(f"   {'':44s} {'host arm':>10s} {'device arm':>11s}   host / device")
    host_sort = float(med(h["off_laps"])[2])
    order = float(med(d["order"]))
    say(f"   {'storage_order alone (device events)':44s} {'':>10s} {order:11.3f}   host sort lap {host_sort:.3f} ms = {host_sort / max(order, 1e-9):.1f} x "
        f"(asked: >= 10 x at 292 247)   [{min(d['order']):.3f}..{max(d['order']):.3f}]")
    for key, label in (("upload", "upload from device tensors (wall)"), ("off", "densify, every switch off (wall)"), ("mix", "densify, mix (wall)"),
                       ("mcmc", "mcmc_refine (wall)")):
        a, b = float(med(h[key])), float(med(d[key]))
        say(f"   {label:44s} {a:10.3f} {b:11.3f}   {a / max(b, 1e-9):6.2f} x   [{min(h[key]):.3f}..{max(h[key]):.3f}] [{min(d[key]):.3f}..{max(d[key]):.3f}]")
        if key != "upload":
            pa, pb = med(h[key + "_laps"]), med(d[key + "_laps"])
            say(f"   {'  laps: totals | rows | order | commit':44s} host {pa[0]:.3f} | {pa[1]:.3f} (+ read-back) | {pa[2]:.3f} (sort) | {pa[3]:.3f}    "
                f"device {pb[0]:.3f} | {pb[1]:.3f} (enqueue) | {pb[2]:.3f} (enqueue) | {pb[3]:.3f} (+ the kernels)")
    say()
    for r in arms.values():
        r.close()
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="20000,292247,1000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=float, default=0.0, help="milliseconds of idling in front of every timed blocking call: a fit calls densify once in "
                    "a hundred steps, the probe straight behind an upload whose freed buffers the driver is still taking back")
    ap.add_argument("--resources", action="store_true", help="append the kernels' registers, LDS and scratch")
    a = ap.parse_args()
    global SETTLE
    SETTLE = a.settle * 1e-3
    say(f"device: {torch.cuda.get_device_name(0)}; {a.settle:g} ms idle in front of every timed blocking call")
    r = Rasterizer(0)
    t0 = time.perf_counter()
    m = torch.randn(1 << 20, 3, device=r.device)
    while time.perf_counter() - t0 < 1.0:   # clocks up
        r.storage_order(m)
        torch.cuda.synchronize()
    r.close()
    ok = all([case(int(n), a.rounds) for n in a.sizes.split(",")])
    if a.resources:   # (compiles the library once more: on a box where that is cheap)
        say("kernel resources (tools/kernel_resources.py k_order):")
        say(subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_resources.py"), "k_order"], capture_output=True, text=True).stdout.rstrip())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
