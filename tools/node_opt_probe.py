"""The node optimiser on the device (deform.NodeOptimizer: sas_nodes_rigidity, sas_nodes_twist_step) beside the host optimiser it stands in
for (profiles/node_opt.txt).

    python tools/node_opt_probe.py [--out FILE] [--gaussians 292247] [--nodes 64,256,1024,4096,16384] [--host-up-to 1024] [--iters 12] [--rounds 5]
                                   [--resources]

ONE process, one context; per node count M (a seeded draw of M of the stand-in scene's own means, the scene bound to them with k = 4, bent by
a parabola, four 256 x 256 views of the bent scene as targets):

  1. each kernel alone, device events around 20 launches back to back (they only enqueue), per launch;
  2. a whole ``fit_node_transforms`` iteration at full size (``factors=(1,)``): the wall clock of the call over its ``iters + 1`` evaluations,
     set-up and final read-back included, with ``optimizer="device"`` against ``optimizer="host"``, the arms alternating inside every round.  The
     host arm runs for M <= --host-up-to only: its [M,M,3] float64 table per iteration is why the device arm exists;
  3. for the device arm, the loop restated from its public pieces (deform, render, prechain, render_backward, deform_backward, NodeOptimizer.step):
     the host clock until the LAST enqueue returns beside the device-event time of the same span -- a loop that only enqueues returns long before
     the device is done; one that waits somewhere returns with it.  Beside it the optimiser's own share, ``NodeOptimizer.step`` 200 times in a
     row (no frames between them), by the same two clocks: which of the loop's calls wait is read from the two lines together.

One warm-up round; medians and [min..max] over the rounds.  Every GPU step runs under a time limit of its own (--limit seconds, a watchdog
thread that ends the process): a probe that hangs must not keep the device.  The condition printed at the end: at every M where both arms ran
the device arm's iteration is not slower than the host arm's by more than the arms' own run-to-run spread."""
import argparse
import os
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from deform_probe import bend, events, fmt, med  # noqa: E402
from sim_a_splat_amd import deform  # noqa: E402
from sim_a_splat_amd.autograd import prechain  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

lines = []
BURST = 20
BG = (0.0, 0.0, 0.0)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


class limit:
    """``with limit(seconds, what):`` -- the process ends (status 124) when the block runs longer: nothing more is started on the GPU."""

    def __init__(self, seconds, what):
        self.timer = threading.Timer(seconds, self.expire)
        self.what, self.seconds = what, seconds

    def expire(self):
        print(f"node_opt_probe: {self.what} ran longer than {self.seconds} s: ending", flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def kernels_alone(r, opt, rounds):
    d32 = torch.randn((opt.m, 3, 4), device=r.device) * 1e-3
    t = {"rigidity": [], "twist_step": []}
    out = torch.empty((opt.m, 3, 4), dtype=torch.float64, device=r.device)
    for k in range(rounds + 1):
        ms, _ = events(lambda: [r.node_rigidity(opt.nodes, opt.transforms64, opt.table, opt.rev_start, opt.rev_edge, out=out) for _ in range(BURST)])
        if k:
            t["rigidity"].append(ms / BURST)
        ms, _ = events(lambda: [r.node_twist_step(opt.nodes, opt.transforms64, opt.m1, opt.m2, opt.transforms, d32, out, 0.01, lr=(1e-4, 1e-4),
                                                  c1=1 - 0.9 ** (j + 1), c2=1 - 0.999 ** (j + 1)) for j in range(BURST)])
        if k:
            t["twist_step"].append(ms / BURST)
    return t


def steps_alone(r, opt, count=200):
    """``NodeOptimizer.step`` ``count`` times with nothing between: (host ms until the last enqueue returned, device ms of the span), per step."""
    d32 = torch.randn((opt.m, 3, 4), device=r.device) * 1e-3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for it in range(count):
        opt.step(d32, it, count)
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    torch.cuda.synchronize()
    return host / count, a.elapsed_time(b) / count


def restated_loop(r, opt, images, V, K, W, H, iters):
    """``fit_node_transforms(optimizer="device")``'s loop from its public pieces: (host ms until the last enqueue returned, device ms of the span)."""
    C = len(V)
    targets = [torch.from_numpy(images[v]).to(r.device) for v in range(C)]
    scale = 1.0 / (3.0 * W * H * C)
    acc = {}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for it in range(iters):
        r.deform(opt.transforms)
        for x in acc.values():
            x.zero_()
        for v in range(C):
            out = r.render(V[v], K[v], W, H, BG)
            rgb, alpha, depth = out["rgb"].clone(), out["alpha"].clone(), out["depth"].clone()
            g_acc, g_a, g_z = prechain(rgb, alpha, depth, BG, 2.0 * scale * (rgb - targets[v]), None, None)
            acc.update(r.render_backward(V[v], K[v], W, H, g_acc, g_a, g_z, want=("means", "quats"), out=acc))
        opt.step(r.deform_backward(acc), it, iters)
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    torch.cuda.synchronize()
    return host / iters, a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--gaussians", type=int, default=292247)
    ap.add_argument("--nodes", default="64,256,1024,4096,16384")
    ap.add_argument("--host-up-to", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single GPU step may take")
    ap.add_argument("--resources", action="store_true", help="append the kernels' registers, LDS and occupancy (compiles the library once more)")
    a = ap.parse_args()
    W = H = 256
    sc = make_scene(a.gaussians, seed=2, log_scale_mean=float(np.log(0.01)))
    n = sc.means.shape[0]
    cams = [ring_camera(W, H, 256.0, yaw_deg=90.0 * k) for k in range(4)]
    V, K = [c.viewmat.astype(np.float32) for c in cams], [c.K.astype(np.float32) for c in cams]
    with limit(a.limit, "the context and the upload"):
        r = Rasterizer(0)
        r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
        t0 = time.perf_counter()
        warm = torch.randn(1 << 18, 3, device=r.device)
        while time.perf_counter() - t0 < 1.0:   # clocks up
            r.knn_nodes(warm, warm[:256], 4)
            torch.cuda.synchronize()
    say(f"device: {torch.cuda.get_device_name(0)}; {n} Gaussians, SH degree {sc.sh_degree}; four {W} x {H} views; medians of {a.rounds} rounds [min..max], ms; "
        f"arms alternating; one warm-up round")
    extent = float(np.ptp(sc.means[:, 0]))
    verdicts = []
    for m in (int(s) for s in a.nodes.split(",")):
        nodes = np.ascontiguousarray(sc.means[np.random.default_rng(7).choice(n, m, replace=False)])
        with limit(a.limit, f"m = {m}: binding and the targets"):
            r.bind_skin(nodes, k=4)
            r.deform(torch.from_numpy(bend(nodes, 0.05 * extent)).to(r.device))
            images = np.stack([r.render(V[v], K[v], W, H, BG)["rgb"].clone().cpu().numpy() for v in range(4)])
            t0 = time.perf_counter()
            opt = deform.NodeOptimizer(r, nodes)
            torch.cuda.synchronize()
            setup = (time.perf_counter() - t0) * 1e3
        say(f"-- m = {m} nodes, {opt.k} neighbours each; NodeOptimizer set-up (knn_points, one read-back, the reverse table; wall) {setup:.2f} ms")
        with limit(a.limit, f"m = {m}: the kernels alone"):
            t = kernels_alone(r, opt, a.rounds)
        say(f"   1. sas_nodes_rigidity alone (events, per launch of {BURST})      {fmt(t['rigidity'])}")
        say(f"      sas_nodes_twist_step alone (events, per launch of {BURST})    {fmt(t['twist_step'])}")
        arms = ["device"] + (["host"] if m <= a.host_up_to else [])
        per = {arm: [] for arm in arms}
        ends = {}
        for k in range(a.rounds + 1):
            for arm in arms:   # the arms alternate inside every round
                with limit(a.limit, f"m = {m}: fit_node_transforms, optimizer={arm}"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = deform.fit_node_transforms(r, images, np.stack(V), np.stack(K), W, H, nodes, iters=a.iters, factors=(1,), optimizer=arm)
                    torch.cuda.synchronize()
                    if k:
                        per[arm].append((time.perf_counter() - t0) * 1e3 / (a.iters + 1))
                    ends[arm] = (res.history[0][1], res.loss)
        for arm in arms:
            say(f"   2. fit_node_transforms iteration, optimizer={arm:6s} (wall / {a.iters + 1} evaluations)   {fmt(per[arm])}   loss {ends[arm][0]:.4e} -> {ends[arm][1]:.4e}")
        if "host" in per:
            d, h = med(per["device"]), med(per["host"])
            spread = max(d[2] - d[1], h[2] - h[1])
            ok = d[0] <= h[0] + spread
            verdicts.append((m, ok))
            say(f"      host / device = {h[0] / d[0]:.2f}; the arms' run-to-run spread is {spread:.3f} ms: the device arm is {'NOT SLOWER' if ok else 'SLOWER'} than the host arm")
        else:
            say(f"      (no host arm beyond m = {a.host_up_to}: its table is {m * m * 24 / 1e9:.2f} GB of float64 per iteration)")
        spans, alone = [], []
        for k in range(a.rounds + 1):
            with limit(a.limit, f"m = {m}: the restated loop"):
                opt.set_transforms(np.tile(np.eye(3, 4), (m, 1, 1)))
                opt.reset_moments()
                span = restated_loop(r, opt, images, V, K, W, H, a.iters)
                own = steps_alone(r, opt)
                if k:
                    spans.append(span)
                    alone.append(own)
        host_ms, dev_ms = [s[0] for s in spans], [s[1] for s in spans]
        say(f"   3. the device arm's loop restated, per iteration: host clock until the last enqueue returned   {fmt(host_ms)}")
        say(f"                                                     device events around the same span            {fmt(dev_ms)}   host / device = {med(host_ms)[0] / med(dev_ms)[0]:.2f}")
        say(f"      NodeOptimizer.step alone, 200 in a row, per step:  host clock until the last enqueue returned   {fmt([s[0] for s in alone])}")
        say(f"                                                         device events around the same span            {fmt([s[1] for s in alone])}")
        r.clear_skin()
    say()
    if verdicts:
        say("the condition (device arm not slower than the host arm beyond the run-to-run spread, wherever both ran): " +
            ", ".join(f"m = {m}: {'holds' if ok else 'FAILS'}" for m, ok in verdicts))
    with limit(a.limit, "closing"):
        r.close()
    if a.resources:
        say("kernel resources (tools/kernel_resources.py k_nodes):")
        say(subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_resources.py"), "k_nodes"], capture_output=True, text=True).stdout.rstrip())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if all(ok for _, ok in verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
