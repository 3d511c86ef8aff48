"""The node driver on the device (deform.NodeDriver: sas_nodes_fit_rigid) beside the host's Kabsch fits it stands in for, and the yardstick
ratios of its kernel (profiles/node_fit.txt).

    python tools/node_fit_probe.py [--out FILE] [--gaussians 292247] [--nodes 64,256,1024,4096,16384] [--host-up-to 1024] [--rounds 5] [--steps 10]
                                   [--demo 60] [--resources [FILE]]

ONE process, one context.  First the kit's cases (tests/tools/node_fit_ref.py) at kn = 0, 1, 6 and 8: the largest |device - longdouble| /
yardstick per case and how many entries differ in bits from the float64 restatement.  Then per node count M (a seeded draw of M of the stand-in
scene's own means, the scene bound to them with k = 4; the moved positions are those of a parabolic bend plus a little noise):

  1. the kernel alone, device events around 20 launches back to back (they only enqueue), per launch, with ``steps`` = 1 and 32;
  2. ``NodeDriver.drive`` (the fit and the deform) from a device tensor: the host clock until it returns beside the device events of the span;
  3. the step "positions -> transforms -> deform -> 256 x 256 frame", wall clock with the frame waited for, with ``NodeDriver`` (positions on
     the device) against ``transforms_from_positions`` + ``deform`` (positions on the host), the arms alternating inside every round.  The host
     arm runs for M <= --host-up-to only.

One warm-up round; medians and [min..max] over the rounds.  Every GPU step runs under a time limit of its own (--limit seconds, a watchdog
thread that ends the process).  The condition printed at the end: at every M where both arms ran the device arm's step is not slower than the
host arm's by more than the arms' own run-to-run spread.  ``--demo N``: examples/demo_deform_cloth.py with N steps under both drivers, in
child processes, its two lines copied."""
import argparse
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
from deform_probe import bend, events, fmt, med  # noqa: E402
from node_opt_probe import limit, lines, say  # noqa: E402
from sim_a_splat_amd import deform  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, ring_camera  # noqa: E402

BURST = 20
BG = (0.0, 0.0, 0.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--gaussians", type=int, default=292247)
    ap.add_argument("--nodes", default="64,256,1024,4096,16384")
    ap.add_argument("--host-up-to", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per round of the step comparison")
    ap.add_argument("--demo", type=int, default=0, help="steps of examples/demo_deform_cloth.py under both drivers (0: not run)")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single GPU step may take")
    ap.add_argument("--resources", nargs="?", const="", default=None, metavar="FILE",
                    help="append the kernels' registers, LDS and occupancy: compiles the library once more, or reads FILE, the output of "
                         "`python tools/kernel_resources.py k_nodes` made beforehand (the probe's GPU time then goes to the GPU)")
    a = ap.parse_args()
    W = H = 256
    sc = make_scene(a.gaussians, seed=2, log_scale_mean=float(np.log(0.01)))
    n = sc.means.shape[0]
    cam = ring_camera(W, H, 256.0, yaw_deg=0.0)
    V, K = cam.viewmat.astype(np.float32), cam.K.astype(np.float32)
    with limit(a.limit, "the context and the upload"):
        r = Rasterizer(0)
        r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, sh_degree=sc.sh_degree)
        t0 = time.perf_counter()
        warm = torch.randn(1 << 18, 3, device=r.device)
        while time.perf_counter() - t0 < 1.0:   # clocks up
            r.knn_nodes(warm, warm[:256], 4)
            torch.cuda.synchronize()
    say(f"device: {torch.cuda.get_device_name(0)}; {n} Gaussians, SH degree {sc.sh_degree}; one {W} x {H} view; medians of {a.rounds} rounds [min..max], ms; "
        f"arms alternating; one warm-up round.  Every figure below is of this GPU run; the host arm's fits run on this machine's CPU.")
    import node_fit_child as nfc
    import node_fit_ref as nf
    say("-- the kit's cases: largest |device - fit_ref(longdouble)| / yardstick (held to 4), entries that differ in bits from fit_ref(float64)")
    with limit(a.limit, "the kit's cases"):
        for name in nf.CASES:
            res = [nfc.check_case(r, name, kn, say=lambda s: None) for kn in nf.KNS]
            say(f"   {name:12s} " + "   ".join(f"kn={kn}: {x['ratio']:.3f}, {x['differ']}/{x['entries']}" for kn, x in zip(nf.KNS, res)) +
                f"   (yardstick up to {max(x['yardstick'] for x in res):.2e})")
    extent = float(np.ptp(sc.means[:, 0]))
    verdicts = []
    for m in (int(s) for s in a.nodes.split(",")):
        rng = np.random.default_rng(7)
        nodes = np.ascontiguousarray(sc.means[rng.choice(n, m, replace=False)])
        G = bend(nodes, 0.05 * extent).astype(np.float64)
        moved = (np.einsum("mab,mb->ma", G[:, :, :3], nodes.astype(np.float64)) + G[:, :, 3] + rng.normal(0.0, 1e-3 * extent, (m, 3))).astype(np.float32)
        with limit(a.limit, f"m = {m}: binding"):
            r.bind_skin(nodes, k=4)
            t0 = time.perf_counter()
            driver = deform.NodeDriver(r, nodes)
            torch.cuda.synchronize()
            setup = (time.perf_counter() - t0) * 1e3
        say(f"-- m = {m} nodes, {driver.k} neighbours each; NodeDriver set-up (knn_points; wall) {setup:.2f} ms")
        moved_dev = torch.from_numpy(moved).to(r.device)
        many = moved_dev[None].repeat(32, 1, 1).contiguous()
        out1 = (torch.empty((m, 3, 4), device=r.device), torch.empty((m, 3, 4), dtype=torch.float64, device=r.device))
        out32 = (torch.empty((32, m, 3, 4), device=r.device), torch.empty((32, m, 3, 4), dtype=torch.float64, device=r.device))
        t = {1: [], 32: [], "host": [], "dev": []}
        with limit(a.limit, f"m = {m}: the kernel alone and drive"):
            for k in range(a.rounds + 1):
                for steps, b, o in ((1, moved_dev, out1), (32, many, out32)):
                    ms, _ = events(lambda: [r.node_fit_rigid(driver.nodes, b, driver.table, out=o[0], out64=o[1]) for _ in range(BURST)])
                    if k:
                        t[steps].append(ms / BURST)
                x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                x.record()
                t0 = time.perf_counter()
                for _ in range(BURST):
                    driver.drive(moved_dev)
                host = (time.perf_counter() - t0) * 1e3
                y.record()
                torch.cuda.synchronize()
                if k:
                    t["host"].append(host / BURST)
                    t["dev"].append(x.elapsed_time(y) / BURST)
        say(f"   1. sas_nodes_fit_rigid alone (events, per launch of {BURST}), steps = 1    {fmt(t[1])}")
        say(f"                                                             steps = 32   {fmt(t[32])}")
        say(f"   2. NodeDriver.drive (fit + deform), {BURST} in a row, per call: host clock until it returned   {fmt(t['host'])}")
        say(f"                                                              device events around the span  {fmt(t['dev'])}")
        arms = ["device"] + (["host"] if m <= a.host_up_to else [])
        per = {arm: [] for arm in arms}
        for k in range(a.rounds + 1):
            for arm in arms:   # the arms alternate inside every round
                with limit(a.limit, f"m = {m}: the step, {arm} arm"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s in range(a.steps):
                        if arm == "device":
                            driver.drive(moved_dev)
                        else:
                            r.deform(deform.transforms_from_positions(nodes, moved))
                        r.render(V, K, W, H, BG, want=("rgb8",))
                        torch.cuda.synchronize()
                    if k:
                        per[arm].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for arm in arms:
            say(f"   3. step positions -> transforms -> deform -> {W} x {H} frame, {arm:6s} arm (wall, frame waited for)   {fmt(per[arm])}")
        if "host" in per:
            d, h = med(per["device"]), med(per["host"])
            spread = max(d[2] - d[1], h[2] - h[1])
            ok = d[0] <= h[0] + spread
            verdicts.append((m, ok))
            say(f"      host / device = {h[0] / d[0]:.2f}; the arms' run-to-run spread is {spread:.3f} ms: the device arm is {'NOT SLOWER' if ok else 'SLOWER'} than the host arm")
        else:
            say(f"      (no host arm beyond m = {a.host_up_to}: its table is {m * m * 24 / 1e9:.2f} GB of float64 per call)")
        r.clear_skin()
    say()
    if verdicts:
        say("the condition (device arm not slower than the host arm beyond the run-to-run spread, wherever both ran): " +
            ", ".join(f"m = {m}: {'holds' if ok else 'FAILS'}" for m, ok in verdicts))
    with limit(a.limit, "closing"):
        r.close()
    if a.demo:
        say(f"examples/demo_deform_cloth.py --steps {a.demo}, both drivers (a child process each):")
        for arm in ("host", "device"):
            p = subprocess.run([sys.executable, str(ROOT / "examples" / "demo_deform_cloth.py"), "--steps", str(a.demo), "--driver", arm], capture_output=True,
                               text=True, timeout=a.limit)
            say("\n".join("   " + ln for ln in p.stdout.strip().split("\n")[-2:]))
            if p.returncode != 0:
                say(f"   the {arm} arm ended with status {p.returncode}: {p.stderr[-500:]}")
                verdicts.append((f"demo {arm}", False))
                break
    if a.resources is not None:
        say("kernel resources (tools/kernel_resources.py k_nodes; a cross-compile for gfx950, which needs no GPU):")
        say(Path(a.resources).read_text().rstrip() if a.resources else
            subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_resources.py"), "k_nodes"], capture_output=True, text=True).stdout.rstrip())
    if a.out:   # (the file's "# Reading it" part is written by hand, behind what this wrote)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if all(ok for _, ok in verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
