"""The adjoint of the deformation to the rest arrays (Rasterizer.deform_backward_rest) and Adam under a skin (adam_step(rest=True)) beside
their neighbours (profiles/deform_rest.txt).

    python tools/deform_rest_probe.py [--out FILE] [--sizes 292247,1000000] [--nodes 64,256,1024,4096,16384] [--ks 4,8] [--rounds 5] [--resources]
    python tools/deform_rest_probe.py --no-timing --resources --out FILE       the resources alone, appended to FILE (no GPU needed)

ONE process, two contexts on one box: a skinned one, and an unskinned one for the plain adam_step.  The rounds alternate the arms; one warm-up
round; medians and [min..max] over the rounds; device events around what only enqueues (deform, deform_backward, deform_backward_rest,
adam_step), the wall clock around what blocks (the torch arm with its synchronisation, render, render_backward, a fit iteration).  Per scene --
the 292 247-Gaussian stand-in and config 3's million -- and per (m, k):

  deform_backward_rest beside deform and deform_backward of the same run, as bytes per microsecond of the traffic each must move per slot:
      deform               48 B of rest planes + 8 kp B of skin planes read, 48 B written
      deform_backward_rest 8 kp B of skin planes + 28 B of gradients read, 28 B of outputs read and written again (84 B; no rest plane)
      deform_backward      48 + 8 kp + 28 B read (its atomics are not counted: profiles/deform_grad.txt has them)
    (kp = 4 or 8 entries; the node records, m * 64 B per workgroup or per lane from cache, are not counted on either side)
  deform_backward_rest beside the same adjoint as torch autograd ops on device tensors
  adam_step(rest=True) beside an unskinned adam_step plus one deform
  a whole fit_dynamic_scene iteration (2 time steps, 2 views of 256 x 256 each, means and colours), with its parts

The nodes are a seeded draw of m of the scene's own means; the upstream gradients are normal draws."""
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
from deform_probe import bend, events, fmt, med, torch_deform, wall  # noqa: E402
from sim_a_splat_amd import deform  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import config_cameras, config_scene_and_cameras, make_scene  # noqa: E402

lines = []
LRS = dict(means=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, quats=1e-3)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def case(n, node_counts, ks, rounds, A, B, fit_at):
    sc = config_scene_and_cameras(3)[0] if n == 1_000_000 else make_scene(n, seed=2, log_scale_mean=float(np.log(0.01)))
    n = sc.means.shape[0]
    dev = A.device
    x = {k: torch.tensor(v, device=dev) for k, v in dict(means=sc.means, opacities=sc.opacities, colors=sc.sh, quats=sc.quats, scales=sc.scales).items()}
    extent = float(np.ptp(sc.means[:, 0]))
    cam = config_cameras(1)[0]
    for r in (A, B):
        r.upload(x["means"], x["opacities"], x["colors"], quats=x["quats"], scales=x["scales"], sh_degree=sc.sh_degree)
    gen = torch.Generator(device=dev).manual_seed(11)
    up = {"means": torch.randn((n, 3), device=dev, generator=gen), "quats": torch.randn((n, 4), device=dev, generator=gen)}
    step_grads = dict(up, colors=torch.randn(tuple(x["colors"].shape), device=dev, generator=gen) * 1e-3)
    say(f"== {n} Gaussians, SH degree {sc.sh_degree}; medians of {rounds} rounds [min..max], ms; arms alternating")
    worst = 0.0
    for m in node_counts:
        nodes = np.ascontiguousarray(sc.means[np.random.default_rng(7).choice(n, m, replace=False)])
        G = torch.from_numpy(bend(nodes, 0.05 * extent)).to(dev)
        for kk in ks:
            kp = 4 if kk <= 4 else 8
            bound = A.bind_skin(nodes, k=kk)
            A.deform(G)
            idx, w = bound["indices"], bound["weights"]
            names = ("deform", "deform_backward", "deform_backward_rest", "adam_step(rest=True)", "adam_step, unskinned")
            t = {a: [] for a in names}
            t_torch = []
            out = {k: torch.zeros_like(v) for k, v in up.items()}

            def torch_adjoint():
                P = {k: x[k].clone().requires_grad_(True) for k in ("means", "quats")}
                means, quats = torch_deform(dict(x, **P), idx, w, G)
                ((means * up["means"]).sum() + (quats * up["quats"]).sum()).backward()
                return P["means"].grad, P["quats"].grad

            step = 0
            for k in range(rounds + 1):
                step += 1
                for a, fn in (("deform", lambda: A.deform(G)), ("deform_backward", lambda: A.deform_backward(up)),
                              ("deform_backward_rest", lambda: A.deform_backward_rest(up, out=out)),
                              ("adam_step(rest=True)", lambda: A.adam_step(step_grads, LRS, step, rest=True)),
                              ("adam_step, unskinned", lambda: B.adam_step(step_grads, LRS, step))):
                    ms, _ = events(fn)
                    if k:
                        t[a].append(ms)
                ms, ref = wall(torch_adjoint)
                if k:
                    t_torch.append(ms)
            got = A.deform_backward_rest(up)
            # torch's arm normalises the blended quaternion through another expression; both are the same function on the probe's bends
            diff = max(float((got[k] - g).abs().max()) / float(g.abs().max()) for k, g in zip(("means", "quats"), ref))
            worst = max(worst, diff)
            say(f"-- m = {m} nodes, k = {kk}: deform_backward_rest differs from torch autograd's by up to {diff:.1e} of the largest entry")
            nbytes = {"deform": 96 + 8 * kp, "deform_backward": 76 + 8 * kp, "deform_backward_rest": 84 + 8 * kp}
            rate = {}
            for a in ("deform", "deform_backward", "deform_backward_rest"):
                rate[a] = n * nbytes[a] / (med(t[a])[0] * 1e3)
                say(f"   {a:24s} (events)   {fmt(t[a])}   {n * nbytes[a] / 1e6:8.2f} MB = {rate[a]:10.0f} bytes per microsecond")
            say(f"   {'':24s}            deform_backward_rest moves its bytes at {rate['deform_backward_rest'] / rate['deform']:.2f} of deform's rate")
            b = med(t["deform_backward_rest"])[0]
            say(f"   the same adjoint as torch autograd ops (wall)  {fmt(t_torch)}   {med(t_torch)[0] / b:8.1f} x deform_backward_rest")
            both = [u + d for u, d in zip(t["adam_step, unskinned"], t["deform"])]
            say(f"   adam_step(rest=True)     (events)   {fmt(t['adam_step(rest=True)'])}")
            say(f"   adam_step, unskinned     (events)   {fmt(t['adam_step, unskinned'])}   + one deform = {fmt(both)}   rest=True is "
                f"{med(t['adam_step(rest=True)'])[0] / med(both)[0]:.2f} of the two")
            if (m, kk) == fit_at:
                fit_iteration(A, nodes, G, torch.from_numpy(bend(nodes, -0.05 * extent)), cam, rounds)
            A.clear_skin()
            A.adam_reset()
            B.adam_reset()
    say()
    return worst


def fit_iteration(A, nodes, G, G2, cam, rounds):
    """A whole fit_dynamic_scene iteration on the bound skin -- 2 time steps (the bend and its mirror image), 2 views each -- and its parts."""
    cams = (list(config_cameras(1)) * 2)[:2]
    V = np.stack([np.asarray(c.viewmat, np.float32) for c in cams])
    K = np.stack([np.asarray(c.K, np.float32) for c in cams])
    Wd, Hd = cam.width, cam.height
    T = np.stack([G.cpu().numpy(), G2.cpu().numpy()]).astype(np.float64)
    frames = []
    for t in range(2):
        A.deform(np.ascontiguousarray(T[t].astype(np.float32)))
        frames.append(dict(images=np.stack([A.render(V[v], K[v], Wd, Hd, (0.0, 0.0, 0.0))["rgb"].cpu().numpy() for v in range(2)]), viewmats=V, Ks=K))
    # a call drops the optimiser state and its first step allocates it anew: the iteration's own time is the slope between two lengths of run
    short, long_ = 2, 10
    tw = []
    for k in range(rounds + 1):
        ms = [wall(lambda: deform.fit_dynamic_scene(A, frames, nodes, what=("means", "colors"), transforms=T, iters=it, extent=1.0))[0] for it in (short, long_)]
        if k:
            tw.append((ms[1] - ms[0]) / (long_ - short))
    g_rgb = torch.randn((Hd, Wd, 3), device=A.device)
    parts = {"render": [], "render_backward": [], "deform": [], "deform_backward_rest": [], "adam_step(rest=True)": []}
    acc = None
    for k in range(rounds + 1):
        ms_d, _ = events(lambda: A.deform(G))
        ms_r, _ = wall(lambda: A.render(V[0], K[0], Wd, Hd, (0.0, 0.0, 0.0)))
        ms_b, acc = wall(lambda: A.render_backward(V[0], K[0], Wd, Hd, g_rgb=g_rgb, want=("means", "colors")))
        ms_a, rest = events(lambda: A.deform_backward_rest({"means": acc["means"]}))
        ms_s, _ = events(lambda: A.adam_step(dict(rest, colors=acc["colors"]), LRS, k + 1, rest=True))
        if k:
            for name, ms in zip(parts, (ms_r, ms_b, ms_d, ms_a, ms_s)):
                parts[name].append(ms)
    say(f"   a fit_dynamic_scene iteration, 2 time steps x 2 views of {Wd} x {Hd}, means and colours (wall; (a run of {long_} - a run of {short}) / {long_ - short})   {fmt(tw)}")
    for name, v in parts.items():
        per = 4 if name.startswith("render") else 2 if name.startswith("deform") else 1
        say(f"      {name:24s} {fmt(v)}   x {per} per iteration = {per * med(v)[0]:8.3f}")
    say(f"      the rest of the iteration is the loss in torch, prechain and the host loop")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="292247,1000000")
    ap.add_argument("--nodes", default="64,256,1024,4096,16384")
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resources", action="store_true", help="append the kernels' registers, LDS and occupancy (compiles the library once more)")
    ap.add_argument("--no-timing", action="store_true", help="measure nothing (no GPU needed): with --resources and --out, append them to FILE as it stands")
    a = ap.parse_args()
    if a.no_timing:
        lines.extend(Path(a.out).read_text().rstrip("\n").split("\n") if a.out and Path(a.out).exists() else [])
        return finish(a, 0.0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    A, B = Rasterizer(0), Rasterizer(0)
    t0 = time.perf_counter()
    warm = torch.randn(1 << 18, 3, device=A.device)
    while time.perf_counter() - t0 < 1.0:   # clocks up
        A.knn_nodes(warm, warm[:256], 4)
        torch.cuda.synchronize()
    worst = 0.0
    node_counts, ks = [int(s) for s in a.nodes.split(",")], [int(s) for s in a.ks.split(",")]
    for n in (int(s) for s in a.sizes.split(",")):
        worst = max(worst, case(n, node_counts, ks, a.rounds, A, B, (node_counts[min(1, len(node_counts) - 1)], ks[0])))
    A.close()
    B.close()
    return finish(a, worst)


def finish(a, worst):
    if a.resources:
        for filt in ("k_deform_rest_grad", "k_deform<"):
            say(f"kernel resources (tools/kernel_resources.py '{filt}'): VGPRs, LDS bytes, waves per SIMD (occ)")
            say(subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_resources.py"), filt], capture_output=True, text=True).stdout.rstrip())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if worst < 1e-3 else 1


if __name__ == "__main__":
    sys.exit(main())
