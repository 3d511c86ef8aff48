"""The adjoint of the deformation (Rasterizer.deform_backward) beside the only way there was before it -- the same adjoint as torch autograd
ops on device tensors -- and beside render_backward of one 256 x 256 view of the same scene (profiles/deform_grad.txt).

    python tools/deform_grad_probe.py [--out FILE] [--sizes 292247,1000000] [--nodes 64,256,1024,2048,16384] [--ks 4,8] [--rounds 5] [--resources]

ONE process, five contexts on one box -- the default one, and one per form of k_deform_grad: the per-node sums in LDS (SAS_SKIN_GRAD_LDS at its ceiling, so that the
budget's default can be judged from both sides) or in global memory (SAS_SKIN_GRAD_LDS=0), the rows added by the lane that made them
(SAS_SKIN_GRAD_STAGED=0) or staged through LDS and added 16 lanes per row (=1).  The rounds alternate the arms; one warm-up round; medians and
[min..max] over the rounds; device events around deform_backward (it only enqueues), the wall clock around what blocks (render_backward, the torch
arm with its synchronisation).  Per scene -- the 292 247-Gaussian stand-in and config 3's million -- and per (m, k).

Atomic bytes: the global arms add one 64-B row per live entry (N k rows; 48 B of a row are touched when no orientation gradient is given, never
here); the LDS arms add blocks * m * 64 B in their flush at most (zeros are not sent).  The rate is set beside the chip-wide float-atomic rate
of about 1.3 TB/s.

The nodes are a seeded draw of m of the scene's own means; the upstream gradients are normal draws.  The four arms' results are compared with
each other (float sums in different orders: the largest relative difference is printed) and, in their translation columns, with torch's."""
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
sys.path.insert(0, str(ROOT / "tools"))
from deform_probe import bend, events, fmt, med, torch_deform, wall  # noqa: E402
from sim_a_splat_amd import _capi  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import config_cameras, config_scene_and_cameras, make_scene  # noqa: E402

lines = []
LDS_MAX = 131072   # SAS_SKIN_GRAD_LDS_MAX (csrc/sas_internal.h)
STAGED_LDS = 16384   # SAS_SKIN_GRAD_STAGED_LDS_BYTES
ARMS = {"LDS, own rows": (LDS_MAX, 0), "LDS, staged": (LDS_MAX, 1), "global, own rows": (0, 0), "global, staged": (0, 1), "the default": None}
ATOMIC_RATE = 1.3e12


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def context(setting):
    old = {k: os.environ.pop(k, None) for k in ("SAS_SKIN_GRAD_LDS", "SAS_SKIN_GRAD_STAGED")}
    if setting is not None:
        os.environ.update(SAS_SKIN_GRAD_LDS=str(setting[0]), SAS_SKIN_GRAD_STAGED=str(setting[1]))
    try:
        return Rasterizer(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def blocks_of(n, m, lds, staged, cus):
    """The persistent grid's workgroups, as sas_scene_deform_backward sizes it."""
    use = (17408 if staged else 0) + (64 * m if lds else 0)
    per_cu = max(1, min(4, (160 * 1024) // use if use else 4))
    return max(1, min((n + 255) // 256, per_cu * cus))


def case(n, node_counts, ks, rounds, arms):
    sc = config_scene_and_cameras(3)[0] if n == 1_000_000 else make_scene(n, seed=2, log_scale_mean=float(np.log(0.01)))
    n = sc.means.shape[0]
    first = next(iter(arms.values()))
    dev = first.device
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    x = {k: torch.tensor(v, device=dev) for k, v in dict(means=sc.means, opacities=sc.opacities, colors=sc.sh, quats=sc.quats, scales=sc.scales).items()}
    extent = float(np.ptp(sc.means[:, 0]))
    cam = config_cameras(1)[0]
    for r in arms.values():
        r.upload(x["means"], x["opacities"], x["colors"], quats=x["quats"], scales=x["scales"], sh_degree=sc.sh_degree)
    gen = torch.Generator(device=dev).manual_seed(11)
    up = {"means": torch.randn((n, 3), device=dev, generator=gen), "quats": torch.randn((n, 4), device=dev, generator=gen)}
    g_rgb = torch.randn((cam.height, cam.width, 3), device=dev, generator=gen)
    say(f"== {n} Gaussians, SH degree {sc.sh_degree}; {cus} CUs; medians of {rounds} rounds [min..max], ms; arms alternating")
    worst = 0.0
    for m in node_counts:
        nodes = np.ascontiguousarray(sc.means[np.random.default_rng(7).choice(n, m, replace=False)])
        G = torch.from_numpy(bend(nodes, 0.05 * extent)).to(dev)
        for kk in ks:
            bound = None
            for r in arms.values():
                bound = r.bind_skin(nodes, k=kk)
                r.deform(G)
            idx, w = bound["indices"], bound["weights"]
            live = int(((idx >= 0) & (w > 0)).sum())
            t = {a: [] for a in arms}
            t_torch, t_back = [], []
            got = {}

            def torch_adjoint():
                Gv = G.clone().requires_grad_(True)
                means, quats = torch_deform(x, idx, w, Gv)
                ((means * up["means"]).sum() + (quats * up["quats"]).sum()).backward()
                return Gv.grad

            for k in range(rounds + 1):
                for arm, r in arms.items():   # the arms alternate inside every round
                    ms, out = events(lambda: r.deform_backward(up))
                    got[arm] = out
                    if k:
                        t[arm].append(ms)
                ms, ref = wall(torch_adjoint)
                if k:
                    t_torch.append(ms)
                ms, _ = wall(lambda: first.render_backward(cam.viewmat, cam.K, cam.width, cam.height, g_rgb=g_rgb, want=("means", "quats")))
                if k:
                    t_back.append(ms)
            top = float(ref.abs().max())
            diff = max(float((got[a] - got[b]).abs().max()) for a in got for b in got) / top
            # torch's arm turns R into a quaternion by the trace formula, another extension off the rotations than k_skin_nodes' u / |u|: its dR
            # differs from the kernels' by that, legitimately.  The translation columns are the same function.
            vs_torch = max(float((got[a][:, :, 3] - ref[:, :, 3]).abs().max()) for a in got) / float(ref[:, :, 3].abs().max())
            worst = max(worst, diff)
            say(f"-- m = {m} nodes, k = {kk}: {live} live entries = {live * 64 / 1e6:.1f} MB of rows; the arms differ by up to {diff:.1e} of the largest entry, "
                f"their dt columns from torch autograd's by up to {vs_torch:.1e} of the largest")
            best = min((a for a in arms if ARMS[a] is not None), key=lambda a: med(t[a])[0])
            for arm, setting in ARMS.items():
                if setting is None:   # what sas_scene_deform_backward chooses by itself
                    lds = LDS_MAX
                    staged = int(64 * m > LDS_MAX or 64 * m <= STAGED_LDS)
                    arm = f"{arm}: {'LDS' if 64 * m <= LDS_MAX else 'global'}, {'staged' if staged else 'own rows'}"
                    t[arm] = t["the default"]
                else:
                    lds, staged = setting
                in_lds = lds and 64 * m <= lds
                if lds and not in_lds and setting is not None:
                    say(f"   deform_backward, {arm:32s} (events)      (m * 64 B is beyond the LDS ceiling: this arm took the global path)   {fmt(t[arm])}")
                    continue
                blocks = blocks_of(n, m, in_lds, staged, cus)
                nbytes = min(blocks * m, live) * 64 if in_lds else live * 64
                rate = nbytes / (med(t[arm])[0] * 1e-3)
                say(f"   deform_backward, {arm:32s} (events)   {fmt(t[arm])}   {blocks:5d} workgroups; atomics to memory {nbytes / 1e6:8.2f} MB "
                    f"{'at most ' if in_lds else ''}= {rate / 1e9:7.1f} GB/s = {rate / ATOMIC_RATE:.3f} of 1.3 TB/s{'   <- fastest' if arm == best else ''}")
            b = med(t[best])[0]
            say(f"   the same adjoint as torch autograd ops (wall)       {fmt(t_torch)}   {med(t_torch)[0] / b:8.1f} x the fastest arm")
            say(f"   render_backward, one 256 x 256 view (wall)          {fmt(t_back)}   the fastest arm is {b / med(t_back)[0]:.3f} of it")
        for r in arms.values():
            r.clear_skin()
    say()
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="292247,1000000")
    ap.add_argument("--nodes", default="64,256,1024,2048,16384")
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resources", action="store_true", help="append the kernels' registers, LDS and occupancy (compiles the library once more)")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}; the LDS budget's default is {_capi.SAS_SKIN_GRAD_LDS_BYTES} B = {_capi.SAS_SKIN_GRAD_LDS_BYTES // 64} nodes")
    arms = {name: context(setting) for name, setting in ARMS.items()}
    t0 = time.perf_counter()
    first = next(iter(arms.values()))
    warm = torch.randn(1 << 18, 3, device=first.device)
    while time.perf_counter() - t0 < 1.0:   # clocks up
        first.knn_nodes(warm, warm[:256], 4)
        torch.cuda.synchronize()
    worst = 0.0
    for n in (int(s) for s in a.sizes.split(",")):
        worst = max(worst, case(n, [int(s) for s in a.nodes.split(",")], [int(s) for s in a.ks.split(",")], a.rounds, arms))
    for r in arms.values():
        r.close()
    if a.resources:
        for filt in ("k_deform_grad", "k_skin_nodes_grad"):
            say(f"kernel resources (tools/kernel_resources.py {filt}):")
            say(subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_resources.py"), filt], capture_output=True, text=True).stdout.rstrip())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if worst < 1e-4 else 1


if __name__ == "__main__":
    sys.exit(main())
