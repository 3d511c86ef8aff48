"""The optimiser step on the resident scene beside the only alternative the library had before it: torch.optim.Adam on device tensors
followed by Rasterizer.upload (profiles/scene_fit.txt).

    python tools/fit_probe.py [--out FILE] [--small]

Two scenes: the 292 247-Gaussian stand-in at a 240x320 Gym camera, and config 3 (1 M Gaussians at 1920x1080); all five variable
groups are stepped, SH degree 3.  Per scene, in one process on one box, device-event times, the calls alternating, medians over the
rounds, after a warm-up that brings the clocks up (tools/ramp_probe.py):

  step alone          Rasterizer.adam_step on given gradients                 | torch Adam step + activations + upload
  whole iteration     render, L1 loss and its gradient, render_backward, step | the same with the torch step and the upload

The step's algorithmic bytes: the gradients read once, the moments and raw values of every group read and written, the planes read and
written (state rows are 16-byte: the means', opacities' and scales' carry 6 unused floats per Gaussian, counted)."""
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


def step_bytes(n, coeff_floats):
    planes = (coeff_floats + 3) // 4
    grads = 4 * (3 + 1 + 4 + 3 + coeff_floats)
    state = 16 * (2 + 1 + 2 + 3 + 2 * planes) * 2
    scene = 16 * (3 + planes) * 2
    return n * (grads + state + scene)


def case(name, n, seed, ls, G, W, H, f, rounds):
    sc = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=G)
    c = ring_camera(W, H, f)
    V, K = c.viewmat, c.K
    bg = (0.0, 0.0, 0.0)
    r = Rasterizer(0)
    up = dict(sh_degree=sc.sh_degree, group_id=sc.group_id, n_groups=G)
    r.upload(sc.means, sc.opacities, sc.sh, quats=sc.quats, scales=sc.scales, **up)
    target = r.render(V, K, W, H, bg)["rgb"].clone()
    dev = r.device
    # the scene a fit would start from: colours and opacities off
    start = dict(means=sc.means, opacities=sc.opacities * 0.7, colors=sc.sh * 0.8, quats=sc.quats, scales=sc.scales)
    r.upload(start["means"], start["opacities"], start["colors"], quats=start["quats"], scales=start["scales"], **up)
    step = [0]

    def grads_of(R):
        out = R.render(V, K, W, H, bg)
        _, g_rgb = fit.l1_loss_and_grad(out["rgb"], target, None)
        g_acc, g_a, _ = prechain(out["rgb"], out["alpha"], out["depth"], bg, g_rgb, None, None)
        return R.render_backward(V, K, W, H, g_acc, g_a, None, want=WHAT)

    acc = grads_of(r)

    def hip_step():
        step[0] += 1
        r.adam_step(acc, LRS, step[0])

    def hip_iteration():
        step[0] += 1
        r.adam_step(grads_of(r), LRS, step[0])

    # the alternative: raw parameters as torch tensors, torch.optim.Adam, activations, upload
    t32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    raw = dict(means=t32(start["means"]), opacities=torch.logit(t32(start["opacities"]).clamp(1e-6, 1 - 1e-6)), dc=t32(start["colors"][:, :1]),
               rest=t32(start["colors"][:, 1:]), quats=t32(start["quats"]), scales=torch.log(t32(start["scales"])))
    rate = dict(means="means", opacities="opacities", dc="sh_dc", rest="sh_rest", quats="quats", scales="scales")
    opt = torch.optim.Adam([dict(params=[p.requires_grad_(True)], lr=LRS[rate[k]]) for k, p in raw.items()], eps=1e-15)
    gid = None if sc.group_id is None else torch.tensor(sc.group_id, device=dev)

    def torch_step(g=None):
        g = acc if g is None else g
        with torch.no_grad():
            o, s = torch.sigmoid(raw["opacities"]), torch.exp(raw["scales"])
            raw["means"].grad, raw["quats"].grad = g["means"], g["quats"]
            raw["dc"].grad, raw["rest"].grad = g["colors"][:, :1], g["colors"][:, 1:]
            raw["opacities"].grad, raw["scales"].grad = g["opacities"] * o * (1 - o), g["scales"] * s
            opt.step()
            r.upload(raw["means"], torch.sigmoid(raw["opacities"]), torch.cat([raw["dc"], raw["rest"]], dim=1), quats=raw["quats"],
                     scales=torch.exp(raw["scales"]), sh_degree=sc.sh_degree, group_id=gid, n_groups=G)

    def torch_iteration():
        torch_step(grads_of(r))

    fwd = lambda: r.render(V, K, W, H, bg)
    bwd = lambda: grads_of(r)
    calls = {"forward frame (render)": fwd, "forward + loss + render_backward, five groups": bwd, "adam_step alone (k_adam_scene)": hip_step,
             "whole iteration with adam_step": hip_iteration, "torch Adam + activations + upload alone": torch_step,
             "whole iteration with torch Adam + upload": torch_iteration}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:   # clocks up
        fwd()
    for fn in calls.values():
        fn()
    res = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            res[k].append(timed(fn))
    kk = sc.sh.shape[1]
    say(f"== {name}: {n} Gaussians, SH degree {sc.sh_degree}, one view of {W}x{H}")
    say(f"{'ms, median of ' + str(rounds) + ' rounds [min..max]':52s} {'device events':>28s} {'call wall':>10s}")
    med = {}
    for k, rows in res.items():
        a = np.array(rows)
        m = np.median(a, axis=0)
        med[k] = m
        say(f"{k:52s} {m[0]:8.3f} [{a[:, 0].min():.3f}..{a[:, 0].max():.3f}] {m[1]:10.3f}")
    b = step_bytes(n, 3 * kk)
    ms = med["adam_step alone (k_adam_scene)"][0]
    say(f"step: {b / n:.0f} algorithmic bytes per Gaussian, {b / 1e9:.3f} GB; {b / (ms * 1e-3) / 1e12:.2f} TB/s achieved = "
        f"{100 * b / (ms * 1e-3) / 1e12 / ROOF_TBS:.0f} % of the {ROOF_TBS:.0f} TB/s roof (device events around the call: launch latency included)")
    say(f"step alone: torch + upload / adam_step = {med['torch Adam + activations + upload alone'][1] / med['adam_step alone (k_adam_scene)'][1]:.0f}x wall "
        f"({med['torch Adam + activations + upload alone'][0] / ms:.0f}x device events)")
    say(f"whole iteration: torch + upload / adam_step = {med['whole iteration with torch Adam + upload'][1] / med['whole iteration with adam_step'][1]:.1f}x wall; "
        f"the step is {100 * ms / med['whole iteration with adam_step'][0]:.0f} % of the iteration's device time")
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
