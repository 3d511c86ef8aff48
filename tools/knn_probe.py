"""The k-nearest-neighbour search of sas_knn_points beside its own brute-force kernel and beside torch (profiles/knn.txt).

    python tools/knn_probe.py [--out FILE] [--sizes 20000,292247,1000000] [--rounds 5] [--torch-rows 16384] [--resources]

ONE process, two contexts on one box: the GRID arm is a default context (the grid the library chooses on the device, ring search, leftover
points through the brute-force kernel), the BRUTE arm is created under SAS_KNN_GRID=1 (every point through k_knn_brute).  The third arm is
chunked ``torch.cdist`` + ``topk(4, largest=False)`` on the same GPU; beyond ``--torch-rows`` query rows it is timed on that many rows
against the whole cloud and scaled by N / rows (marked).  The rounds alternate the arms; one warm-up round; medians and [min..max] over the
rounds, device events around each call, k = 3.  torch's distances come from the matrix form of cdist and are not exact; their largest
relative deviation from the library's is printed.  Per size a VOLUME cloud (the synthetic stand-in's centres: make_scene) and a SURFACE cloud (a
bumpy closed surface, as depth frames fuse to).  The grid and brute arms' results are compared bit for bit.

The verdict asked of the grid path: faster than the forced brute force at 292 247 and at 1 000 000 points by more than the spread."""
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
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def context(grid):
    old = os.environ.pop("SAS_KNN_GRID", None)
    if grid:
        os.environ["SAS_KNN_GRID"] = str(grid)
    try:
        return Rasterizer(0)
    finally:
        os.environ.pop("SAS_KNN_GRID", None)
        if old is not None:
            os.environ["SAS_KNN_GRID"] = old


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def surface(n, seed):
    """n points on a closed bumpy surface of radius about 1 (spherical harmonics-like bumps), float32."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rad = 1.0 + 0.15 * np.sin(5.0 * v[:, 0]) * np.cos(4.0 * v[:, 1]) + 0.1 * np.sin(7.0 * v[:, 2])
    return (v * rad[:, None]).astype(np.float32)


def torch_knn(p, rows, chunk=2048):
    """dist2 of the 3 nearest other points for the first ``rows`` points against all of p: cdist + topk, chunked."""
    out = []
    for a in range(0, rows, chunk):
        d = torch.cdist(p[a:min(a + chunk, rows)], p)   # (the matrix form |a|^2 + |b|^2 - 2 a.b: near distances lose digits, see the deviation)
        out.append(torch.topk(d, 4, dim=1, largest=False).values[:, 1:] ** 2)
    return torch.cat(out)


def case(n, kind, rounds, torch_rows, arms):
    pts = make_scene(n, seed=2).means if kind == "volume" else surface(n, 5)
    p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(arms["grid"].device)
    rows = min(n, torch_rows)
    t = {"grid": [], "brute": [], "torch": []}
    res, st = {}, {}
    for k in range(rounds + 1):
        for arm in ("grid", "brute", "torch"):   # the arms alternate inside every round
            if arm == "torch":
                ms, out = events(lambda: torch_knn(p, rows))
                ms *= n / rows
            else:
                ms, out = events(lambda: arms[arm].knn_points(p, 3))
                st[arm] = arms[arm].knn_stats()
            res[arm] = out
            if k:   # (the first round warms allocators and clocks up)
                t[arm].append(ms)
    same = torch.equal(res["grid"]["dist2"], res["brute"]["dist2"]) and torch.equal(res["grid"]["index"], res["brute"]["index"])
    ref = res["grid"]["dist2"][:rows]
    dev = float(((res["torch"] - ref).abs() / ref.clamp_min(1e-30)).max())
    med = {a: float(np.median(v)) for a, v in t.items()}
    g = st["grid"]
    say(f"== {n} points, {kind}; k = 3; medians of {rounds} rounds [min..max], ms; grid and brute arms {'identical bits' if same else 'DIFFER'}; "
        f"torch's squared distances deviate from them by up to {dev:.1e} (relative)")
    say(f"   grid {g['grid'][0]} x {g['grid'][1]} x {g['grid'][2]} cells (occupied coarse cells {g['occupied'][0]} of 32^3, {g['occupied'][1]} of 16^3), "
        f"leftover points {g['leftover']}")
    for a, label in (("grid", "grid path"), ("brute", "SAS_KNN_GRID=1 (brute force)"),
                     ("torch", "torch cdist + topk" + ("" if rows == n else f" ({rows} rows, x {n / rows:.1f})"))):
        say(f"   {label:44s} {med[a]:10.3f}   [{min(t[a]):.3f}..{max(t[a]):.3f}]   {med[a] / max(med['grid'], 1e-9):8.1f} x the grid path")
    wins = max(t["grid"]) < min(t["brute"])
    say(f"   grid against brute force: {'the slowest grid round is faster than the fastest brute-force round' if wins else 'NOT faster beyond the spread'}")
    say()
    return same, wins


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="20000,292247,1000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-rows", type=int, default=16384)
    ap.add_argument("--resources", action="store_true", help="append the kernels' registers, LDS and scratch (compiles the library once more)")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}")
    arms = {"grid": context(0), "brute": context(1)}
    t0 = time.perf_counter()
    m = torch.randn(1 << 18, 3, device=arms["grid"].device)
    while time.perf_counter() - t0 < 1.0:   # clocks up
        arms["grid"].knn_points(m, 3)
        torch.cuda.synchronize()
    verdicts = {}
    ok = True
    for n in (int(s) for s in a.sizes.split(",")):
        for kind in ("volume", "surface"):
            same, wins = case(n, kind, a.rounds, a.torch_rows, arms)
            ok = ok and same
            verdicts[(n, kind)] = wins
    asked = [k for k in verdicts if k[0] >= 292_247]
    say("verdict: the grid path beats the forced brute force beyond the run-to-run spread at " +
        (", ".join(f"{n} ({kind})" for n, kind in asked if verdicts[(n, kind)]) or "no asked size") +
        ("" if all(verdicts[k] for k in asked) else "; NOT at " + ", ".join(f"{n} ({kind})" for n, kind in asked if not verdicts[(n, kind)])))
    for r in arms.values():
        r.close()
    if a.resources:
        say("kernel resources (tools/kernel_resources.py k_knn):")
        say(subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_resources.py"), "k_knn"], capture_output=True, text=True).stdout.rstrip())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
