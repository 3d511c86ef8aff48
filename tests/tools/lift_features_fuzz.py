"""Differential fuzzer of feature lifting (Rasterizer.lift_features), in the style of obs_fuzz.py's lift arm.  Every expectation comes
from the C oracle through tests/tools/lift_features_ref.py and NumPy; nothing expected is a GPU output, and every comparison is exact
int64 equality.  Scenes and cameras are oracle_fuzz.py's recipes at sizes of this tool's own, from generator streams of its own; a
case is a function of its seed.

  scene      n in {1, 7, 50, 150}, splat scale over two decades, opacity bands, depth planes, SH degree -1..3, groups G in {1, 3, 8}
             with random rigid poses; one case in four POISONED (oracle_fuzz.poison_scene), and one in six with one Gaussian's
             opacity set to NaN or +Inf outright (obs_fuzz.LIFT_SEEDS_OPACITY_NOT_FINITE's kind: such a Gaussian is composited with
             alpha 0.999 wherever it is listed, and the lanes of a ragged tile beyond the image must still give it nothing)
  camera     1-3 views of draw_camera (inside the cloud, fx != fy, off-centre principal points, one in ten odd), W, H in 17..120,
             one case in ten a strip of 1000-3000 px by 1-16 px
  features   C in {1..20, 256}; N(0, 1), or N(0, 1) with 2 % of the values from {NaN, +-Inf, +-1e30, +-0.0, (m + 0.5) / scale};
             feature_scale 32767 / max|finite f| (the call's own choice, checked), or a power of two 2^13..2^16 under which part of
             the values saturate and the (m + 0.5) / scale are exact .5 ties
  mask       none / uniform per pixel / constant on 4x4 blocks (zeros and non-zero bytes other than 1)
  again      one case in four lifts a second set of images into the same buffers with the same scale

    python tests/tools/lift_features_fuzz.py [n_seeds] [first_seed]         (exit code 1 on any difference; prints each case)

Test infrastructure: lives under tests/ because it calls the oracle (the checker)."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lift_features_ref as fr  # noqa: E402
import lift_ref  # noqa: E402
import obs_fuzz as of  # noqa: E402
import oracle_fuzz as fz  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene, random_group_poses  # noqa: E402

SIZES = (1, 7, 50, 150)
GROUPS = (1, 3, 8)
SUITE_SEEDS = tuple(range(40))   # the cases tests/test_gpu_s_lift_features.py runs
SPECIALS = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0], np.float32)


def draw_case(seed: int) -> dict:
    rng = np.random.default_rng(377_000 + seed)
    n = int(rng.choice(SIZES, p=[0.1, 0.2, 0.35, 0.35]))
    ls = float(rng.uniform(np.log(0.003), np.log(0.3)))
    G = int(rng.choice(GROUPS))
    sc = make_scene(n, seed=388_000 + seed, log_scale_mean=ls, n_groups=G)
    fz.shape_scene(rng, sc)
    deg = int(rng.choice([-1, 0, 1, 2, 3, 3, 3]))
    W, H = int(rng.integers(17, 121)), int(rng.integers(17, 121))
    strip = bool(rng.random() < 0.1)
    if strip:
        W, H = fz.draw_strip(rng, (1000, 3001), (1000, 3001))
    poisoned = bool(rng.random() < 0.25)
    if poisoned:
        fz.poison_scene(rng, sc)
    not_finite = bool(rng.random() < 1.0 / 6.0)
    if not_finite:
        sc.opacities.reshape(-1)[int(rng.integers(0, n))] = np.float32([np.nan, np.inf][int(rng.integers(0, 2))])
    n_views = int(rng.integers(1, 4))
    odd = []
    cams = [fz.draw_camera(rng, W, H, odd) for _ in range(n_views)]
    poses = random_group_poses(G, seed=399_000 + seed, max_angle=0.6, max_shift=0.3)
    C = int(rng.choice(list(range(1, 21)) + [256] * 4))
    c = dict(seed=seed, scene=sc, deg=deg, n_groups=G, cams=cams, W=W, H=H, poisoned=poisoned, not_finite=not_finite, strip=strip,
             odd=any(odd), poses=[poses], C=C, features=str(rng.choice(["normal", "special"])),
             scale=str(rng.choice(["auto", "saturating"])), mask=str(rng.choice(["none", "uniform", "blocks"])),
             again=bool(rng.random() < 0.25), data_seed=int(rng.integers(0, 2 ** 31)))
    return c


def describe(c: dict) -> str:
    return (f"seed {c['seed']}: n={c['scene'].means.shape[0]} degree={c['deg']} groups={c['n_groups']} {c['W']}x{c['H']} views={len(c['cams'])} "
            f"C={c['C']} features={c['features']} scale={c['scale']} mask={c['mask']} again={c['again']}{' strip' if c['strip'] else ''}"
            f"{' odd-camera' if c['odd'] else ''}{' POISONED' if c['poisoned'] else ''}{' OPACITY-NOT-FINITE' if c['not_finite'] else ''}")


def inputs(c: dict) -> dict:
    """The images [sets][V,H,W,C], masks [sets][V,H,W] or None, and the scale (None: the call picks it) of a case."""
    rng = np.random.default_rng(c["data_seed"])
    V, W, H, C = len(c["cams"]), c["W"], c["H"], c["C"]
    sets = 2 if c["again"] else 1
    power = float(np.float32(2.0 ** int(rng.integers(13, 17))))   # the saturating scale: |f| beyond 4 .. 0.5 clamps
    tie_unit = np.float32(1.0 / power) if c["scale"] == "saturating" else np.float32(1.0)
    images, masks = [], []
    for _ in range(sets):
        f = rng.normal(size=(V, H, W, C)).astype(np.float32)
        if c["features"] == "special":
            flat = f.reshape(-1)
            k = max(1, flat.size // 50)
            at = rng.integers(0, flat.size, size=k)
            flat[at[: k // 2]] = SPECIALS[rng.integers(0, SPECIALS.size, size=k // 2)]
            flat[at[k // 2:]] = (rng.integers(-40, 40, size=k - k // 2) + 0.5).astype(np.float32) * tie_unit   # exact .5 ties under the saturating scale
        images.append(f)
        if c["mask"] == "none":
            masks.append(None)
        elif c["mask"] == "uniform":
            masks.append(rng.choice(np.array([0, 1, 255], np.uint8), size=(V, H, W)))
        else:
            b = rng.choice(np.array([0, 0, 1, 7], np.uint8), size=(V, (H + 3) // 4, (W + 3) // 4))
            masks.append(np.ascontiguousarray(np.repeat(np.repeat(b, 4, axis=1), 4, axis=2)[:, :H, :W]))
    scale = None
    if c["scale"] == "saturating" or c["again"]:   # (two calls into one buffer need one scale)
        scale = power if c["scale"] == "saturating" else fr.auto_scale(np.stack(images))
    return dict(images=images, masks=masks, scale=scale)


def reference(c: dict) -> dict:
    """dict(want, inp, notes) of a case, on the CPU."""
    sc = of.kit_scene(c, fz.scene_inputs(c))
    inp = inputs(c)
    n, W, H = len(sc["means"]), c["W"], c["H"]
    scale = inp["scale"] if inp["scale"] is not None else fr.auto_scale(inp["images"][0])
    sums, weight = np.zeros((n, c["C"]), np.int64), np.zeros(n, np.int64)
    weights = [lift_ref.weights_oracle(sc, (cm.viewmat, cm.K, W, H), c["poses"][0]) for cm in c["cams"]]
    for img, mask in zip(inp["images"], inp["masks"]):
        for v, w in enumerate(weights):
            s, wt = fr.sums(w, img[v], scale, None if mask is None else mask[v])
            sums += s
            weight += wt
    notes = dict(seen=int((weight > 0).sum()), saturated=int((np.abs(fr.quantise_features(inp["images"][0], scale)) == fr.FQ_MAX).sum()))
    return dict(want=dict(sums=sums, weight=weight, feature_scale=np.float64(scale)), inp=inp, notes=notes)


def run(r, c: dict, inp: dict) -> dict:
    sc = c["scene"]
    si = fz.scene_inputs(c)
    r.upload(sc.means, sc.opacities, si["colors"], quats=si["quats"], scales=si["scales"], covariances=si["cov"], sh_degree=c["deg"],
             group_id=sc.group_id, n_groups=c["n_groups"])
    r.set_group_poses(c["poses"][0])
    Vs, Ks = np.stack([cm.viewmat for cm in c["cams"]]), np.stack([cm.K for cm in c["cams"]])
    sums = weight = None
    for img, mask in zip(inp["images"], inp["masks"]):
        o = r.lift_features(Vs, Ks, c["W"], c["H"], img, feature_scale=inp["scale"], mask=mask, sums=sums, weight=weight)
        sums, weight = o["sums"], o["weight"]
    return dict(sums=sums.cpu().numpy(), weight=weight.cpu().numpy(), feature_scale=np.float64(o["feature_scale"]))


def run_case(r, c: dict) -> list:
    ref = reference(c)
    return of.compare(run(r, c, ref["inp"]), ref["want"])


def main(argv) -> int:
    from sim_a_splat_amd.rasterizer import Rasterizer
    n_seeds = int(argv[1]) if len(argv) > 1 else 300
    first = int(argv[2]) if len(argv) > 2 else 0
    r = Rasterizer(0)
    bad = 0
    for seed in range(first, first + n_seeds):
        c = draw_case(seed)
        diffs = run_case(r, c)
        print(describe(c), "->", "equal" if not diffs else "DIFFERENT: " + "; ".join(diffs), flush=True)
        bad += bool(diffs)
    r.close()
    print(f"{n_seeds} cases from seed {first}: {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
