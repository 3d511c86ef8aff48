"""The cases of the MCMC density-control tests (tests/test_mcmc_cpu.py, tests/test_gpu_y_mcmc.py): drawn scenes with every opacity a factor
2.5 away from ``min_opacity`` (mcmc_ref.decide asserts a factor two: two optimiser steps at fit_cases.LRS, which move an opacity by a tenth,
stay inside it), source opacities at most 0.99, drawn quaternions and anisotropic scales; and the float32 restatement's errors against
float64.

    python tests/tools/mcmc_cases.py        prints F32_ERR and NOISE_F32_ERR as they stand today

Sizes: 1 and 63 (less than a wave), 600 (three workgroups, a ragged last one, no multiple of 64), 65 795 = 256 * 257 + 3 (more workgroup
totals than the scan workgroup has lanes, several thousand draws across many workgroups)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(Path(__file__).resolve().parent)):
    if p not in sys.path:
        sys.path.insert(0, p)
import mcmc_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

MIN_OPACITY = 0.005
SEED = 11
DEAD_SHARE = 0.3
BIG = 256 * 257 + 3
# name -> (n, sh_degree, groups, kind)
CASES = {
    "n1": (1, 0, 0, "n1"),                          # one alive Gaussian, grow_factor 2: one draw
    "n63_sh3_groups": (63, 3, 3, "mix"),
    "n600_groups": (600, 0, 3, "mix"),
    "n600_sh3": (600, 3, 0, "mix"),
    "big": (BIG, 0, 0, "mix"),
    "grow_only": (600, 0, 0, "grow_only"),          # no dead
    "relocate_only": (600, 0, 3, "relocate_only"),  # cap_max <= N: N stays
    "partial_growth": (600, 3, 0, "partial"),       # N < cap_max < 1.05 N
    "nothing": (600, 0, 0, "nothing"),              # no dead and no room: D == 0
    "one_alive": (600, 0, 0, "one_alive"),          # copies + 1 far above 51, o' below min_opacity: the lower clamp binds
    "one_alive_opaque": (600, 0, 0, "one_alive_opaque"),   # ... an opacity of exactly 1: o' = 1, the upper clamp binds
    "dominated": (600, 0, 0, "dominated"),          # one opacity 0.99 among 0.011-s
}
NAMES = tuple(CASES)
CAMERA = dict(W=64, H=48, f=50.0, yaw=25.0, elev=0.2)
NOISE = dict(scale=10.0, step=3, seed=5)
NOISE_NAMES = ("n600_sh3", "n63_sh3_groups", "cov6")

# max |x32 - x64| / max |x64| over the sources' new opacities (clamped) and scales, per case: mcmc_ref.relocate in float32 against float64
# (float32_errors below; tests/test_mcmc_cpu.py holds the tables to it).  The GPU test's bounds are four times these; where the clamp binds
# on every source the figure is 0 and the GPU's opacity must be the clamp's own value.
F32_ERR = {
    "n1": dict(opacity=3.37e-07, scale=3.70e-07),
    "n63_sh3_groups": dict(opacity=5.33e-08, scale=7.26e-08),
    "n600_groups": dict(opacity=7.21e-08, scale=1.78e-06),
    "n600_sh3": dict(opacity=7.13e-08, scale=1.03e-06),
    "big": dict(opacity=8.07e-08, scale=2.11e-06),
    "grow_only": dict(opacity=5.86e-08, scale=9.70e-08),
    "relocate_only": dict(opacity=7.14e-08, scale=1.93e-07),
    "partial_growth": dict(opacity=6.67e-08, scale=2.59e-06),
    "one_alive": dict(opacity=0.00e+00, scale=1.26e-05),
    "one_alive_opaque": dict(opacity=0.00e+00, scale=1.00e+00),   # (the float32 sum of 51 rows at o' = 1 cancels to nothing: the GPU test holds this scale to the float64 restatement's BITS)
    "dominated": dict(opacity=4.59e-08, scale=6.14e-06),
}
# max |mean32 - mean64| / max |displacement64| of mcmc_ref.noise, per noise case
NOISE_F32_ERR = {
    "n600_sh3": 1.26e-06,
    "n63_sh3_groups": 1.02e-06,
    "cov6": 9.07e-07,
}


def _seed(name):
    return 700 + NAMES.index(name)


def case(name):
    """(scene in scene_cases' dict form, config dict for Rasterizer.mcmc_refine / mcmc_ref.refine)."""
    n, deg, G, kind = CASES[name]
    rng = np.random.default_rng(_seed(name))
    kk = (deg + 1) ** 2
    means = rng.normal(0.0, 0.45, (n, 3)).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    colors = rng.normal(0.0, 0.2, (n, kk, 3)).astype(np.float32)
    colors[:, 0] += 0.8
    scales = (rng.uniform(0.03, 0.2, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3))).astype(np.float32)
    dead_o, alive_o = rng.uniform(0.05, 0.4, n) * MIN_OPACITY, rng.uniform(2.5 * MIN_OPACITY, 0.9, n)
    if kind in ("mix", "relocate_only", "partial"):
        dead = rng.random(n) < DEAD_SHARE
        dead[0], dead[n - 1] = False, n > 1
    elif kind in ("one_alive", "one_alive_opaque"):
        dead = np.ones(n, bool)
        dead[n // 3] = False
        alive_o[n // 3] = 0.05 if kind == "one_alive" else 1.0
    elif kind == "dominated":
        dead = np.arange(n) % 6 == 1
        alive_o[:] = 0.011
        alive_o[n // 2] = 0.99
    else:
        dead = np.zeros(n, bool)
    op = np.where(dead, dead_o, alive_o).astype(np.float32)
    sc = dict(means=means, op=op, colors=colors, sh=deg, quats=quats, scales=scales, cov6=None, gid=None, G=0, Rt=None)
    if G:
        sc.update(gid=rng.integers(0, G, n).astype(np.uint8), G=G, Rt=sc_kit.random_group_poses(G, _seed(name), max_angle=1.0, max_shift=0.5))
    full = mcmc_ref.grow_count(n, 10 ** 9, 1.05)
    cfg = dict(min_opacity=MIN_OPACITY, seed=SEED, grow_factor=1.05, cap_max=1_000_000)
    if kind == "n1":
        cfg["grow_factor"] = 2.0
    elif kind in ("relocate_only", "nothing"):
        cfg["cap_max"] = n - 5
    elif kind == "partial":
        cfg["cap_max"] = n + full // 2
    return sc, cfg


def ref_scene(sc):
    """scene_cases' dict as mcmc_ref takes it."""
    n = np.asarray(sc["means"]).shape[0]
    return dict(means=sc["means"], opacities=sc["op"], colors=np.asarray(sc["colors"]).reshape(n, -1, 3), quats=sc["quats"], scales=sc["scales"],
                covariances=sc.get("cov6"), gid=sc["gid"])


def kit_scene(sc, new):
    """mcmc_ref's new scene back in scene_cases' form (float32), with sc's degree, groups and poses."""
    return dict(sc, means=np.asarray(new["means"], np.float32), op=np.asarray(new["opacities"], np.float32), colors=new["colors"], quats=new["quats"],
                scales=np.asarray(new["scales"], np.float32), gid=new["gid"])


_RUNS = {}


def reference(name, dtype=np.float64):
    """mcmc_ref.refine of the case (computed once per dtype, never changed)."""
    key = (name, np.dtype(dtype).name)
    if key not in _RUNS:
        sc, cfg = case(name)
        _RUNS[key] = mcmc_ref.refine(ref_scene(sc), cfg, dtype)
    return _RUNS[key]


def float32_errors(name):
    """dict(opacity=, scale=): max |x32 - x64| / max |x64| over the sources' new opacities and scales; None: the case has no source."""
    a, b = reference(name)["rel"], reference(name, np.float32)["rel"]
    if a is None:
        return None
    o64, s64 = exact_sources(name)
    rel = lambda x32, x64: float(np.abs(x32.astype(np.float64) - x64).max() / np.abs(x64).max())
    return dict(opacity=rel(b["o_new"], o64), scale=rel(b["s_new"], s64))


def exact_sources(name):
    """The sources' new opacities ``[m]`` (clamped) and scales ``[m,3]`` of the float64 restatement, NOT rounded to float32."""
    a = reference(name)["rel"]
    lo, hi = float(np.float32(MIN_OPACITY)), float(np.float32(1.0 - mcmc_ref.FLT_EPSILON))
    return np.clip(a["opacity"], lo, hi), a["ratio"][:, None] * case(name)[0]["scales"][a["sources"]].astype(np.float64)


def noise_scene(name):
    """The scene of a noise case in scene_cases' form: a refine case's, or fit_cases' cov6 scene with a third of its opacities made small."""
    if name != "cov6":
        return case(name)[0]
    import fit_cases
    sc = fit_cases.scene("cov6")
    op = sc["op"].copy()
    op[::3] = np.random.default_rng(9).uniform(0.001, 0.03, len(op[::3])).astype(np.float32)
    return dict(sc, op=op)


def noise_reference(name, dtype=np.float64):
    key = ("noise", name, np.dtype(dtype).name)
    if key not in _RUNS:
        _RUNS[key] = mcmc_ref.noise(ref_scene(noise_scene(name)), NOISE["scale"], NOISE["step"], NOISE["seed"], dtype)
    return _RUNS[key]


def noise_float32_error(name):
    m = np.asarray(noise_scene(name)["means"], np.float64)
    a, b = noise_reference(name), noise_reference(name, np.float32).astype(np.float64)
    return float(np.abs(b - a).max() / np.abs(a - m).max())


def camera():
    c = CAMERA
    return sc_kit.ring(c["W"], c["H"], f=c["f"], yaw=c["yaw"], elev=c["elev"])


if __name__ == "__main__":
    print("F32_ERR = {")
    for name in NAMES:
        e = float32_errors(name)
        if e is not None:
            print(f'    "{name}": dict(opacity={e["opacity"]:.2e}, scale={e["scale"]:.2e}),')
    print("}")
    print("NOISE_F32_ERR = {")
    for name in NOISE_NAMES:
        print(f'    "{name}": {noise_float32_error(name):.2e},')
    print("}")
    for name in NAMES:
        r = reference(name)
        print(f"# {name}: n {CASES[name][0]} -> {r['n']}, relocated {r['relocated']}, added {r['added']}, sources {int((r['copies'] > 0).sum())}, "
              f"most copies {int(r['copies'].max())}")
