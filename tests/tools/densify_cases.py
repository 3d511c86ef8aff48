"""The cases of the density-control tests (tests/test_densify_cpu.py, tests/test_gpu_w_densify.py): drawn scenes, drawn statistics that
realise a drawn mix of classes with every value a factor 2.5 away from its threshold (densify_ref.decide asserts a factor two: two optimiser
steps at fit_cases.LRS, which move a scale by a per cent and an opacity by a tenth, stay inside it), and the float32
restatement's error of the children's means against float64.

    python tests/tools/densify_cases.py        prints F32_ERR as it stands today

Sizes: 1 and 63 (less than a wave), 600 (three workgroups, a ragged last one, no multiple of 64), 65 795 = 256 * 257 + 3 (more workgroup
totals than the scan workgroup has lanes)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(Path(__file__).resolve().parent)):
    if p not in sys.path:
        sys.path.insert(0, p)
import densify_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

CONFIG = dict(grow_grad2d=2e-4, grow_scale3d=0.05, prune_opacity=0.02, prune_scale3d=0.5, scene_extent=2.0, split_factor=1.6, seed=11)
GROW_SCALE, PRUNE_SCALE = CONFIG["grow_scale3d"] * CONFIG["scene_extent"], CONFIG["prune_scale3d"] * CONFIG["scene_extent"]
MIX = dict(clone=0.3, split=0.3, prune=0.2)
BIG = 256 * 257 + 3
# name -> (n, sh_degree, groups, kind, max_gaussians as a function of the uncapped plan or None)
CASES = {
    "n1": (1, 0, 0, "all_split"),
    "n63_sh3_groups": (63, 3, 3, "mix"),
    "n600_groups": (600, 0, 3, "mix"),
    "n600_sh3": (600, 3, 0, "mix"),
    "big": (BIG, 0, 0, "mix"),
    "nothing": (600, 0, 0, "nothing"),
    "all_split": (600, 0, 3, "all_split"),
    "all_but_one_pruned": (600, 0, 0, "all_but_one_pruned"),
    "cap_clones": (600, 0, 0, "cap_clones"),
    "cap_splits": (600, 3, 3, "cap_splits"),
}
NAMES = tuple(CASES)
CAMERA = dict(W=64, H=48, f=50.0, yaw=25.0, elev=0.2)

# max |x32 - x64| / max |x64| over the children's means, per case: densify_ref in float32 against float64 (float32_error below;
# tests/test_densify_cpu.py holds the table to it).  The GPU test's bound is four times these.
F32_ERR = {
    "n1": 1.06e-07,
    "n63_sh3_groups": 2.08e-07,
    "n600_groups": 1.92e-07,
    "n600_sh3": 2.31e-07,
    "big": 3.14e-07,
    "all_split": 3.08e-07,
    "cap_splits": 1.26e-07,
}


def _seed(name):
    return 500 + NAMES.index(name)


def _classes(name, n, rng):
    """The drawn class per Gaussian: 0 stays, 1 clone, 2 split, 3 pruned for opacity, 4 pruned for size, 5 split although huge."""
    kind = CASES[name][3]
    if kind == "nothing":
        return np.zeros(n, int)
    if kind == "all_split":
        return np.where(rng.random(n) < 0.2, 5, 2)
    if kind == "all_but_one_pruned":
        c = rng.choice([3, 4], n)
        c[n // 3] = 0
        return c
    u = rng.random(n)
    c = np.zeros(n, int)
    c[u < MIX["clone"]] = 1
    c[(u >= MIX["clone"]) & (u < MIX["clone"] + MIX["split"])] = 2
    pr = (u >= MIX["clone"] + MIX["split"]) & (u < MIX["clone"] + MIX["split"] + MIX["prune"])
    c[pr] = rng.choice([3, 4], int(pr.sum()))
    c[(c == 2) & (rng.random(n) < 0.15)] = 5
    return c


def case(name):
    """(scene in scene_cases' dict form, statistics dict of numpy arrays, config dict for Rasterizer.densify / densify_ref)."""
    n, deg, G, kind = CASES[name]
    rng = np.random.default_rng(_seed(name))
    cls = _classes(name, n, rng)
    kk = (deg + 1) ** 2
    means = rng.normal(0.0, 0.45, (n, 3)).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    colors = rng.normal(0.0, 0.2, (n, kk, 3)).astype(np.float32)
    colors[:, 0] += 0.8
    # the largest scale decides: small, between the two thresholds, or huge
    top = np.where(np.isin(cls, (1,)), rng.uniform(0.1, 0.4, n) * GROW_SCALE,
                   np.where(np.isin(cls, (4, 5)), rng.uniform(2.5, 3.5, n) * PRUNE_SCALE, rng.uniform(2.5 * GROW_SCALE, 0.4 * PRUNE_SCALE, n)))
    top = np.where((cls == 0) | (cls == 3), np.where(rng.random(n) < 0.5, rng.uniform(0.1, 0.4, n) * GROW_SCALE, top), top)
    scales = (top[:, None] * rng.uniform(0.3, 1.0, (n, 3))).astype(np.float32)
    scales[np.arange(n), rng.integers(0, 3, n)] = top.astype(np.float32)
    thr = CONFIG["prune_opacity"]
    op = np.where(cls == 3, rng.uniform(0.05, 0.4, n) * thr, rng.uniform(2.5 * thr, 0.9, n)).astype(np.float32)
    high = np.isin(cls, (1, 2, 5))
    count = rng.integers(1, 6, n).astype(np.int32)
    avg = np.where(high, rng.uniform(2.5, 10.0, n), rng.uniform(0.0, 0.4, n)) * CONFIG["grow_grad2d"]
    grad_sum = (avg * count).astype(np.float32)
    unseen = (~high) & (rng.random(n) < 0.2)   # never seen: a sum without a count does not make it `high`
    count[unseen] = 0
    grad_sum[unseen] = np.float32(1.0)
    sc = dict(means=means, op=op, colors=colors, sh=deg, quats=quats, scales=scales, cov6=None, gid=None, G=0, Rt=None)
    if G:
        sc.update(gid=rng.integers(0, G, n).astype(np.uint8), G=G, Rt=sc_kit.random_group_poses(G, _seed(name), max_angle=1.0, max_shift=0.5))   # (far apart: a frame shows who moved with whom)
    stats = dict(grad_sum=grad_sum, count=count, max_radius=np.zeros(n, np.float32))
    cfg = dict(CONFIG)
    if kind in ("cap_clones", "cap_splits"):
        pruned, cc, scand = densify_ref.decide(ref_scene(sc), stats, cfg)
        kept = int((~pruned).sum())
        cfg["max_gaussians"] = kept + (int(cc.sum()) // 2 if kind == "cap_clones" else int(cc.sum()) + int(scand.sum()) // 2)
    return sc, stats, cfg


def ref_scene(sc):
    """scene_cases' dict as densify_ref takes it."""
    n = np.asarray(sc["means"]).shape[0]
    return dict(means=sc["means"], opacities=sc["op"], colors=np.asarray(sc["colors"]).reshape(n, -1, 3), quats=sc["quats"], scales=sc["scales"], gid=sc["gid"])


def kit_scene(sc, new):
    """densify_ref's new scene back in scene_cases' form (float32), with sc's degree, groups and poses."""
    return dict(sc, means=np.asarray(new["means"], np.float32), op=new["opacities"], colors=new["colors"], quats=new["quats"], scales=new["scales"], gid=new["gid"])


_RUNS = {}


def reference(name, dtype=np.float64):
    """densify_ref.densify of the case (computed once per dtype, never changed)."""
    key = (name, np.dtype(dtype).name)
    if key not in _RUNS:
        sc, stats, cfg = case(name)
        _RUNS[key] = densify_ref.densify(ref_scene(sc), stats, cfg, dtype)
    return _RUNS[key]


def float32_error(name):
    """max |x32 - x64| / max |x64| over the children's means (None: the case splits nothing)."""
    a, b = reference(name), reference(name, np.float32)
    first = a["n_survivors"] + a["cloned"]
    if a["split"] == 0:
        return None
    x64, x32 = a["scene"]["means"][first:], b["scene"]["means"][first:].astype(np.float64)
    return float(np.abs(x32 - x64).max() / np.abs(x64).max())


def camera():
    c = CAMERA
    return sc_kit.ring(c["W"], c["H"], f=c["f"], yaw=c["yaw"], elev=c["elev"])


if __name__ == "__main__":
    print("F32_ERR = {")
    for name in NAMES:
        e = float32_error(name)
        if e is not None:
            print(f'    "{name}": {e:.2e},')
    print("}")
