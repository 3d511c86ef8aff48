"""Differential fuzzer of the feature channels (sas_render_features) against the frame's own colour path.

    python tests/tools/feature_fuzz.py [--cases 1500] [--poisoned 300] [--seed 0] [--log profiles/features_fuzz.txt]
    SAS_LIB_PATH=variants/lib_bounds.so python tests/tools/feature_fuzz.py ...   (also reports the bounds counter)

Every drawn case (scene size 0..3000, splat groups or none, image 8..400 pixels a side, C in 1..40, a random camera)
checks one identity bit for bit:
  1  recolour: features in [0,1] -> clamp(F[..., o:o+3], 0, 1) equals the rgb of the scene recoloured with those three
     channels (sh_degree -1, background = the feature background's triple), on the production (lazy) path
  3  channel isolation: channel k of the C-channel frame equals the same column rendered alone (C = 1)
Every poisoned case (NaN, +-Inf, +-1e30 in a fifth of the features) checks that the frame equals the frame of the
features mapped as colours are (NaN -> -FLT_MAX, +-Inf -> +-FLT_MAX), comparing uint32 views.
Exit status 1 on any mismatch (or bounds violation).
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from sim_a_splat_amd import _capi  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402
from sim_a_splat_amd.synthetic import look_at_viewmat, intrinsics, make_scene, random_group_poses  # noqa: E402

FMAX = np.float32(3.402823466e38)


def draw(rng, case):
    n = int(rng.choice([0, 1, 2, int(rng.integers(3, 200)), int(rng.integers(200, 3001))]))
    G = int(rng.choice([0, 0, 2, 5]))
    s = make_scene(n, seed=case, log_scale_mean=float(np.log(rng.uniform(0.005, 0.08))), n_groups=G)
    G = G if s.group_id is not None else 0
    W, H = int(rng.integers(8, 401)), int(rng.integers(8, 401))
    f = float(rng.uniform(0.3, 1.5)) * max(W, H)
    eye = rng.normal(size=3)
    eye *= rng.uniform(0.5, 4.0) / np.linalg.norm(eye)
    V = look_at_viewmat(eye, target=rng.normal(0, 0.2, size=3))
    K = intrinsics(f, f * rng.uniform(0.8, 1.2), W * rng.uniform(0.3, 0.7), H * rng.uniform(0.3, 0.7))
    Rt = random_group_poses(G, seed=case + 7) if G else None
    return s, G, Rt, (V, K, W, H)


def upload(r, s, G, Rt, colors=None):
    r.upload(s.means, s.opacities, s.sh if colors is None else colors, quats=s.quats, scales=s.scales,
             sh_degree=s.sh_degree if colors is None else -1, group_id=s.group_id, n_groups=G)
    if G:
        r.set_group_poses(Rt)


def features(r, s, G, Rt, view, f, fbg=None):
    upload(r, s, G, Rt)
    r.upload_features(f)
    V, K, W, H = view
    return r.render_features(V, K, W, H, feature_background=fbg)["features"].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=1500)
    ap.add_argument("--poisoned", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    r = Rasterizer(0)
    bad, counts, t0 = [], {"recolour": 0, "isolation": 0, "poisoned": 0}, time.time()
    for case in range(a.cases + a.poisoned):
        rng = np.random.default_rng([a.seed, case])
        s, G, Rt, view = draw(rng, case)
        n = s.means.shape[0]
        V, K, W, H = view
        C = int(rng.integers(1, 41))
        if case >= a.cases:
            kind = "poisoned"
            f = rng.uniform(-2, 2, size=(n, C)).astype(np.float32)
            hit = rng.random(size=f.shape) < 0.2
            f[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), size=int(hit.sum()))
            mapped = np.where(np.isnan(f), -FMAX, np.clip(f, -FMAX, FMAX)).astype(np.float32)
            fbg = rng.uniform(-1, 1, size=C).astype(np.float32)
            ok = np.array_equal(features(r, s, G, Rt, view, f, fbg).view(np.uint32),
                                features(r, s, G, Rt, view, mapped, fbg).view(np.uint32))
        elif C >= 3 and rng.random() < 0.5:
            kind = "recolour"
            f = rng.uniform(0, 1, size=(n, C)).astype(np.float32)
            fbg = rng.uniform(0, 1, size=C).astype(np.float32)
            F = features(r, s, G, Rt, view, f, fbg)
            o = int(rng.integers(0, C - 2))
            upload(r, s, G, Rt, colors=np.ascontiguousarray(f[:, o:o + 3]))
            rgb = r.render(V, K, W, H, tuple(float(v) for v in fbg[o:o + 3]), want=("rgb",))["rgb"].cpu().numpy()
            ok = np.array_equal(rgb.view(np.uint32), np.clip(F[..., o:o + 3], 0, 1).view(np.uint32))
        else:
            kind = "isolation"
            f = rng.normal(size=(n, C)).astype(np.float32)
            F = features(r, s, G, Rt, view, f)
            k = int(rng.integers(0, C))
            one = features(r, s, G, Rt, view, np.ascontiguousarray(f[:, k:k + 1]))
            ok = np.array_equal(one[..., 0].view(np.uint32), F[..., k].view(np.uint32))
        counts[kind] += 1
        if not ok:
            bad.append(dict(case=case, kind=kind, n=n, C=C, W=W, H=H, groups=G))
    r.close()
    res = dict(cases=a.cases, poisoned=a.poisoned, seed=a.seed, by_identity=counts, mismatches=len(bad), first=bad[:5],
               lib=str(_capi.LIB_PATH.name), seconds=round(time.time() - t0, 1))
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        out = (ctypes.c_uint64 * 4)()
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.sas_debug_bounds(out, 0)
        res["bounds_violations"] = int(out[0])
    line = json.dumps(res)
    print(line)
    if a.log:
        with open(a.log, "a") as fh:
            fh.write(line + "\n")
    return 1 if bad or res.get("bounds_violations", 0) else 0


if __name__ == "__main__":
    sys.exit(main())
